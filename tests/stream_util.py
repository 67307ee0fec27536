"""A delayed producer for the stream-order tests (test_gpu_caller_stream.py): on a torch stream, a chain of ordinary element-wise torch operations on a
scratch tensor, then the copies that write a frame into the caller's planes.  A reader that is not ordered behind the stream finds the planes as they were
before the chain: the race is decided by milliseconds of GPU work, not by the host's timing.

The chain's length is calibrated once per process, with torch events on the GPU: the repeat count doubles until the chain ALONE takes between MIN_MS and MAX_MS.
  MIN_MS = 2    two orders of magnitude above the host time between a frame call and the launch of the first kernel that reads a plane
                (profiles/frame_properties_refactor.md: ~50 us of host time for the WHOLE enqueue of 15 launches, the head of the feature stage its first)
  MAX_MS = 10   half of GATE_STAND_DOWN (20 ms, lvt_amd/csrc/lvt_handover.h): no gate of a tracker that waits for the chain stands down, so its gate counters
                stay those of a handle that never waited
A chain that cannot be brought into the window fails the test with the measured time; nothing is skipped.  GPU only."""
import pytest

MIN_MS, MAX_MS = 2.0, 10.0
SCRATCH_WORDS = 32 << 20      # fp32 words the chain streams through per operation: every operation is bound by the GPU's memory, not by the host's launch rate

_state = {}


def _chain(scratch, reps):
    for _ in range(reps):
        scratch.mul_(1.0000001).add_(1e-9)


def _timed(stream, scratch, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        _chain(scratch, reps)
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate():
    """(scratch tensor, repeat count, measured ms), once per process"""
    if "reps" in _state:
        return _state["scratch"], _state["reps"], _state["ms"]
    import torch
    scratch = torch.ones(SCRATCH_WORDS, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    _timed(stream, scratch, 2)    # (the first launches load the kernels)
    reps, ms = 1, 0.0
    while True:
        ms = min(_timed(stream, scratch, reps) for _ in range(2))
        if ms >= MIN_MS or reps >= (1 << 16):
            break
        reps *= 2
    if not (MIN_MS <= ms <= MAX_MS):
        pytest.fail(f"delayed producer: {reps} repeats of the chain take {ms:.3f} ms on the GPU, outside [{MIN_MS}, {MAX_MS}] ms")
    print(f"delayed producer: {reps} repeats over {SCRATCH_WORDS * 4 >> 20} MiB take {ms:.3f} ms")
    _state.update(scratch=scratch, reps=reps, ms=ms)
    return scratch, reps, ms


def produce(stream, copies, delayed=True):
    """on `stream`: the calibrated chain (delayed), then dst.copy_(src) for every (dst, src) of `copies` -- device tensors, dst usually a view of a pitched
    plane.  Returns at once; nothing is synchronised"""
    import torch
    scratch, reps, _ = calibrate() if delayed else (None, 0, 0.0)
    with torch.cuda.stream(stream):
        if delayed:
            _chain(scratch, reps)
        for dst, src in copies:
            dst.copy_(src, non_blocking=True)


def pending_marker(stream):
    """an event behind everything enqueued on `stream` so far: marker.query() is False while the producer has not finished"""
    import torch
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev
