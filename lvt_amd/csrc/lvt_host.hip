// lvt_host.hip -- host side of the MI355X-native LVT tracking path: context/arena management, the fixed
// per-frame launch chain, the reference-compatible C-ABI (include/lvt_c.h) and the additive entry
// points (include/lvt_amd_ext.h).  The host mirrors lvt_system::create/track/reset
// (reference lvt/src/lvt_system.cpp) but performs NO tracking arithmetic: the whole state machine
// runs on the device, the host enqueues the chain and reads back one result record per frame.
//
// Three HIP streams form a software pipeline: the FEATURE stage (k_score .. k_brief, wide kernels) runs up
// to two frames ahead on stream_f; the TRACKING chain (matching of the newest map points, the serial Levenberg-Marquardt pose
// refinement, map maintenance -- latency-bound, a few workgroups) runs frame after frame on `stream`; the EARLY stream starts the
// next frame's map matching the moment a frame's pose exists and builds the row-match candidate lists.  Feature buffers are
// triple buffered; the streams hand over through sequence numbers polled by one-wave gate kernels (LVT_AMD_ORDERING=events: event
// barriers instead).  Results land in a ring of pinned records with completion flags the host polls, so frames can be enqueued
// asynchronously (lvt_amd_track_device_async / lvt_amd_wait).
#define LVT_EXPORT_FUNCTIONS
#include "../../include/lvt_amd_ext.h"

#include "k_features.hip"
#include "k_track.hip"
#include "k_hamming.hip"
#include "k_lists.hip"
#include "k_rectify.hip"
#include "k_reduce.hip"
#include "k_sensor.hip"
#include "k_depthreg.hip"
#include "k_equalise.hip"
#include "k_depthguard.hip"
#include "k_mask.hip"
#include "k_labelmask.hip"
#include "k_state.hip"
#include "k_poseinfo.hip"
#include "k_reloc.hip"
#include "lvt_odometry.h"

#include <atomic>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <functional>
#include <vector>

namespace lvt {

#define HIPCHK(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            (ctx)->set_error(std::string(#call) + ": " + hipGetErrorString(e__));          \
            throw std::runtime_error((ctx)->err);                                          \
        }                                                                                  \
    } while (0)

constexpr int EXT_MAX = 16384;
// workgroups of k_candidates<ROW> on the early stream: 256 of them (one per CU, as on the feature stream) cost 6 % of the frame
// rate -- they share SIMDs and LDS with the single-workgroup kernels of the tracking chain running beside them; 16 make the kernel
// itself too slow (measured: 24 / 32 / 40 / 48 / 64 / 256 -> 8 180 / 8 330 / 8 320 / 8 270 / 8 240 / 7 840 frames/s)
constexpr int ROW_BLOCKS = 32;
constexpr int MATCH_BLOCKS_GATED = 16;  // k_match_map when it polls for the early stream itself (single sequence): see k_track.hip (8 / 16 / 32: 8 840 / 8 890 / 8 900 frames/s; fewer parked workgroups leave more CUs to other processes on the GPU)
constexpr int ROW_BLOCKS_BATCH = 16;  // per sequence of a lock-step batch (16 sequences: 8 / 16 / 32 / 64 / 256 -> 30.8k / 36.9k / 35.8k / 35.0k / 31.1k frames/s)
constexpr int RING = 8;  // frames that may be in flight / un-collected
// workgroups per sequence of the binned list kernels (k_lists.hip: equal parts of the queries; LVT_AMD_LISTS_WGS=row,map overrides).  Measured in round 4
// (64 sequences, HIP-event time of the row-list launch): 2 / 8 / 16 workgroups per sequence = 113 / 151 / 241 us; lock-step batches of 16 / 32 sequences
// 68.5k / 88.8k, 68.2k / 82.4k, 59.2k / 77.1k frames/s -- every workgroup stages the whole train set again, and from 32 sequences on the chip is full anyway
constexpr int LISTS_WGS_ROW = 2, LISTS_WGS_MAP = 1;
// handles per DEVICE whose k_match_map may poll for the early stream itself: each parks MATCH_BLOCKS_GATED workgroups with 50 KB of LDS;
// 4 x 16 of them still leave most CUs with the 159 KB a k_cells workgroup needs, more handles use the separate one-wave gate kernel
constexpr int MAX_FOLDED_GATES = 4;

// first kernel of the feature stage of a BATCH: publish every sequence's inputs (a single sequence gets them as a kernel
// argument of k_score)
__global__ void k_feat_begin(const Seq *seqs, const FrameArgs *fa, int par) {
    if (threadIdx.x != 0) return;
    feat_begin(seq_const(seqs, blockIdx.x), fa[blockIdx.x], par);
}
// the same with the sequences' inputs in the kernel's own arguments (up to FEAT_PACK sequences): no read of pinned host memory over PCIe at the head of the feature stage
constexpr int FEAT_PACK = 32;
struct FrameArgsPack {
    FrameArgs a[FEAT_PACK];
};
static_assert(sizeof(Seq *) + sizeof(FrameArgsPack) + sizeof(int) + 2 * sizeof(seq_t) < 4096, "k_feat_begin_pack's arguments must stay under 4096 bytes");
// ... and with k_gate_buf's wait in front (want != 0: the tracking chain of the frame that used this buffer last must have released it): one launch at the head of a
// batch's feature stage instead of two
__global__ void k_feat_begin_pack(const Seq *seqs, FrameArgsPack pk, int par, seq_t want) {
    if (threadIdx.x != 0) return;
    const Seq &S = seq_const(seqs, blockIdx.x);
    if (want) gate_buf_wait(S, want, par);
    const FrameArgs f = pk.a[blockIdx.x];
    feat_begin(S, f, par);
}

// tightly packed host-layout images (stride == cols) -> pitched device images.
// Host images enter through a pinned staging buffer -- or, when the caller's buffer is page-locked itself, in place -- that this
// kernel reads over PCIe and writes as the pitched planes k_score wants: blockIdx.y = image.  One launch replaces two pageable H2D
// copies + two re-pitch kernels (0.32 ms per stereo pair -> see DESIGN.md section 6).  The source may start at ANY byte address and
// hold any byte count (1241 x 376 = 466 616 is 8 mod 16): bytes up to the first 16-byte boundary and behind the last whole vector
// travel one by one, everything between as aligned 16-byte loads -- no load reaches outside [src, src + n).
__global__ __launch_bounds__(256) void k_stage_in(const uint8_t *src0, const uint8_t *src1, uint8_t *dst0, uint8_t *dst1, int W, int H, int pitch) {
    stage_in_body(blockIdx.y ? src1 : src0, blockIdx.y ? dst1 : dst0, W, H, pitch, (size_t)blockIdx.x * blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}
// the (unpitched) depth image, T = float (fp32 metres) or uint16_t (raw sensor units; the plane stays 16-bit in HBM): 16-byte loads between the first 16-byte
// boundary of the source and its last whole vector, single elements on either side -- no load reaches outside [src, src + n); the destination is written
// element by element (it is 16-byte aligned, the source need only be aligned to its element: head < 16 / sizeof(T), and n - tail0 < 16 / sizeof(T), elements)
template <typename T>
__global__ __launch_bounds__(256) void k_stage_copy(const T *src, T *dst, size_t n) {
    constexpr size_t PER = 16 / sizeof(T);
    union Vec {
        uint4 q;
        T e[PER];
    };
    const size_t head = min((size_t)(((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T)), n);
    const size_t nv = (n - head) / PER, tail0 = head + nv * PER;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t v = t0; v < nv; v += stride) {
        Vec u;
        u.q = *reinterpret_cast<const uint4 *>(src + head + v * PER);
        T *d = dst + head + v * PER;
#pragma unroll
        for (size_t k = 0; k < PER; k++) d[k] = u.e[k];
    }
    if (t0 < head) dst[t0] = src[t0];
    if (t0 < n - tail0) dst[tail0 + t0] = src[tail0 + t0];
}
// pull a tightly packed depth plane of n elements (format fmt) into d_dst, which is sized for fp32
static void launch_stage_copy(hipStream_t st, const uint8_t *src, float *d_dst, size_t n, int fmt) {
    if (fmt == DEPTH_U16) hipLaunchKernelGGL(k_stage_copy<uint16_t>, dim3(256), dim3(256), 0, st, reinterpret_cast<const uint16_t *>(src), reinterpret_cast<uint16_t *>(d_dst), n);
    else hipLaunchKernelGGL(k_stage_copy<float>, dim3(256), dim3(256), 0, st, reinterpret_cast<const float *>(src), d_dst, n);
}

// handles alive in this process: a handle whose k_match_map polls for its early stream parks 32 workgroups (50 KB of LDS each)
// on the GPU; with many handles on one device that would leave no CU with enough free LDS for the 159-KB k_cells workgroups
// they are waiting for -- beyond 4 handles the separate one-wave gate kernel is used again (enqueue_frame)
// Counted PER DEVICE: handles on different GPUs of one process share no hardware queue and no CU.
constexpr int MAX_DEVICES = 64;
static std::atomic<int> g_live_contexts[MAX_DEVICES];

// An lvt_handle is either a Context (a sequence, or a lock-step batch, with its own launch chain) or a PoolSlot (lvt_pool.h: one sequence of a
// lock-step batch SHARED by the pooled handles of a device); the first word tells them apart.
constexpr uint64_t CTX_MAGIC = 0x4C56545F43545831ull, SLOT_MAGIC = 0x4C56545F534C5431ull;

// EuRoC pre-step (k_rectify.hip): the maps of one camera.  Stand-alone (lvt_amd_rectify[_device]) or attached to a tracker, whose feature stage then
// starts with k_rectify_frames (lvt_amd_set_rectifiers)
struct Rectifier {
    int w = 0, h = 0, pitch = 0;                 // the DESTINATION (the maps' size) and the pitch of d_dst
    int sw = 0, sh = 0;                          // the SOURCE: the raw image, lens.width x lens.height
    lvt_amd_lens lens = {};                      // the record it was made from (lvt_amd_rectifier_get_info)
    int device = 0;                              // the HIP device the maps live on
    float *d_map1 = nullptr, *d_map2 = nullptr;
    int2 *d_fix = nullptr;                       // both maps interleaved, 1/32-px fixed point (k_rectify_fix): what k_rectify_frames reads
    uint8_t *d_src = nullptr, *d_dst = nullptr;  // staging for the host-buffer entry point
};

// pinned staging of one frame's host planes, [image | image or depth], each part padded to 16 B: what the host writes and what the device pulls
struct HostStage {
    uint8_t *h = nullptr, *dev = nullptr;  // the same memory as the host / the device addresses it
    size_t second = 0;                     // offset of the second plane (the bytes reserved per 8-bit image, a 16-B multiple)
};

struct Context {
    uint64_t magic = CTX_MAGIC;
    double host_enq_us = 0, host_wait_us = 0;  // host time spent enqueueing / blocking (LVT_AMD_HOST_TIMING=1 prints it at destroy)
    long host_enq_n = 0, host_wait_n = 0;
    int gate_timeouts_seen = 0, gate_fatal_seen = 0;
    // a gate that ran into its time limit means that the streams do not run side by side (a tool serialises the dispatches, or the streams share a
    // hardware queue): the handle then moves to event ordering by itself, once, at the next frame it enqueues (unless LVT_AMD_ORDERING=polling insists)
    bool want_events = false, ordering_forced = false;
    hipEvent_t ev_switch = nullptr, ev_switch_e = nullptr;
    long test_gate_timeout = 0, switched_at = -1;  // LVT_AMD_TEST_GATE_TIMEOUT=n: the early gate of frame n reports a time-out
    long long planes_in_place = 0, planes_staged = 0;  // host-buffer entry points: image / depth planes read in place (page-locked caller buffers) / copied through the staging buffer
    int device = 0;            // the HIP device that owns every allocation, stream and event of this handle (recorded at creation)
    int B = 1;                 // sequences advanced in lock-step by one launch chain
    int launch_seqs = 0;       // > 0: the NEXT step is launched for the first launch_seqs sequences only (a pool with empty upper seats)
    int ring_seqs[8] = {};     // ... and what every un-collected step was launched for
    int sensor = 1;
    Params prm{};
    // A MIXED batch (lvt_amd_batch_create_mixed): sequence s has its own parameters prms[s] (image size, intrinsics, detection grid, radii, thresholds);
    // prm and pitch are then sequence 0's (what the sequence-0 read-back calls use).  k_score / k_cells take their work from the two tables
    // (build_mixed_tables); every other kernel of the chain is per-sequence by blockIdx.z and reads Seq::prm.  A uniform batch has mixed == false,
    // empty tables and exactly the launches it had before mixed batches existed.
    bool mixed = false;
    std::vector<Params> prms;            // mixed: [B]; otherwise empty
    std::vector<lvt_amd_params> in_prms; // what the caller handed in: [B] (mixed) or [1]
    uint32_t *d_score_tab = nullptr, *d_cells_tab = nullptr;
    int n_score_wgs = 0, n_cells_wgs = 0;
    // per-launch decisions over the batch's sequences (a uniform context: its one parameter set's values)
    bool any_staged = false, any_strips = false;
    int max_cells = 0;
    const Params &seq_prm(int s) const { return mixed ? prms[s] : prm; }
    hipStream_t stream = nullptr;    // tracking chain
    hipStream_t stream_f = nullptr;  // feature stage
    hipStream_t stream_e = nullptr;  // early part of find_matches of the next frame (behind the previous frame's k_pnp)
    bool own_stream = false;
    // A CALLER'S stream (lvt_amd_set_stream: own_stream == false).  The caller's planes are read on stream_f, so every step records ev_caller on `stream` at its
    // head and stream_f waits for it: what the caller enqueued on its stream before the frame call has completed before any kernel of the frame reads a plane.
    // The event lands behind the previous frame's tracking chain on the same stream: such a handle's feature stage no longer runs ahead of its tracking.  Created
    // by the first lvt_amd_set_stream; a handle on its private stream never records or waits for it.
    hipEvent_t ev_caller = nullptr;
    std::vector<void *> allocs;
    const Seq *d_seqs = nullptr;  // written ONCE, by create_context, from h_seqs; no kernel and no later host code writes it (lvt_dev.h: SeqArg)
    std::vector<Seq> h_seqs;   // host mirror (device pointers inside)
    std::vector<Ctl *> d_ctl;
    Ctl *h_ctl = nullptr;          // pinned, RING x B records
    Ctl *h_ctl_dev = nullptr;      // the same memory as the device sees it (k_triangulate writes each frame's record there)
    // completion flags, pinned + coherent, RING x B: k_triangulate stores the frame's sequence number behind its record and the
    // host polls it -- an event record on the tracking stream costs that stream 3-4 us per frame (measured), and nothing else
    // on the device needs the event in the normal mode
    seq_t *h_done = nullptr, *h_done_dev = nullptr;
    // synchronous calls: k_pnp hands the pose over as soon as it exists (PoseRec + flag, same pinned scheme), the call returns on it
    // and the frame's tail finishes behind the caller's next upload; the frame is collected (full record) by the next entry point
    PoseRec *h_pose = nullptr, *h_pose_dev = nullptr;
    seq_t *h_pose_done = nullptr, *h_pose_done_dev = nullptr;
    bool binned_lists = false; // lock-step batches: k_hamming_batched_lists builds the early map lists and the row lists (LVT_AMD_BINNED_LISTS=0 / 1)
    bool early_pose = true;    // LVT_AMD_SYNC_TAIL=wait: synchronous calls return only when the whole frame is done
    bool early_pending = false;  // the last synchronous call returned on its early pose: its frame is still un-collected (and is nobody's to wait for)
    FrameArgs *h_fargs = nullptr;  // pinned, RING x B
    // POSE UNCERTAINTY (lvt_amd_enable_pose_info): an enabled handle launches k_pose_info behind k_pnp, which writes every sequence's record of the frame into
    // its slot of this ring (pinned + coherent, RING x B, beside h_ctl; allocated by the first enable).  The frame's completion flag is released by a later
    // kernel of the same stream, so a collected frame's record is complete.  Not state: snapshots neither hold nor restore it.
    bool pose_info = false;
    lvt_amd_pose_info *h_pinfo = nullptr, *h_pinfo_dev = nullptr;
    hipEvent_t ev_done[RING] = {};  // the only events of the normal mode: the streams hand over through polling gates (k_gate*)
    // LVT_AMD_ORDERING=events: the streams are ordered by event barriers only and the early stream is not used (the tracking chain
    // does all the matching).  Slower (~6 300 instead of ~7 000 frames/s), but free of kernels that wait for another queue's
    // kernels -- required under tools that serialise the dispatches of all queues (rocprofv3 --pmc): a polling gate then holds
    // the only dispatch slot while what it waits for cannot start.
    bool events_only = false;
    CellOrder cell_order;   // detection cells by decreasing area: the order a batch's k_cells workgroups start in
    // A batch's k_score is thousands of small workgroups: while its grid is being dispatched, every CU slot that frees up goes to the next of them, and the
    // tracking / early chains' workgroups (56 - 133 KB of LDS each) wait until it is through (rocprofv3 timeline: k_match_map 57 - 64 us beside it, 12 alone).
    // In TWO launches the chip drains once in the middle and they get in: +4 .. 8 % for 8 - 24 KITTI-shaped sequences, -6 % from 28 on, where the feature
    // stage is the longer chain and the drain is pure loss.  Which side a batch is on shows in its own early gate (Ctl::dbg[32 / 35 / 33]: start, features
    // seen, pose seen): a gate that mostly waits for the previous pose says the feature stream is ahead.  LVT_AMD_SCORE_PIECES=1 / 2 fixes the choice.
    bool feat_pack = true;     // LVT_AMD_NO_FEAT_PACK (set to anything): a batch's inputs go through pinned host memory (k_feat_begin) behind a k_gate_buf launch of their own
    int brief_from_image = 0;  // LVT_AMD_BRIEF_FROM_IMAGE=1: no box-sum plane; k_brief_img builds the 9 x 9 sums of a key point's patch in LDS (k_features.hip)
    int score_pieces = 1;
    bool score_pieces_auto = true;
    double gate_balance_us = 0;  // running mean of (wait for the pose) - (wait for the features)
    // raw corners a k_cells workgroup holds in LDS.  A batch with more cell workgroups than CUs (16 KITTI-shaped sequences: 320 on 256) runs them with room for
    // RAW_CAP_SMALL corners -- 80 KB of LDS instead of 159, TWO workgroups per CU (k_cells is held to 64 VGPRs for that: at 66 it ran one per CU whatever its LDS) --
    // and a cell with more raw corners than that takes the exact global-memory path, as one beyond RAW_CAP does (LVT_AMD_CELLS_RAW_CAP overrides)
    int cells_raw_cap = RAW_CAP;
    unsigned cell_token = 0;  // one per k_cells launch, never reset: what a split cell's helper workgroups publish their survivors under
    int cell_split = 2;     // workgroups a single sequence's tall detection cell is cut into (cells_work_split; LVT_AMD_CELL_SPLIT=0 | 2 | 3)
    int lists_wgs_row = LISTS_WGS_ROW, lists_wgs_map = LISTS_WGS_MAP;
    int match_blocks_batch = 32;   // workgroups per sequence of a batch's k_match_map (it lists the points appended since the early part: none on most frames,
                                   // and every workgroup's thread 0 recomputes the prediction before it can leave): 256 -> 32 = +6 % frames/s at 16 sequences
                                   // (LVT_AMD_MATCH_BLOCKS_BATCH overrides)
    bool force_row_fallback = false;  // LVT_AMD_TEST_ROW_FALLBACK=1 (tests): k_triangulate does not wait for the early stream's row lists, it builds them itself
                                      // WHILE the early stream's kernel writes the same words -- the situation its 5-ms time-out leads to
    hipEvent_t ev_feat[NPAR] = {};
    hipEvent_t ev_depth = nullptr;  // RGB-D host-buffer calls: the depth plane is pulled on the early stream beside the feature kernels; k_gather waits for it
    bool depth_wait = false;
    std::function<void()> before_gather;  // host work to run once the detection kernels are enqueued (the RGB-D depth upload)
    // owned staging for the host-buffer entry points, per feature buffer
    uint8_t *d_img[NPAR][2] = {};
    HostStage stage[NPAR];  // pinned staging of host images (lvt_track): [left | right or depth]
    float *d_depth[NPAR] = {};
    // asynchronous host-buffer calls (lvt_amd_track_async / lvt_amd_track_rgbd_async): one image set and one staging buffer per RING slot -- frame t's
    // slot was last used by frame t - RING, which make_room() has collected, so neither the pull (a write) nor the CPU copy into the staging
    // buffer needs a device-side hand-over.  The pull kernel runs at the head of the frame's feature stage, on the feature stream: a stream of its own
    // (4 400 against 8 100 frames/s), the null stream or other priorities (6 100) and the copy engine (5 600) were measured and removed
    // (profiles/r04_async_host.md; the variants are in the history at 7f39175).
    uint8_t *d_img_ring[RING][2] = {};
    float *d_depth_ring[RING] = {};
    HostStage stage_ring[RING];
    long long async_frames = 0;
    // A stereo frame handed to lvt_amd_track_async is HELD until the next one arrives (or somebody waits for it): the held frame's k_cells launch then carries
    // the workgroups that pull the NEXT frame's images (k_features.hip, NextPull), and a frame whose images came that way starts without a pull of its own.
    struct PendingFrame {
        bool valid = false, pulled = false;
        FrameArgs f{};
        const uint8_t *src[2] = {nullptr, nullptr};
        uint8_t *dst[2] = {nullptr, nullptr};
        int row_bytes = 0, rows = 0, pitch = 0;  // the pulled planes: bytes per row (n_cols, times bpp on a colour handle), rows and their pitch
    } pend;
    NextPull next_pull{};   // what this enqueue_frame's k_cells pulls (src[0] == nullptr: nothing)
    bool fuse_pull = true;  // LVT_AMD_FUSED_PULL=0: every frame pulls its own images at the head of its feature stage
    long long fused_pulls = 0;
    int feature_cus = 0;    // CUs the feature stream is confined to (0: all; lock-step batches, see create_context)
    float *d_ext[NPAR][2] = {};
    // RAW stereo frames (lvt_amd_set_rectifiers / lvt_amd_batch_set_rectifiers): a sequence with a pair of rectifiers attached takes raw images through every
    // stereo entry point.  The entry points work as for rectified frames -- their FrameArgs name the raw planes (the caller's, or the staged ones) --, and
    // enqueue_frame puts ONE k_rectify_frames launch at the head of the feature stage that writes the sequence's own rectified planes (per feature-buffer
    // parity) and points the frame at them.  Borrowed: the rectifiers outlive the handle or are detached first.
    std::vector<Rectifier *> rect;     // [B][2], nullptr: none (empty until the first attach)
    std::vector<uint8_t *> d_rect;     // [B][NPAR][2] rectified planes, each sequence's own pitch
    int n_rect = 0;                    // sequences with rectifiers
    bool has_rect(int s) const { return n_rect > 0 && rect[2 * (size_t)s] != nullptr; }
    // THE FRAME'S SIZE of sequence s: what every stereo entry point takes.  The sequence's own img_width x img_height, or, with rectifiers attached, their
    // SOURCE size (both eyes' are equal: set_rectifiers) -- the raw image need not have the tracker's size ("LENS MODELS", include/lvt_amd_ext.h).  Everything
    // allocated or sized by the frame's bytes follows it (staging, the host entry points' planes, the colour and converted planes); everything behind the
    // rectified plane stays at the sequence's size.  `resized`: the two differ -- only then does anything here allocate or launch differently.
    // With a REDUCTION in force (lvt_amd_set_reduction, below) there are three sizes: the FRAME (the record's width x height, what the entry points take), the
    // BASE (the reduced plane: the rectifiers' source where a pair is attached, else the sequence's) and the sequence's.  Without one the frame IS the base.
    int base_W(int s) const { return has_rect(s) ? rect[2 * (size_t)s]->sw : seq_prm(s).W; }
    int base_H(int s) const { return has_rect(s) ? rect[2 * (size_t)s]->sh : seq_prm(s).H; }
    int frame_W(int s) const { return has_reduce(s) ? red[(size_t)s].width : base_W(s); }
    int frame_H(int s) const { return has_reduce(s) ? red[(size_t)s].height : base_H(s); }
    bool resized(int s) const { return (has_rect(s) || has_reduce(s)) && (frame_W(s) != seq_prm(s).W || frame_H(s) != seq_prm(s).H); }
    // pitch of the context's own gray planes of sequence s at the frame's size (a resized sequence: its own; otherwise plane_pitch, as ever)
    int frame_pitch(int s) const { return resized(s) ? (frame_W(s) + 63) / 64 * 64 : h_seqs[(size_t)s].plane_pitch; }
    // ... and of its reduced planes, at the base size: what frame_pitch is to a sequence with rectifiers alone
    int base_pitch(int s) const { return (base_W(s) != seq_prm(s).W || base_H(s) != seq_prm(s).H) ? (base_W(s) + 63) / 64 * 64 : h_seqs[(size_t)s].plane_pitch; }
    // LARGE frames (lvt_amd_set_reduction / lvt_amd_batch_set_reduction): a sequence with a reduction takes frames of the record's width x height through every
    // frame-taking entry point.  As for colour frames the FrameArgs name the large planes (the caller's, or the context's own pulled ones), and enqueue_frame puts
    // ONE k_reduce_frames launch at the head of the feature stage -- behind the conversion, ahead of the rectify block -- that writes the sequence's own reduced
    // planes (per feature-buffer parity, the base size) and points the frame at them.  A property of the handle, not state: reset and snapshots leave it alone.
    std::vector<lvt_amd_reduction> red;  // [B] (empty until the first set); factor < 2: none
    std::vector<uint8_t *> d_red;        // [B][NPAR][2] reduced planes, each sequence's base_pitch (an RGB-D sequence: eye 0 only)
    std::vector<size_t> red_bytes;       // [B] bytes each of the sequence's reduced planes holds (0: none)
    int n_reduce = 0;                    // sequences with a reduction
    bool ring_reduced[RING] = {};        // per un-collected / last frame: sequence 0's image went through k_reduce_frames (lvt_amd_get_plane(.., 9, ..))
    bool has_reduce(int s) const { return n_reduce > 0 && red[(size_t)s].factor >= 2; }
    // the host entry points of a RESIZED handle pull gray raw images into these planes instead of d_img / d_img_ring (allocated when first needed, at the
    // source's size; given back when the frame's size changes: frame_planes_release)
    uint8_t *d_raw[NPAR][2] = {};
    uint8_t *d_raw_ring[RING][2] = {};
    // COLOUR frames (lvt_amd_set_pixel_format / lvt_amd_batch_set_pixel_format): a sequence with a colour format takes interleaved colour images through every
    // frame-taking entry point.  As for raw frames the FrameArgs name the colour planes (the caller's, or the context's own pulled ones), and enqueue_frame puts
    // ONE k_gray_frames launch at the head of the feature stage -- ahead of the rectify block -- that writes the sequence's own gray planes and points the frame at them.
    std::vector<int> pixfmt;           // [B] LVT_AMD_PIX_* (empty until the first colour set: every sequence gray)
    std::vector<uint8_t *> d_gray;     // [B][NPAR][2] converted planes, each sequence's frame_pitch (an RGB-D sequence: eye 0 only)
    std::vector<size_t> gray_bytes;    // [B] bytes each of the sequence's converted planes holds (0: none yet)
    int n_colour = 0;                  // sequences with a colour format
    bool ring_converted[RING] = {};    // per un-collected / last frame: sequence 0's image went through k_gray_frames (what lvt_amd_get_plane(.., 3, ..) may read back)
    int fmt_of(int s) const { return n_colour > 0 ? pixfmt[(size_t)s] : PIX_GRAY8; }
    // SENSOR formats (lvt_amd_set_sensor_format / lvt_amd_batch_set_sensor_format): a sequence with one takes the sensor's plane -- a Bayer mosaic, YUV 4:2:2,
    // 16-bit gray -- through every frame-taking entry point.  It takes the colour formats' route and their planes (a sequence has one or the other, never
    // both): the FrameArgs name the sensor's plane, and enqueue_frame puts ONE k_sensor_frames launch in k_gray_frames' place that writes d_gray and points
    // the frame at it; a MONO16 sequence with an auto window gets k_sensor_hist and k_sensor_levels in front.  A property of the handle, not state.
    std::vector<lvt_amd_sensor_format> sens;  // [B] (empty until the first set); format == 0: none
    std::vector<uint32_t *> d_sens_hist;      // [B] 2 x 4096 bins of a sequence with an auto window (zero between frames: k_sensor_levels clears them)
    int *d_sens_win = nullptr;                // [RING][B][2 eyes][lo, hi]: the windows k_sensor_levels found, per un-collected frame (allocated with the first auto window)
    std::vector<uint8_t> sens_mapped;         // [RING][B] != 0: the sequence's frame of that step went through k_sensor_frames as MONO16
    int n_sensor = 0, n_sensor_auto = 0;      // sequences with a sensor format / with an auto window
    bool has_sensor(int s) const { return n_sensor > 0 && sens[(size_t)s].format != SENSOR_NONE; }
    bool has_sensor_auto(int s) const { return has_sensor(s) && sens[(size_t)s].format == SENSOR_MONO16 && sens[(size_t)s].auto_window != 0; }
    // "this sequence converts": it has a colour or a sensor format -- its frames are byte images bpp_of(s) * width wide that a launch at the head of the feature
    // stage turns into d_gray (a Bayer sequence converts at one byte per pixel)
    bool converts(int s) const { return fmt_of(s) != PIX_GRAY8 || has_sensor(s); }
    int bpp_of(int s) const { return has_sensor(s) ? sensor_bpp(sens[(size_t)s].format) : pix_bpp(fmt_of(s)); }
    // host entry points of a colour handle pull the colour bytes -- a byte image n_cols * bpp wide -- into these planes (allocated when first needed, sized for
    // 4 bytes per pixel): per feature buffer for the synchronous calls, per RING slot for the asynchronous ones
    uint8_t *d_col[NPAR][2] = {};
    uint8_t *d_col_ring[RING][2] = {};
    int colour_pitch() const { return (frame_W(0) * bpp_of(0) + 63) / 64 * 64; }
    // UNREGISTERED DEPTH (lvt_amd_set_depth_camera / lvt_amd_batch_set_depth_camera): a sequence with a depth camera takes its depth plane as the sensor
    // delivers it -- the camera's size, either format -- through every RGB-D entry point.  As for colour frames the FrameArgs name the sensor's plane (the
    // caller's, or the context's own pulled one), and enqueue_frame registers it into the sequence's own fp32 plane (k_depth_clear at the head of the feature
    // stage, k_depth_register in front of k_gather) and points the frame at that.  A property of the handle, not state: snapshots neither hold nor restore it.
    std::vector<lvt_amd_depth_camera> depth_cam;  // [B] (empty until the first set); width == 0: none
    std::vector<float *> d_reg;                   // [B][NPAR] registered planes, fp32, plane_pitch words per row
    int n_depth_cam = 0;                          // sequences with a depth camera
    bool ring_registered[RING] = {};              // per un-collected / last frame: sequence 0's depth went through k_depth_register (lvt_amd_get_plane(.., 4, ..))
    bool has_depth_cam(int s) const { return n_depth_cam > 0 && depth_cam[(size_t)s].width > 0; }
    // DIM frames (lvt_amd_set_equalisation / lvt_amd_batch_set_equalisation): a sequence with an equalisation record has the gray plane its detector would read --
    // behind the conversion and the remap -- equalised by two launches at the head of the feature stage (k_clahe_lut, k_clahe_apply), into planes of its own the
    // frame is then pointed at.  A property of the handle, not state: reset and snapshots leave it alone.
    std::vector<lvt_amd_equalisation> equal;  // [B] (empty until the first set); tiles_x == 0: none
    std::vector<uint8_t *> d_eq;              // [B][NPAR][2] equalised planes, each sequence's own pitch (an RGB-D sequence: eye 0 only)
    std::vector<uint8_t *> d_eq_lut;          // [B][2] the tables of a sequence's eye: 16 x 16 x 256 bytes.  ONE copy: the writer (k_clahe_lut) and the reader
                                              // (k_clahe_apply) of frame t and the writer of frame t + 1 are on the same in-order stream
    int n_equal = 0;                          // sequences with the property
    bool ring_equalised[RING] = {};           // per un-collected / last frame: sequence 0's image went through k_clahe_apply (lvt_amd_get_plane(.., 5, ..))
    bool has_equal(int s) const { return n_equal > 0 && equal[(size_t)s].tiles_x > 0; }
    // FEATURE MASKS (lvt_amd_set_mask / lvt_amd_batch_set_mask and their _device forms): a sequence with a mask has the key points k_gather kept filtered by ONE
    // k_mask_features launch between k_gather and k_brief.  The planes are the tracker's own copies, per EYE and not per parity: a set needs a quiet handle, so
    // no frame in flight ever reads a plane that is being written.  A property of the handle, not state: reset and snapshots leave it alone.
    std::vector<uint8_t *> d_mask;            // [B][2] u8 planes, each sequence's own pitch (allocated at the first set, kept across an unset)
    std::vector<uint8_t> mask_on;             // [B][2] != 0: the eye has a mask (empty until the first set)
    int n_mask = 0;                           // sequences with a mask on either eye
    bool ring_masked[RING] = {};              // per un-collected / last frame: the step went through k_mask_features under the masks the handle has now
    bool has_mask(int s, int e) const { return n_mask > 0 && mask_on[(size_t)s * 2 + e] != 0; }
    // LABEL MASKS (lvt_amd_set_label_mask / lvt_amd_batch_set_label_mask, lvt_amd_frame_labels / _device): a sequence with a record may be handed a label image per
    // eye for its NEXT frame, with frames in flight.  The attachment waits in a ring beside h_fargs, in the slot that frame will use and TAGGED with its number
    // (enq + 1 at its enqueue_frame): a frame held in `pend` has its number already and never takes the labels meant for the frame behind it.  enqueue_frame puts
    // ONE k_label_mask launch at the head of the feature stage that builds the plane (per feature-buffer parity) k_mask_features then filters that eye with.
    // The record is a property of the handle, not state: reset and snapshots leave it alone (a reset drops a pending attachment).
    struct LabelAttach {
        long long frame = 0;                  // the frame number the images belong to; 0: nothing attached
        const uint8_t *src[2] = {nullptr, nullptr};  // device addresses (the caller's planes, or this slot's own copies); nullptr: the eye has no labels
        int pitch[2] = {0, 0};
    };
    std::vector<lvt_amd_label_mask> label;    // [B] (empty until the first set); label_width == 0: none
    std::vector<uint8_t *> d_lmask;           // [B][NPAR][2] built planes, each sequence's own pitch
    std::vector<LabelAttach> label_ring;      // [RING][B]
    std::vector<uint8_t> label_built;         // [RING][B][2] != 0: the step built a plane for the eye (what k_mask_features of that step was handed)
    std::vector<uint8_t *> h_lab_stage, d_lab_ring;  // [B] host calls: RING x 2 label images, page-locked / in HBM (allocated by the sequence's first host call)
    int n_label = 0;                          // sequences with a record
    bool has_label(int s) const { return n_label > 0 && label[(size_t)s].label_width > 0; }
    bool built_label(int slot, int s, int e) const { return !label_built.empty() && label_built[((size_t)slot * B + s) * 2 + e] != 0; }
    // DEPTH GUARD (lvt_amd_set_depth_guard / lvt_amd_batch_set_depth_guard): an RGB-D sequence with a record has the key points k_gather kept filtered by ONE
    // k_depth_guard launch directly behind k_gather, ahead of k_mask_features.  A property of the handle, not state: reset and snapshots leave it alone.
    std::vector<lvt_amd_depth_guard> depth_guard;  // [B] (empty until the first set; radius 0: the sequence has none)
    int n_guard = 0;                          // sequences with a guard
    bool ring_guarded[RING] = {};             // per un-collected / last frame: the step went through k_depth_guard under the records the handle has now
    bool has_guard(int s) const { return n_guard > 0 && depth_guard[(size_t)s].radius > 0; }
    // the depth plane the host entry points of sequence 0 take: the camera's size where one is set, else the image's
    size_t depth_px() const { return has_depth_cam(0) ? (size_t)depth_cam[0].width * depth_cam[0].height : (size_t)prm.W * prm.H; }
    int depth_cols() const { return has_depth_cam(0) ? depth_cam[0].width : prm.W; }
    size_t depth_cap = 0, depth_ring_cap = 0;     // pixels d_depth[] / d_depth_ring[] hold
    int pitch = 0;
    RelocBufs reloc{};             // relocalisation: the call's own buffers (allocated by the first call; reloc.work == nullptr before it)
    int *d_snap_status = nullptr;  // snapshots: [B][4] map_cur, map_n, staged_cur, staged_n as k_state_pack found them (allocated by the first take)
    long enq = 0, done = 0;    // frames enqueued / collected
    long delivered = 0;        // frames whose record delivery has been enqueued (k_triangulate, the next frame's k_gate_late, or k_deliver)
    bool sync_call = false;    // the frame being enqueued is collected right away: k_triangulate delivers its record itself
    int last_slot = 0, last_par = 0;
    std::string err;
    // optional per-kernel timing with HIP events on the launch streams (lvt_amd_profile_*)
    bool prof = false;
    static constexpr int PROF_SLOTS = 33;
    hipEvent_t ev[PROF_SLOTS][2] = {};
    bool ev_used[PROF_SLOTS] = {};
    double prof_ms[PROF_SLOTS] = {};
    long prof_calls[PROF_SLOTS] = {};

    void set_error(const std::string &s) { err = s; }
    // A capacity report is its frame's own (include/lvt_c.h).  It stays until it has been read through lvt_amd_last_error AND a later frame has been collected
    // that fits: a caller that reads the string every N frames still learns of a cut, one that reads it after every frame sees each frame's own report.
    // (Every other report -- HIP errors, gate time-outs -- stays until the next one, as before.)
    long long ovf_done = -1, ovf_read_done = -1;  // `done` behind the frame that set the report / at the last read of it
    bool capacity_report() const { return err.compare(0, 17, "capacity overflow") == 0; }

    template <typename T>
    T *dalloc_uncached(size_t n) {  // device memory no cache holds (MTYPE UC): what one workgroup stores, another of the same launch may read without fences
        void *p = nullptr;
        size_t bytes = ((n * sizeof(T) + 255) / 256) * 256;
        if (bytes == 0) bytes = 256;
        HIPCHK(this, hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached));
        HIPCHK(this, hipMemset(p, 0, bytes));
        allocs.push_back(p);
        return static_cast<T *>(p);
    }
    template <typename T>
    T *dalloc(size_t n) {
        void *p = nullptr;
        size_t bytes = ((n * sizeof(T) + 255) / 256) * 256;
        if (bytes == 0) bytes = 256;
        HIPCHK(this, hipMalloc(&p, bytes));
        zero_now(p, bytes);
        allocs.push_back(p);
        return static_cast<T *>(p);
    }
    // hipMemset of device memory goes to the NULL stream and may return before it has run; the streams of a single sequence are non-blocking, i.e. not ordered
    // behind the NULL stream.  Buffers are also allocated with frames in flight (the image ring of the asynchronous host calls, one slot per frame for the first
    // RING frames): the pull launched into a fresh plane a few microseconds later must not be overtaken by the plane's own clear
    void zero_now(void *p, size_t bytes) {
        HIPCHK(this, hipMemset(p, 0, bytes));
        HIPCHK(this, hipStreamSynchronize(nullptr));
    }

    void dfree(void *p) {  // give a dalloc'ed buffer back before the context ends (nullptr: nothing)
        if (!p) return;
        for (size_t i = 0; i < allocs.size(); i++)
            if (allocs[i] == p) {
                allocs.erase(allocs.begin() + (long)i);
                (void)hipFree(p);
                return;
            }
    }

    bool counted = false;
    void count_in(int dev) {
        device = dev;
        g_live_contexts[dev % MAX_DEVICES].fetch_add(1);
        counted = true;
    }
    int live_on_device() const { return g_live_contexts[device % MAX_DEVICES].load(); }
    Context() {}
    ~Context() {
        if (counted) g_live_contexts[device % MAX_DEVICES].fetch_sub(1);
        if (stream || !own_stream) (void)hipStreamSynchronize(stream);  // (a caller's stream may be NULL, the legacy default stream: the chain on it ends before its buffers go)
        if (stream_f) (void)hipStreamSynchronize(stream_f);
        if (stream_e) (void)hipStreamSynchronize(stream_e);
        for (void *p : allocs) (void)hipFree(p);
        for (auto &x : stage_ring) if (x.h) (void)hipHostFree(x.h);
        for (auto &e : ev)
            for (auto &x : e)
                if (x) (void)hipEventDestroy(x);
        for (auto &x : ev_done) if (x) (void)hipEventDestroy(x);
        for (auto &x : ev_feat) if (x) (void)hipEventDestroy(x);
        if (ev_depth) (void)hipEventDestroy(ev_depth);
        if (ev_switch) (void)hipEventDestroy(ev_switch);
        if (ev_switch_e) (void)hipEventDestroy(ev_switch_e);
        if (ev_caller) (void)hipEventDestroy(ev_caller);
        for (auto &x : stage) if (x.h) (void)hipHostFree(x.h);
        for (uint8_t *x : h_lab_stage) if (x) (void)hipHostFree(x);
        if (h_ctl) (void)hipHostFree(h_ctl);
        if (h_done) (void)hipHostFree(h_done);
        if (h_pose) (void)hipHostFree(h_pose);
        if (h_pose_done) (void)hipHostFree(h_pose_done);
        if (h_fargs) (void)hipHostFree(h_fargs);
        if (h_pinfo) (void)hipHostFree(h_pinfo);
        if (stream && own_stream) (void)hipStreamDestroy(stream);
        if (stream_f) (void)hipStreamDestroy(stream_f);
        if (stream_e) (void)hipStreamDestroy(stream_e);
    }
};

// A handle belongs to the device that was current when it was created (or the one named to lvt_amd_create_on_device).  Every entry
// point makes that device current for the duration of the call and restores the caller's: a thread-per-GPU process can
// drive its handles from any thread without calling hipSetDevice itself.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(const Context *c) {
        int cur = -1;
        if (c && hipGetDevice(&cur) == hipSuccess && cur != c->device && hipSetDevice(c->device) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// ---- parameters ---------------------------------------------------------------------------------
static bool derive_params(const lvt_amd_params &in, int sensor, Params &p) {
    if (in.img_width <= 0 || in.img_height <= 0 || in.detection_cell_size <= 0 || in.max_keypoints_per_cell <= 0 ||
        in.tracking_radius <= 0 || in.agast_threshold <= 0)
        return false;  // the reference asserts these (lvt_image_features_handler.cpp:88-93)
    std::memset(&p, 0, sizeof(p));
    p.fx = in.fx, p.fy = in.fy, p.cx = in.cx, p.cy = in.cy, p.baseline = in.baseline;
    p.k1 = in.k1, p.k2 = in.k2, p.p1 = in.p1, p.p2 = in.p2, p.k3 = in.k3;
    p.near_plane = in.near_plane_distance, p.far_plane = in.far_plane_distance;
    p.tri_ratio = in.triangulation_ratio_test_threshold;
    p.track_ratio = in.tracking_ratio_test_threshold;
    p.desc_th = in.descriptor_matching_threshold;
    p.W = in.img_width, p.H = in.img_height;
    p.min_matches = in.min_num_matches_for_tracking;
    p.tracking_radius = in.tracking_radius;
    p.cell_size = in.detection_cell_size;
    p.max_kp_cell = in.max_keypoints_per_cell;
    p.agast_th = in.agast_threshold;
    p.agast_th_low = (int)((double)in.agast_threshold * 0.5 + 0.5);  // handler.cpp:165
    p.untracked_th = in.untracked_threshold;
    p.staged_th = in.staged_threshold;
    p.tri_policy = in.triangulation_policy;
    p.sensor = sensor;
    // detection grid -- handler.cpp:95-114
    p.cells_y = 1 + ((p.H - 1) / p.cell_size);
    p.cells_x = 1 + ((p.W - 1) / p.cell_size);
    p.n_cells = p.cells_x * p.cells_y;
    if (p.n_cells > CELLS_MAX) return false;
    if (std::min(p.cell_size, p.W) > CELL_SIDE_MAX || std::min(p.cell_size, p.H) > CELL_SIDE_MAX) return false;  // (k_features.hip: 12-bit cell-local keys)
    // matching hash grid -- struct.cpp:47-53
    const float kc = (float)HASH_CELL;
    p.hash_ccx = (int)std::ceil(p.W / kc);
    p.hash_ccy = (int)std::ceil(p.H / kc);
    p.cell_search_radius = (p.tracking_radius == HASH_CELL) ? 1 : (int)std::ceil((float)p.tracking_radius / kc);
    // image bounds -- lvt_local_map.cpp:84-123 (per instance)
    if (std::fabs(p.k1) < 1e-5) {
        p.min_x = 0.0f, p.max_x = (float)p.W, p.min_y = 0.0f, p.max_y = (float)p.H;
    } else {
        float x[4], y[4];
        undistort_point(p, 0.0f, 0.0f, x[0], y[0]);
        undistort_point(p, (float)p.W, 0.0f, x[1], y[1]);
        undistort_point(p, 0.0f, (float)p.H, x[2], y[2]);
        undistort_point(p, (float)p.W, (float)p.H, x[3], y[3]);
        p.min_x = std::min(x[0], x[2]);
        p.max_x = std::max(x[1], x[3]);
        p.min_y = std::min(y[0], y[1]);
        p.max_y = std::max(y[2], y[3]);
    }
    p.undistort = (std::fabs(p.k1) > 1e-5) ? 1 : 0;
    p.cell_magic = (unsigned)((0x100000000ull + (unsigned long long)p.cell_size - 1) / (unsigned long long)p.cell_size);
    p.big_cell_strips = (p.cell_size > BIG_CELL_SIDE) ? 1 : 0;  // (TUM's single 2000-px cell; the 250-px cells of KITTI / EuRoC keep the two-launch feature chain)
    return true;
}

static void default_params(lvt_amd_params *p) {  // lvt_parameters.cpp:29-52
    std::memset(p, 0, sizeof(*p));
    p->fx = p->fy = p->cx = p->cy = 0.5f;
    p->near_plane_distance = 0.1f;
    p->far_plane_distance = 500.0f;
    p->triangulation_ratio_test_threshold = 0.60f;
    p->tracking_ratio_test_threshold = 0.80f;
    p->descriptor_matching_threshold = 30.0f;
    p->min_num_matches_for_tracking = 10;
    p->tracking_radius = 25;
    p->agast_threshold = 25;
    p->untracked_threshold = 10;
    p->staged_threshold = 2;
    p->detection_cell_size = 250;
    p->max_keypoints_per_cell = 150;
    p->triangulation_policy = 1;
}

// minimal reader for the reference's flat `%YAML:1.0` configs (lvt_parameters.cpp:54-93): every field
// is overwritten; a key that is missing reads as 0 (cv::FileNode default), reals round to ints.
static bool params_from_file(const char *fname, lvt_amd_params *p) {
    FILE *f = fname ? std::fopen(fname, "r") : nullptr;
    if (!f) return false;
    std::vector<std::pair<std::string, double>> kv;
    char line[1024];
    while (std::fgets(line, sizeof(line), f)) {
        char *hash = std::strchr(line, '#');
        if (hash) *hash = 0;
        char *colon = std::strchr(line, ':');
        if (!colon || line[0] == '%') continue;
        std::string key(line, colon - line);
        size_t a = key.find_first_not_of(" \t"), b = key.find_last_not_of(" \t");
        if (a == std::string::npos) continue;
        key = key.substr(a, b - a + 1);
        char *end = nullptr;
        double v = std::strtod(colon + 1, &end);
        if (end == colon + 1) continue;
        kv.emplace_back(key, v);
    }
    std::fclose(f);
    auto get = [&](const char *k) -> double {
        for (auto &e : kv)
            if (e.first == k) return e.second;
        return 0.0;
    };
    auto geti = [&](const char *k) -> int { return (int)std::nearbyint(get(k)); };
    p->fx = (float)get("fx"), p->fy = (float)get("fy"), p->cx = (float)get("cx"), p->cy = (float)get("cy");
    p->k1 = (float)get("k1"), p->k2 = (float)get("k2"), p->p1 = (float)get("p1"), p->p2 = (float)get("p2"), p->k3 = (float)get("k3");
    p->baseline = (float)get("baseline");
    p->img_width = geti("img_width"), p->img_height = geti("img_height");
    p->near_plane_distance = (float)get("near_plane_distance");
    p->far_plane_distance = (float)get("far_plane_distance");
    p->triangulation_ratio_test_threshold = (float)get("triangulation_ratio_test_threshold");
    p->tracking_ratio_test_threshold = (float)get("tracking_ratio_test_threshold");
    p->min_num_matches_for_tracking = geti("min_num_matches_for_tracking");
    p->tracking_radius = geti("tracking_radius");
    p->agast_threshold = geti("agast_threshold");
    p->untracked_threshold = geti("untracked_threshold");
    p->staged_threshold = geti("staged_threshold");
    p->descriptor_matching_threshold = (float)get("descriptor_matching_threshold");
    p->detection_cell_size = geti("detection_cell_size");
    p->max_keypoints_per_cell = geti("max_keypoints_per_cell");
    p->triangulation_policy = geti("triangulation_policy");
    return true;
}

// ---- context creation ---------------------------------------------------------------------------
static void alloc_feat(Context *c, Feat &F) {
    F.x = c->dalloc<float>(NF_MAX), F.y = c->dalloc<float>(NF_MAX), F.resp = c->dalloc<float>(NF_MAX);
    F.bx = c->dalloc<float>(NF_MAX), F.by = c->dalloc<float>(NF_MAX), F.depth = c->dalloc<float>(NF_MAX);
    F.desc = c->dalloc<uint64_t>((size_t)NF_MAX * 4);
    F.flag = c->dalloc<uint8_t>(NF_MAX);
    F.hcx = c->dalloc<int16_t>(NF_MAX), F.hcy = c->dalloc<int16_t>(NF_MAX);
    F.n = c->dalloc<int>(1);
}
static void alloc_points(Context *c, MapSoA &P, int cap) {
    P.pos = c->dalloc<double>((size_t)cap * 3);
    P.desc = c->dalloc<uint64_t>((size_t)cap * 4);
    P.counter = c->dalloc<int>(cap), P.age = c->dalloc<int>(cap), P.match_idx = c->dalloc<int>(cap);
}

static void drain(Context *c);

// the record of a sequence that has not tracked yet, with the chain words this context's next frame expects (nothing pending): what lvt_system::reset leaves,
// and what an applied snapshot takes its chain words from (k_state.hip)
// the pose-uncertainty records of sequence s: status 0 until the next tracked frame (reset, restore, enable)
static void pose_info_clear(Context *c, int s) {
    if (!c->h_pinfo) return;
    for (int r = 0; r < RING; r++) std::memset(&c->h_pinfo[(size_t)r * c->B + s], 0, sizeof(lvt_amd_pose_info));
}
static Ctl fresh_ctl(const Context *c) {
    Ctl z;
    std::memset(&z, 0, sizeof(z));
    z.state = 1;
    z.last_matches[0] = z.last_matches[1] = z.last_matches[2] = 0x7FFFFFFF;
    z.last_pose.q[0] = 1.0;
    z.mm_last_q[0] = 1.0;
    z.mm_ang_vel[0] = 1.0;
    z.optimized.q[0] = z.predicted.q[0] = 1.0;
    z.out_R[0] = z.out_R[4] = z.out_R[8] = 1.0;
    z.out_status = 1;
    z.pnp_seq = (seq_t)c->enq;  // the next frame's gate waits for this value: nothing is pending
    z.early_state = early_word((seq_t)c->enq, EARLY_NOTHING);
    z.track_done_seq = (seq_t)c->enq;
    z.late_gate_seq = (seq_t)c->enq;
    z.gate_timeouts = c->gate_timeouts_seen, z.gate_fatal = c->gate_fatal_seen;  // (the host compares these running counters with what it has seen)
    return z;
}
static void reset_state(Context *c, int only = -1) {  // lvt_system::reset (lvt_system.cpp:44-68); only >= 0: that sequence of a batch alone
    drain(c);
    if (only < 0) c->gate_timeouts_seen = 0, c->gate_fatal_seen = 0;
    if (only < 0 && c->capacity_report()) c->err.clear();  // (the frames it spoke of are gone)
    for (int s = 0; s < c->B; s++) {
        if (only >= 0 && s != only) continue;
        const Ctl z = fresh_ctl(c);
        HIPCHK(c, hipMemcpyAsync(c->d_ctl[s], &z, sizeof(Ctl), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(c->h_seqs[s].map_n, 0, sizeof(int), c->stream));
        HIPCHK(c, hipMemsetAsync(c->h_seqs[s].map_cur, 0, sizeof(int), c->stream));
        HIPCHK(c, hipMemsetAsync(c->h_seqs[s].staged_n, 0, sizeof(int), c->stream));
        HIPCHK(c, hipMemsetAsync(c->h_seqs[s].staged_cur, 0, sizeof(int), c->stream));
        for (int r = 0; r < RING; r++) c->h_ctl[r * c->B + s] = z;
        pose_info_clear(c, s);
        for (int r = 0; r < RING && !c->label_ring.empty(); r++) c->label_ring[(size_t)r * c->B + s] = Context::LabelAttach{};  // (a pending attachment goes with the frames)
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
}

// The work tables of a mixed batch (k_score_mixed / k_cells_mixed, k_features.hip), one 32-bit entry per workgroup.  Pure host code.
//  cells: (sequence << 16 | eye << 8 | cell) for every detection cell of every image (an RGB-D sequence has one image), by NON-INCREASING cell area
//         over all sequences; ties keep the order (sequence, cell, eye).
//  score: (image << 22 | tile row << 8 | tile column), image = 2 sequence + eye; image i owns the workgroups [off_i, off_i + n_i) with off the prefix sum of
//         the images' tile counts n_i = tiles_x tiles_y.  Workgroup g runs on XCD g & 7: the image's workgroups, ordered by (g & 7, g), take its tiles in
//         row-major order, so every XCD's L2 sees one band of tile rows whatever n_i and off_i are.
// false: an image has more tile columns / rows than an entry holds.
static bool build_mixed_tables(const std::vector<Params> &ps, std::vector<uint32_t> &cells, std::vector<uint32_t> &score) {
    struct Ent {
        int area;
        uint32_t v;
    };
    std::vector<Ent> es;
    cells.clear(), score.clear();
    for (size_t s = 0; s < ps.size(); s++) {
        const Params &p = ps[s];
        const int eyes = (p.sensor == 2) ? 1 : 2;
        for (int cc = 0; cc < p.n_cells; cc++) {
            const int cx = cc % p.cells_x, cy = cc / p.cells_x;
            const int area = std::min(p.cell_size, p.W - cx * p.cell_size) * std::min(p.cell_size, p.H - cy * p.cell_size);
            for (int e = 0; e < eyes; e++) es.push_back({area, (uint32_t)s << 16 | (uint32_t)e << 8 | (uint32_t)cc});
        }
        const int tx = (p.W + TS_W - 1) / TS_W, ty = (p.H + TS_H - 1) / TS_H;
        if (tx > MIXED_TILE_COLS || ty > MIXED_TILE_ROWS) return false;
        for (int e = 0; e < eyes; e++) {
            const size_t off = score.size(), n = (size_t)tx * ty;
            const uint32_t img = (uint32_t)(2 * s + e);
            score.resize(off + n);
            uint32_t t = 0;
            for (size_t x = 0; x < 8; x++)
                for (size_t g = off + ((x - off) & 7); g < off + n; g += 8, t++) score[g] = img << 22 | (t / (uint32_t)tx) << 8 | (t % (uint32_t)tx);
        }
    }
    std::stable_sort(es.begin(), es.end(), [](const Ent &a, const Ent &b) { return a.area > b.area; });
    for (const Ent &e : es) cells.push_back(e.v);
    return true;
}

// in: ONE parameter set for all B sequences, or -- mixed -- B of them
static Context *create_context(const lvt_amd_params *in, bool mixed, int sensor, int B, int device) {
    if (sensor != 1 && sensor != 2) return nullptr;
    std::vector<Params> prms(mixed ? B : 1);
    for (size_t s = 0; s < prms.size(); s++)
        if (!derive_params(in[s], sensor, prms[s])) return nullptr;
    const Params prm = prms[0];
    std::vector<uint32_t> cells_tab, score_tab;
    if (mixed && !build_mixed_tables(prms, cells_tab, score_tab)) return nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return nullptr;  // no CPU fallback, by design
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (device < 0) device = cur;
    if (device >= ndev) return nullptr;
    Context *c = new Context();
    c->device = device;
    DeviceGuard guard(c);
    try {
        c->count_in(device);
        c->B = B;
        c->sensor = sensor;
        c->prm = prm;
        c->mixed = mixed;
        if (mixed) c->prms = prms;
        c->in_prms.assign(in, in + prms.size());
        for (const Params &q : prms) {
            c->any_staged = c->any_staged || q.staged_th > 0;
            c->any_strips = c->any_strips || q.big_cell_strips != 0;
            c->max_cells = std::max(c->max_cells, q.n_cells);
        }
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        {   // A lock-step batch's feature stream is confined to 7/8 of the device's CUs.  k_cells' workgroups (80 KB of LDS each, two per CU, 50 - 90 us)
            // otherwise hold EVERY CU's LDS while they run, and the single-workgroup kernels of the tracking / early chains (50 - 135 KB) -- whose loop
            // pnp -> early map -> match -> resolve -> pnp is a batch's period up to ~28 sequences -- queue behind them (k_track_mid: 36 us in the
            // pipeline, 12 alone).  Measured, frames/s with all CUs -> with 224 of 256: 8 sequences 43.5k -> 45.7k, 16: 70.1k -> 74.9k, 24: 82.4k -> 86.6k;
            // 32 sequences are bound by the feature stream itself (k_score is VALU-bound) and lose: 92.6k -> 88.6k, so larger batches keep every CU.
            // LVT_AMD_FEATURE_CUS=n overrides (0: all CUs).  (A CU-masked stream cannot be created non-blocking: it synchronises with the NULL
            // stream like any default-flag stream.  The library's own streams are never the NULL stream; a caller may put the tracking chain there
            // (lvt_amd_set_stream(h, NULL)).  Every launch of the masked stream then also waits for the NULL-stream work enqueued before it, and every
            // launch on the NULL stream for the masked stream's earlier work: edges from later to earlier work only, as every gate's wait is
            // (lvt_handover.h) -- no wait can come to depend on work queued behind it.  DESIGN.md section 2, "A caller's stream".)
            int ncu = 0;
            if (B >= 2 && B <= 28) {
                int total = 0;
                if (hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && total >= 64) ncu = total / 8 * 7;
            }
            if (const char *e = std::getenv("LVT_AMD_FEATURE_CUS")) ncu = (B >= 2) ? std::atoi(e) : 0;
            if (ncu > 0 && ncu < 1024) {
                uint32_t mask[32] = {};
                for (int i = 0; i < ncu; i++) mask[i >> 5] |= 1u << (i & 31);
                HIPCHK(c, hipExtStreamCreateWithCUMask(&c->stream_f, 32, mask));
                c->feature_cus = ncu;
            } else
                HIPCHK(c, hipStreamCreateWithFlags(&c->stream_f, hipStreamNonBlocking));
        }
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream_e, hipStreamNonBlocking));
        c->own_stream = true;
        for (auto &e : c->ev_done) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : c->ev_feat) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_depth, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_switch_e, hipEventDisableTiming));
        if (const char *e = std::getenv("LVT_AMD_TEST_GATE_TIMEOUT")) c->test_gate_timeout = std::atol(e);
        {
            // "events": barrier-only ordering; "polling": the polling gates + early stream; unset: polling for the first live
            // handle of the process, events for the ones created beside it -- the gates of several independent handles share
            // the process's few hardware queues and hold up each other's kernels (4 handles: 5 300 frames/s aggregate with
            // polling gates, 9 200 with events); several sequences on one GPU belong in one lock-step batch anyway
            const char *o = std::getenv("LVT_AMD_ORDERING");
            if (o && std::strcmp(o, "events") == 0) c->events_only = true;
            else if (o && std::strcmp(o, "polling") == 0) c->events_only = false, c->ordering_forced = true;
            else c->events_only = B == 1 && c->live_on_device() > 1;
        }
        c->pitch = ((prm.W + 63) / 64) * 64;
        HIPCHK(c, hipHostMalloc((void **)&c->h_ctl, sizeof(Ctl) * B * RING, hipHostMallocCoherent));
        HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_ctl_dev, c->h_ctl, 0));
        HIPCHK(c, hipHostMalloc((void **)&c->h_done, sizeof(seq_t) * B * RING, hipHostMallocCoherent));
        HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_done_dev, c->h_done, 0));
        std::memset(c->h_done, 0, sizeof(seq_t) * B * RING);
        HIPCHK(c, hipHostMalloc((void **)&c->h_pose, sizeof(PoseRec) * B * RING, hipHostMallocCoherent));
        HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_pose_dev, c->h_pose, 0));
        HIPCHK(c, hipHostMalloc((void **)&c->h_pose_done, sizeof(seq_t) * B * RING, hipHostMallocCoherent));
        HIPCHK(c, hipHostGetDevicePointer((void **)&c->h_pose_done_dev, c->h_pose_done, 0));
        std::memset(c->h_pose_done, 0, sizeof(seq_t) * B * RING);
        if (const char *e = std::getenv("LVT_AMD_SYNC_TAIL")) c->early_pose = std::strcmp(e, "wait") != 0;
        c->binned_lists = B > 1;
        if (const char *e = std::getenv("LVT_AMD_BINNED_LISTS")) c->binned_lists = std::atoi(e) != 0;
        if (const char *e = std::getenv("LVT_AMD_TEST_ROW_FALLBACK")) c->force_row_fallback = std::atoi(e) != 0;
        {   // cells by decreasing area (stable): see k_cells
            int idx[CELLS_MAX], area[CELLS_MAX];
            for (int cc = 0; cc < prm.n_cells; cc++) {
                const int cx = cc % prm.cells_x, cy = cc / prm.cells_x;
                idx[cc] = cc;
                area[cc] = std::min(prm.cell_size, prm.W - cx * prm.cell_size) * std::min(prm.cell_size, prm.H - cy * prm.cell_size);
            }
            std::stable_sort(idx, idx + prm.n_cells, [&](int a, int b) { return area[a] > area[b]; });
            for (int cc = 0; cc < CELLS_MAX; cc++) c->cell_order.v[cc] = (uint8_t)(cc < prm.n_cells ? idx[cc] : 0);
        }
        if (std::getenv("LVT_AMD_NO_FEAT_PACK")) c->feat_pack = false;
        if (const char *e = std::getenv("LVT_AMD_BRIEF_FROM_IMAGE")) c->brief_from_image = std::atoi(e) ? 1 : 0;
        if (const char *e = std::getenv("LVT_AMD_SCORE_PIECES")) c->score_pieces = std::max(1, std::min(8, std::atoi(e))), c->score_pieces_auto = false;
        {
            int n_cu = 256;
            (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
            if (!mixed && !prm.big_cell_strips && prm.n_cells * 2 * B > n_cu) c->cells_raw_cap = RAW_CAP_SMALL;
            if (mixed && !c->any_strips && (int)cells_tab.size() > n_cu) c->cells_raw_cap = RAW_CAP_SMALL;  // (the same rule: more cell workgroups than CUs)
        }
        if (mixed) c->score_pieces = 1, c->score_pieces_auto = false;  // a mixed batch's k_score is one launch over its tile table (no pieces)
        if (const char *e = std::getenv("LVT_AMD_CELL_SPLIT")) c->cell_split = std::max(0, std::min(SPLIT_MAX, std::atoi(e)));
        if (const char *e = std::getenv("LVT_AMD_CELLS_RAW_CAP")) c->cells_raw_cap = std::max(RAW_CAP_SMALL, std::min(RAW_CAP, std::atoi(e) & ~1));
        if (const char *e = std::getenv("LVT_AMD_FUSED_PULL")) c->fuse_pull = std::atoi(e) != 0;
        // list kernels: a workgroup of 8 wavefronts works its queries off 32 at a time (four per wavefront), every workgroup stages the train set itself (94 KB of LDS)
        c->lists_wgs_row = c->lists_wgs_map = (B <= 16) ? 4 : 2;  // (measured: 16 sequences 67 / 81 / 81 / 80 k frames/s with 1 / 2 / 4 / 8, 64 sequences 108 / 106 / 102 / 101 -- two there: one workgroup per sequence is 1.6 % faster in frames/s with a kernel twice as long)
        if (const char *e = std::getenv("LVT_AMD_LISTS_WGS")) {
            int r = 0, m = 0;
            const int got = std::sscanf(e, "%d,%d", &r, &m);
            if (got >= 1) c->lists_wgs_row = std::max(1, std::min(64, r));
            if (got >= 2) c->lists_wgs_map = std::max(1, std::min(64, m));
        }
        if (const char *e = std::getenv("LVT_AMD_MATCH_BLOCKS_BATCH")) c->match_blocks_batch = std::max(1, std::min(256, std::atoi(e)));
        HIPCHK(c, hipHostMalloc((void **)&c->h_fargs, sizeof(FrameArgs) * B * RING, hipHostMallocDefault));
        std::memset(c->h_fargs, 0, sizeof(FrameArgs) * B * RING);  // (all-zero: fp32 depth, no external corners, present)
        c->h_seqs.resize(B);
        c->d_ctl.resize(B);
        for (int s = 0; s < B; s++) {
            // every allocation whose size follows the image or the detection grid is sized by THIS sequence's parameters
            const Params &q = prms[mixed ? s : 0];
            const int pitch = ((q.W + 63) / 64) * 64;
            const size_t plane = (size_t)pitch * q.H;
            Seq &S = c->h_seqs[s];
            std::memset(&S, 0, sizeof(S));
            S.prm = q;
            S.ctl = c->d_ctl[s] = c->dalloc<Ctl>(1);
            S.plane_pitch = pitch;
            {
                size_t off = 0;
                for (int cc = 0; cc < q.n_cells; cc++) {
                    const int cx = cc % q.cells_x, cy = cc / q.cells_x;
                    const int cw = std::min(q.cell_size, q.W - cx * q.cell_size), ch = std::min(q.cell_size, q.H - cy * q.cell_size);
                    S.cell_scratch_off[cc] = off;
                    off += (size_t)cw * ch * 6;
                }
            }
            for (int e = 0; e < 2; e++) S.cell_scratch[e] = c->dalloc<uint32_t>((size_t)q.W * q.H * 6 + 64);
            for (int e = 0; e < 2; e++) {
                S.strip_kp[e] = q.big_cell_strips ? c->dalloc<uint32_t>((size_t)q.n_cells * STRIPS * RAW_CAP) : c->dalloc_uncached<uint32_t>((size_t)q.n_cells * SPLIT_MAX * SPLIT_KP_CAP);
                S.strip_n[e] = c->dalloc_uncached<int>((size_t)CELLS_MAX * STRIPS);
                S.cell_big[e] = c->dalloc<int>(CELLS_MAX);
            }
            S.lists_fb = c->dalloc<int>(LFB_WORDS);
            for (int par = 0; par < NPAR; par++) {
                FrameBuf &FB = S.fb[par];
                FB.fc = c->dalloc<FeatCtl>(1);
                for (int e = 0; e < 2; e++) {
                    FB.score[e] = c->dalloc<uint8_t>(plane + 64);
                    FB.boxsum[e] = c->dalloc<uint16_t>(plane + 64);
                    {
                        const size_t tiles_x = (size_t)(q.W + TS_W - 1) / TS_W;
                        FB.seg_keys[e] = c->dalloc<uint32_t>((size_t)q.H * tiles_x * TS_W);
                        FB.seg_cnt[e] = c->dalloc<uint16_t>((size_t)q.H * tiles_x);
                    }
                    FB.cell_kp[e] = c->dalloc<float>((size_t)CELLS_MAX * CELL_OUT_CAP * 3);
                    FB.cell_n[e] = c->dalloc<int>(CELLS_MAX);
                    alloc_feat(c, FB.feat[e]);
                    if (s == 0) {
                        c->d_ext[par][e] = c->dalloc<float>((size_t)EXT_MAX * 2);
                        c->d_img[par][e] = c->dalloc<uint8_t>(plane + 64);
                    }
                    FB.ext_xy_own[e] = c->d_ext[par][e];
                }
                if (s == 0 && sensor == 2) c->d_depth[par] = c->dalloc<float>((size_t)q.W * q.H + 4), c->depth_cap = (size_t)q.W * q.H;
            }
            for (int k = 0; k < 2; k++) {
                alloc_points(c, S.map[k], MAP_MAX);
                alloc_points(c, S.staged[k], STAGED_MAX);
            }
            S.map_cur = c->dalloc<int>(1), S.map_n = c->dalloc<int>(1);
            S.staged_cur = c->dalloc<int>(1), S.staged_n = c->dalloc<int>(1);
            S.proj = c->dalloc<float>((size_t)MAP_MAX * 2);
            S.vis = c->dalloc<int8_t>(MAP_MAX);
            S.match = c->dalloc<int>(MAP_MAX);
            S.cand = c->dalloc<uint32_t>((size_t)MAP_MAX * KC);
            S.ncand = c->dalloc<int>(MAP_MAX);
            S.qidx = c->dalloc<uint32_t>(MAP_MAX);
            S.sproj = c->dalloc<float>((size_t)STAGED_MAX * 2);
            S.svis = c->dalloc<int8_t>(STAGED_MAX);
            S.smatch = c->dalloc<int>(STAGED_MAX);
            S.scand = c->dalloc<uint32_t>((size_t)STAGED_MAX * KC);
            S.sncand = c->dalloc<int>(STAGED_MAX);
            S.sdel = c->dalloc<uint8_t>(STAGED_MAX);
            S.pnp_X = c->dalloc<double>((size_t)NF_MAX * 3);
            S.pnp_obs = c->dalloc<float>((size_t)NF_MAX * 2);
            S.pnp_feat = c->dalloc<int>(NF_MAX);
            S.pnp_err = c->dalloc<double>((size_t)NF_MAX * 2 + 2);  // + the sink slot of inactive sweep lanes (pnp_solve)
            S.pnp_level = c->dalloc<int8_t>(NF_MAX);
            S.rcand = c->dalloc<uint32_t>((size_t)NPAR * NF_MAX * KC);  // per frame buffer
            S.rncand = c->dalloc<int>(NPAR * NF_MAX);
            S.pair_l = c->dalloc<int>(NF_MAX), S.pair_r = c->dalloc<int>(NF_MAX);
            S.tri_X = c->dalloc<double>((size_t)NF_MAX * 3);
            S.tri_ok = c->dalloc<int8_t>(NF_MAX);
        }
        {
            Seq *d = c->dalloc<Seq>(B);
            HIPCHK(c, hipMemcpy(d, c->h_seqs.data(), sizeof(Seq) * B, hipMemcpyHostToDevice));
            c->d_seqs = d;
        }
        if (mixed) {
            c->n_score_wgs = (int)score_tab.size(), c->n_cells_wgs = (int)cells_tab.size();
            c->d_score_tab = c->dalloc<uint32_t>(score_tab.size());
            c->d_cells_tab = c->dalloc<uint32_t>(cells_tab.size());
            HIPCHK(c, hipMemcpy(c->d_score_tab, score_tab.data(), sizeof(uint32_t) * score_tab.size(), hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(c->d_cells_tab, cells_tab.data(), sizeof(uint32_t) * cells_tab.size(), hipMemcpyHostToDevice));
            HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cells_mixed), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        }
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cells<true>), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cells<false>), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hamming_batched_lists<MODE_MAP, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hamming_batched_lists<MODE_MAP, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hamming_batched_lists<MODE_ROW, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hamming_batched_lists<MODE_ROW, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cells_strip), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gather<true>), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_gather<false>), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cells_big), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cells_radii), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cells_select), hipFuncAttributeMaxDynamicSharedMemorySize, CELLS_LDS_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pnp<true>), hipFuncAttributeMaxDynamicSharedMemorySize, PNP_DYN_BYTES));
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pnp<false>), hipFuncAttributeMaxDynamicSharedMemorySize, PNP_DYN_BYTES));
        reset_state(c);
    } catch (...) {
        delete c;
        return nullptr;
    }
    return c;
}
static Context *create_context(const lvt_amd_params &in, int sensor, int B, int device = -1) { return create_context(&in, false, sensor, B, device); }

// ---- the per-frame launch chain -------------------------------------------------------------------
static const char *kProfNames[Context::PROF_SLOTS] = {
    "k_feat_begin", "k_gate [early stream: waits for the previous k_pnp]", "k_score", "k_cells(pass0)", "k_rectify_frames", "k_gather(+ the rare retry pass)", "k_brief", "k_gate_late [waits for the early stream]",
    "k_match_map(wait for the early stream + begin + new points)", "k_early_map [early stream]", "k_early_mid [early stream]", "k_hamming_batched_lists(map) [early stream]", "k_track_mid(resolve+pass2+bookkeep+cull)", "k_pnp(+project staged)", "k_gray_frames",
    "k_pose_info", "k_candidates(staged)", "k_depth_clear", "k_candidates(row) [early stream]", "k_hamming_batched_lists(row)", "k_triangulate(staged update+row resolve+triangulate+finalize)", "k_depth_register",
    "k_state_pack", "k_state_unpack", "k_clahe_lut", "k_clahe_apply", "k_mask_features", "k_depth_guard", "k_label_mask", "k_reduce_frames", "k_sensor_frames", "k_sensor_hist", "k_sensor_levels"};

#define LAUNCH(slot, st, kern, grid, block, lds, ...)                              \
    do {                                                                           \
        if (c->prof) (void)hipEventRecord(c->ev[slot][0], st);                     \
        hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__);               \
        if (c->prof) {                                                             \
            (void)hipEventRecord(c->ev[slot][1], st);                              \
            c->ev_used[slot] = true;                                               \
        }                                                                          \
    } while (0)

// kernels of the early / tracking chains: a single sequence travels BY VALUE in the kernel arguments (k_track.hip, SeqArg)
#define LAUNCH_S(slot, st, kern, grid, block, lds, ...)                                                      \
    do {                                                                                                     \
        if (B == 1) LAUNCH(slot, st, kern<true>, grid, block, lds, SeqArg<true>{c->h_seqs[0]}, __VA_ARGS__); \
        else LAUNCH(slot, st, kern<false>, grid, block, lds, SeqArg<false>{S}, __VA_ARGS__);                  \
    } while (0)
#define LAUNCH_SM(slot, st, kern, MODE_, grid, block, lds, ...)                                                        \
    do {                                                                                                               \
        if (B == 1) LAUNCH(slot, st, (kern<MODE_, true>), grid, block, lds, SeqArg<true>{c->h_seqs[0]}, __VA_ARGS__);   \
        else LAUNCH(slot, st, (kern<MODE_, false>), grid, block, lds, SeqArg<false>{S}, __VA_ARGS__);                   \
    } while (0)

static void collect_oldest(Context *c);

// ---- a frame's inputs ---------------------------------------------------------------------------------
// Every path BUILDS a FrameArgs -- from FrameArgs{}: fp32 depth, no external corners, present -- and assigns the whole value to its place in the ring:
// a slot still holds the frame of RING steps ago, and nothing of it may reach the kernels.
static FrameArgs stereo_args(const void *left, const void *right, int pitch_bytes) {
    FrameArgs f{};
    f.img[0] = static_cast<const uint8_t *>(left);
    f.img[1] = static_cast<const uint8_t *>(right);
    f.img_pitch = pitch_bytes;
    return f;
}
static FrameArgs with_depth(FrameArgs f, const void *depth, int depth_pitch_bytes, int fmt, float scale) {
    f.depth = static_cast<const float *>(depth);
    f.depth_pitch = depth_pitch_bytes / ((fmt == DEPTH_U16) ? 2 : 4);  // elements inside the kernels
    f.depth_format = fmt;
    f.depth_scale = (fmt == DEPTH_U16) ? scale : 0.f;
    return f;
}
static FrameArgs rgbd_args(const void *gray, int gray_pitch, const void *depth, int depth_pitch_bytes, int fmt, float scale) {
    return with_depth(stereo_args(gray, gray, gray_pitch), depth, depth_pitch_bytes, fmt, scale);  // (eye 1 of an RGB-D sequence: every kernel stands down for it)
}
static FrameArgs absent_args() {  // the sequence has no frame in this lock-step step
    FrameArgs f{};
    f.absent = 1;
    return f;
}
// lvt_track_with_external_corners; xy: the frame's own lists (a pooled seat's), nullptr: the context's (d_ext[par])
static FrameArgs with_corners(FrameArgs f, int n_left, int n_right, const float *xy_left = nullptr, const float *xy_right = nullptr) {
    f.ext_corners = 1;
    f.n_ext[0] = n_left, f.n_ext[1] = n_right;
    f.ext_xy[0] = xy_left, f.ext_xy[1] = xy_right;
    return f;
}
// sequence s of ring slot `slot`.  The slot is the caller's to name, and to name LATE: make_room / drain / flush_pending may enqueue the held frame and move enq.
static FrameArgs &frame_args(Context *c, int slot, int s = 0) { return c->h_fargs[(size_t)slot * c->B + s]; }
static int next_slot(const Context *c) { return (int)(c->enq % RING); }  // the slot the next enqueue_frame reads

// frame inputs must already be in h_fargs[slot] (and any upload enqueued on stream_f)
struct HostTimer {
    double *acc;
    std::chrono::steady_clock::time_point t0;
    explicit HostTimer(double *a) : acc(a), t0(std::chrono::steady_clock::now()) {}
    ~HostTimer() { *acc += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
};
// the frame (sequence number) that used the feature buffer of the frame about to be enqueued last: gate_buf_wait's `want` (only from frame NPAR on)
static seq_t buffer_last_user(const Context *c) { return (seq_t)(c->enq + 1 - NPAR); }
// the frame properties' part of the chain (lvt_frame_props.h, which needs the refusal path further down: declared here for enqueue_frame).  The depth tables of
// a step are kept between its two launches: the first in place, further ones on the heap; `first` is written only when a sequence registers
struct DepthRegStep {
    DepthRegTable tab;
    int n, px;  // descriptors, and the largest depth image (pixels) among them
};
struct DepthRegPlan {
    DepthRegStep first;
    std::vector<DepthRegStep> more;
    int n = 0;  // tables
};
static void convert_colour_frames(Context *c, int slot, int par, int Bz);
static void reduce_frames(Context *c, int slot, int par, int Bz);
static void convert_sensor_frames(Context *c, int slot, int par, int Bz);
static void rectify_raw_frames(Context *c, int slot, int par, int Bz);
static void equalise_frames(Context *c, int slot, int par, int Bz);
static void begin_depth_registration(Context *c, int slot, int par, int Bz, DepthRegPlan &plan);
static void scatter_depth_planes(Context *c, const DepthRegPlan &plan);
static void mask_features(Context *c, int slot, int par, int Bz);
static void build_label_masks(Context *c, int slot, int par, int Bz);
static void guard_features(Context *c, int slot, int par, int Bz);
static void enqueue_frame(Context *c) {
    HostTimer ht(&c->host_enq_us);
    c->host_enq_n++;
    const int B = c->B;
    // sequences this step's kernels are launched for: all of them -- or, for a pool whose upper seats are empty, the seats in use (lvt_pool.h);
    // B stays the batch's size: strides of the pinned rings, single-sequence / batch code paths
    const int Bz = (c->launch_seqs > 0 && c->launch_seqs < B) ? c->launch_seqs : B;
    c->ring_seqs[(int)(c->enq % RING)] = Bz;
    const Params &p = c->prm;
    const Seq *S = c->d_seqs;
    const int slot = (int)(c->enq % RING), par = (int)(c->enq % NPAR);
    if (c->want_events && !c->events_only) {
        // polling -> events, between two frames.  The frames already enqueued were ordered by the gates: (i) the last of them expects THIS frame's
        // gate to deliver its record -- deliver it now; (ii) their ev_done events were never recorded, so this frame's feature stage waits for
        // everything the tracking stream holds instead (the frames after it are behind it on the same stream; from frame + NPAR on the events exist).
        if (c->enq > 0 && c->delivered < c->enq) {
            const int pslot = (int)((c->enq - 1) % RING);
            hipLaunchKernelGGL(k_deliver, dim3(1, 1, Bz), dim3(64), 0, c->stream, S, c->h_ctl_dev + (size_t)pslot * B, c->h_done_dev + (size_t)pslot * B, (seq_t)c->enq);
            c->delivered = c->enq;
        }
        // the early stream may still hold kernels of the pre-switch frames (k_gate, k_early_map, k_candidates<ROW>, k_row_done: they write the row lists
        // and FeatCtl::row_seq of buffers the event-ordered frames reuse) -- exactly when the streams did not run side by side.  Both other streams wait
        // for it; its gates time out by themselves, so this cannot deadlock.
        (void)hipEventRecord(c->ev_switch_e, c->stream_e);
        (void)hipStreamWaitEvent(c->stream, c->ev_switch_e, 0);
        (void)hipStreamWaitEvent(c->stream_f, c->ev_switch_e, 0);
        (void)hipEventRecord(c->ev_switch, c->stream);
        (void)hipStreamWaitEvent(c->stream_f, c->ev_switch, 0);
        c->events_only = true;
        c->want_events = false;
        c->switched_at = (long)c->enq;
    }
    const FrameArgs *fa = &frame_args(c, slot);
    const int ext = (B == 1) ? fa[0].ext_corners : 0;  // (a pool's step may mix seats with and without external corners: k_cells is launched, cell_begin skips the seats that bring their own)
    hipStream_t sf = c->stream_f, st = c->stream;
    for (int i = 0; i < Context::PROF_SLOTS; i++) c->ev_used[i] = false;
    // ---- a caller's stream: the step's planes were written by work the caller enqueued there -- the feature stage, their only reader outside `st` itself, waits for it
    if (!c->own_stream) {
        (void)hipEventRecord(c->ev_caller, st);
        (void)hipStreamWaitEvent(sf, c->ev_caller, 0);
    }
    // ---- feature stage (stream_f): may start as soon as the tracking chain of frame enq-NPAR released this buffer
    // ---- the frame properties' launches at its head, ahead of the buffer gate (lvt_frame_props.h: why stream order alone covers each hand-over).  They point the
    //      step's FrameArgs at the planes they write, so they come before k_score<true> / k_feat_begin* carries the records to the device: convert, then reduce
    //      (a large frame is averaged as the gray image the caller would have handed in), then remap (the reference's order), then equalise (the plane k_score would have read), then the clear of the registered depth planes, whose scatter goes out
    //      in front of k_gather.
    c->ring_converted[slot] = c->ring_reduced[slot] = c->ring_registered[slot] = c->ring_equalised[slot] = c->ring_masked[slot] = c->ring_guarded[slot] = false;
    if (!c->label_built.empty()) std::fill_n(c->label_built.begin() + (size_t)slot * B * 2, (size_t)B * 2, (uint8_t)0);
    if (c->n_colour) convert_colour_frames(c, slot, par, Bz);
    if (c->n_sensor) convert_sensor_frames(c, slot, par, Bz);  // (a sequence has a colour or a sensor format, never both: the same place in the order)
    if (c->n_reduce) reduce_frames(c, slot, par, Bz);
    if (c->n_rect) rectify_raw_frames(c, slot, par, Bz);
    if (c->n_equal) equalise_frames(c, slot, par, Bz);
    DepthRegPlan dreg;
    if (c->n_depth_cam) begin_depth_registration(c, slot, par, Bz, dreg);
    if (c->n_label) build_label_masks(c, slot, par, Bz);
    const bool evo = c->events_only;
    const bool feat_pack = B > 1 && Bz <= FEAT_PACK && c->feat_pack;  // (k_feat_begin_pack: the buffer gate rides in it)
    if (c->enq >= NPAR) {
        if (!evo) {  // polls; see k_gate_buf (ev_done is never recorded in this mode)
            if (!feat_pack) hipLaunchKernelGGL(k_gate_buf, dim3(1, 1, Bz), dim3(64), 0, sf, S, buffer_last_user(c), par);
        } else if (c->switched_at < 0 || (long)c->enq - NPAR >= c->switched_at) {  // (frames from before a switch of the ordering: covered by ev_switch)
            (void)hipStreamWaitEvent(sf, c->ev_done[(int)((c->enq - NPAR) % RING)], 0);
        }
    }
    if (B == 1) {  // the frame's inputs travel as a kernel argument: no separate "begin" launch, no device read of pinned host memory
        LAUNCH(2, sf, k_score<true>, dim3((p.W + TS_W - 1) / TS_W, (p.H + TS_H - 1) / TS_H, 2), dim3(256), 0, S, c->h_fargs[slot], par, 0, c->brief_from_image ? 0 : 1);
    } else {
        if (feat_pack) {
            FrameArgsPack pk;
            std::memset(&pk, 0, sizeof(pk));
            for (int s = 0; s < Bz; s++) pk.a[s] = fa[s];
            LAUNCH(0, sf, k_feat_begin_pack, dim3(Bz), dim3(64), 0, S, pk, par, (c->enq >= NPAR && !evo) ? buffer_last_user(c) : (seq_t)0);
        } else
            LAUNCH(0, sf, k_feat_begin, dim3(Bz), dim3(64), 0, S, fa, par);
        if (c->mixed) {  // exactly the tiles that exist, each image's placed over the XCDs by the table (build_mixed_tables)
            LAUNCH(2, sf, k_score_mixed, dim3(c->n_score_wgs), dim3(256), 0, S, c->d_score_tab, par, c->brief_from_image ? 0 : 1);
        } else {   // the batch's images in score_pieces launches: see Context::score_pieces
            const int P = std::max(1, std::min(c->score_pieces, Bz));
            for (int q = 0; q < P; q++) {
                const int z0 = 2 * (int)((long)Bz * q / P), z1 = 2 * (int)((long)Bz * (q + 1) / P);
                if (q == 0) LAUNCH(2, sf, k_score<false>, dim3((p.W + TS_W - 1) / TS_W, (p.H + TS_H - 1) / TS_H, z1 - z0), dim3(256), 0, S, FrameArgs{}, par, z0, c->brief_from_image ? 0 : 1);
                else hipLaunchKernelGGL(k_score<false>, dim3((p.W + TS_W - 1) / TS_W, (p.H + TS_H - 1) / TS_H, z1 - z0), dim3(256), 0, sf, S, FrameArgs{}, par, z0, c->brief_from_image ? 0 : 1);
            }
        }
    }
    if (!ext) {
        {
            // detection pass 0 (the <200-corner retry pass runs inside k_gather: it is almost never taken)
            // (a single sequence: + the workgroups that pull the next asynchronous host frame, one 16-byte vector per thread)
            const int pull_wgs = (B == 1 && c->next_pull.src[0]) ? std::min(64, (int)(((size_t)c->next_pull.W * c->next_pull.H / 16 + 1023) / 1024)) : 0;  // (W: bytes per row, n_cols * bpp on a colour handle)
            // a single sequence's tall cells run as cell_split co-operating workgroups (cells_work_split); grid: helpers, main workgroups, pull, padded to 8
            const int ns = (B == 1 && !p.big_cell_strips) ? c->cell_split : 0;
            const int gx = (ns >= 2) ? ((((p.n_cells + 7) & ~7) * ns + pull_wgs + 7) & ~7) : p.n_cells + pull_wgs;
            if (c->mixed) LAUNCH(3, sf, k_cells_mixed, dim3(c->n_cells_wgs), dim3(1024), cells_lds_bytes(c->cells_raw_cap), S, c->d_cells_tab, par, c->cells_raw_cap);
            else LAUNCH_S(3, sf, k_cells, (B == 1 ? dim3(gx, 2, 1) : dim3(p.n_cells * 2 * Bz, 1, 1)), dim3(1024), cells_lds_bytes(c->cells_raw_cap), par, c->cell_order, 2 * Bz, c->cells_raw_cap, c->next_pull, ns, (++c->cell_token ? c->cell_token : ++c->cell_token));
            // (a mixed batch: when ANY sequence has cells tall enough to cut, over the largest grid -- a sequence without such cells leaves at cell_big != 1,
            //  a cell index beyond a sequence's grid at cell_begin)
            if (c->any_strips) {  // oversized cells: NMS as row strips on several CUs, then ANMS of the merged survivors in three launches
                const int nc = c->max_cells;
                hipLaunchKernelGGL(k_cells_strip, dim3(nc * STRIPS, 2, Bz), dim3(1024), CELLS_LDS_BYTES, sf, S, par);
                hipLaunchKernelGGL(k_cells_big, dim3(nc, 2, Bz), dim3(1024), CELLS_LDS_BYTES, sf, S, par);
                hipLaunchKernelGGL(k_cells_radii, dim3(nc * RADII_WGS, 2, Bz), dim3(1024), CELLS_LDS_BYTES, sf, S, par);
                hipLaunchKernelGGL(k_cells_select, dim3(nc, 2, Bz), dim3(1024), CELLS_LDS_BYTES, sf, S, par);
                if (c->prof) (void)hipEventRecord(c->ev[3][1], sf);  // (the slot's time covers the five launches)
            }
        }
    }
    if (c->before_gather) {  // (the GPU is busy with k_score / k_cells from here on: host-side copies behind this point are free)
        c->before_gather();
        c->before_gather = nullptr;
    }
    if (c->depth_wait) {
        (void)hipStreamWaitEvent(sf, c->ev_depth, 0);
        c->depth_wait = false;
    }
    scatter_depth_planes(c, dreg);  // (behind the wait for ev_depth: a host call's depth plane arrives on the early stream)
    LAUNCH_S(5, sf, k_gather, dim3(1, 2, Bz), dim3(1024), CELLS_LDS_BYTES, par);
    if (c->n_guard) guard_features(c, slot, par, Bz);  // (directly behind k_gather: the plane it sampled is the plane the guard reads)
    if (c->n_mask || c->n_label) mask_features(c, slot, par, Bz);  // (the seam: k_gather has written the Feat arrays and *F.n, k_brief reads them)
    const bool brief_publishes = !evo && B == 1;  // (single sequence: k_brief's last workgroup publishes feat_seq; see k_feat_done)
    if (c->brief_from_image) LAUNCH_S(6, sf, k_brief_img, dim3(64, 2, Bz), dim3(256), 0, par, brief_publishes ? (seq_t)(c->enq + 1) : (seq_t)0);
    else LAUNCH_S(6, sf, k_brief, dim3(64, 2, Bz), dim3(256), 0, par, brief_publishes ? (seq_t)(c->enq + 1) : (seq_t)0);
    if (!evo && !brief_publishes) hipLaunchKernelGGL(k_feat_done, dim3(Bz), dim3(64), 0, sf, S, par, (seq_t)(c->enq + 1));
    const int bl = c->binned_lists ? 1 : 0;
    if (evo && bl && c->sensor == 1) LAUNCH_SM(19, sf, k_hamming_batched_lists, MODE_ROW, dim3(c->lists_wgs_row, 1, Bz), dim3(LS_THREADS), LS_LDS_BYTES, par, (seq_t)0);
    if (evo) LAUNCH_SM(18, sf, k_candidates, MODE_ROW, dim3(256, 1, Bz), dim3(256), 0, 0, par, (seq_t)0, bl);  // (normal mode: on the early stream, below)
    if (evo) hipLaunchKernelGGL(k_feat_done, dim3(Bz), dim3(64), 0, sf, S, par, (seq_t)(c->enq + 1));
    if (evo) (void)hipEventRecord(c->ev_feat[par], sf);
    // ---- early stream: projection, candidate lists and greedy resolution of the map points that survived the previous frame,
    //      as soon as that frame's pose exists (its k_pnp) -- its k_triangulate only appends behind them
    const seq_t seq = (seq_t)(c->enq + 1);  // this frame's sequence number; the previous frame's is enq (0: none)
    if (!evo) {
        hipStream_t se = c->stream_e;
        LAUNCH_S(1, se, k_gate, dim3(1, 1, Bz), dim3(64), 0, par, (seq_t)c->enq, seq, (c->test_gate_timeout && (long)seq == c->test_gate_timeout) ? 1 : 0);  // polls the previous k_pnp and this frame's features
        if (bl) LAUNCH_SM(11, se, k_hamming_batched_lists, MODE_MAP, dim3(c->lists_wgs_map, 1, Bz), dim3(LS_THREADS), LS_LDS_BYTES, par, seq);
        LAUNCH_S(9, se, k_early_map, dim3((bl && B > 1) ? 32 : 256, 1, Bz), dim3(256), 0, par, seq, bl);  // (behind the binned list kernel it is the fall-back only)
        LAUNCH_S(10, se, k_early_mid, dim3(1, 1, Bz), dim3(RES_THREADS), 0, par, seq);
        if (c->sensor == 1) {
            // row-match candidate lists of THIS frame (needed by its k_triangulate, ~70 us from here): they need the two feature
            // sets only, and the feature stream is the longest chain -- here, behind the early part, they lengthen neither it nor
            // the hand-over to the tracking stream.  Few workgroups: the tracking chain's single-workgroup kernels run meanwhile.
            if (bl) LAUNCH_SM(19, se, k_hamming_batched_lists, MODE_ROW, dim3(c->lists_wgs_row, 1, Bz), dim3(LS_THREADS), LS_LDS_BYTES, par, seq);
            LAUNCH_SM(18, se, k_candidates, MODE_ROW, dim3(B == 1 ? ROW_BLOCKS : ROW_BLOCKS_BATCH, 1, Bz), dim3(256), 0, 0, par, seq, bl);
            hipLaunchKernelGGL(k_row_done, dim3(Bz), dim3(64), 0, se, S, par, seq);
        }
    }
    // ---- tracking chain (stream): strictly ordered frame after frame
    // (no barrier on the features here: k_gate_late returns only after the early stream's gate has seen them complete, and
    //  every barrier / event packet costs this stream 3-4 us per frame)
    {
        // the previous frame's record, if nobody has been asked to deliver it yet
        Ctl *prec = nullptr;
        seq_t *pdone = nullptr;
        if (!evo && c->delivered < c->enq) {
            const int pslot = (int)((c->enq - 1) % RING);
            prec = c->h_ctl_dev + (size_t)pslot * B, pdone = c->h_done_dev + (size_t)pslot * B;
            c->delivered = c->enq;
        }
        if (evo) {
            (void)hipStreamWaitEvent(st, c->ev_feat[par], 0);  // (the early stream never claims the frame: early_ran_seq stays behind)
            LAUNCH_S(8, st, k_match_map, dim3(256, 1, Bz), dim3(256), 0, par, seq, 0, (Ctl *)nullptr, (seq_t *)nullptr);
        } else if (B == 1 && c->live_on_device() <= MAX_FOLDED_GATES) {
            // one launch: delivers the record, waits for the early stream (polled, no barrier packet), lists the points appended since
            LAUNCH_S(8, st, k_match_map, dim3(MATCH_BLOCKS_GATED, 1, 1), dim3(256), 0, par, seq, 1, prec, pdone);
        } else {
            LAUNCH_S(7, st, k_gate_late, dim3(1, 1, Bz), dim3(64), 0, par, seq, prec, pdone);
            LAUNCH_S(8, st, k_match_map, dim3(B > 1 ? c->match_blocks_batch : 256, 1, Bz), dim3(256), 0, par, seq, 0, (Ctl *)nullptr, (seq_t *)nullptr);
        }
    }
    LAUNCH_S(12, st, k_track_mid, dim3(1, 1, Bz), dim3(RES_THREADS), 0, par, seq);
    {
        const bool ep = c->sync_call && c->early_pose && !c->prof && B == 1;
        LAUNCH_S(13, st, k_pnp, dim3(1, 1, Bz), dim3(PNP_THREADS), PNP_DYN_BYTES, par, seq, ep ? c->h_pose_dev + (size_t)slot * B : (PoseRec *)nullptr,
                 ep ? c->h_pose_done_dev + (size_t)slot * B : (seq_t *)nullptr);
    }
    if (c->pose_info) LAUNCH_S(15, st, k_pose_info, dim3(1, 1, Bz), dim3(PI_THREADS), 0, c->h_pinfo_dev + (size_t)slot * B);
    if (c->any_staged)  // (a configuration without staging -- EuRoC, TUM -- never has staged points to list; in a mixed batch such a sequence leaves at the kernel's head)
        LAUNCH_SM(16, st, k_candidates, MODE_STAGED, dim3(64, 1, Bz), dim3(256), 0, 0, par, (seq_t)0, 0);
    LAUNCH_S(20, st, k_triangulate, dim3(1, 1, Bz), dim3(1024), 0, par, seq, c->h_ctl_dev + (size_t)slot * B,
           c->h_done_dev + (size_t)slot * B, evo ? 0 : (c->force_row_fallback ? 2 : 1), (evo || c->sync_call) ? 1 : 0);
    if (evo || c->sync_call) c->delivered = c->enq + 1;
    if (evo) (void)hipEventRecord(c->ev_done[slot], st);  // (events-only ordering: the feature stream's barrier needs it)
    c->enq++;
}

// spin until pinned flag `a` (or `b`, if given) carries `want`; every 2^20 spins (~10 ms) the tracking stream is asked (*q): a dead stream must not hang the caller
enum class SpinStop { FLAG_A, FLAG_B, STREAM_ERROR, STREAM_IDLE };
static SpinStop spin_on_flags(Context *c, seq_t want, volatile seq_t *a, volatile seq_t *b, unsigned &spins, hipError_t *q) {
    for (;;) {
        if (__atomic_load_n(a, __ATOMIC_ACQUIRE) == want) return SpinStop::FLAG_A;
        if (b && __atomic_load_n(b, __ATOMIC_ACQUIRE) == want) return SpinStop::FLAG_B;
        __builtin_ia32_pause();
        if ((++spins & 0xFFFFF) == 0) {
            *q = hipStreamQuery(c->stream);
            if (*q != hipErrorNotReady) return *q == hipSuccess ? SpinStop::STREAM_IDLE : SpinStop::STREAM_ERROR;
        }
    }
}
// wait for the oldest un-collected frame; its record becomes "last"
static void collect_oldest(Context *c) {
    HostTimer ht(&c->host_wait_us);
    c->host_wait_n++;
    if (c->done >= c->enq) return;
    const int slot = (int)(c->done % RING);
    const int Bz = (c->ring_seqs[slot] > 0 && c->ring_seqs[slot] <= c->B) ? c->ring_seqs[slot] : c->B;  // sequences the step was launched for
    if (c->delivered < c->done + 1) {  // the last enqueued frame of an asynchronous run: nobody has been asked to deliver it yet
        hipLaunchKernelGGL(k_deliver, dim3(1, 1, Bz), dim3(64), 0, c->stream, c->d_seqs, c->h_ctl_dev + (size_t)slot * c->B,
                           c->h_done_dev + (size_t)slot * c->B, (seq_t)(c->done + 1));
        c->delivered = c->done + 1;
    }
    {   // the frame is complete when every sequence's flag carries its number (the flags follow the records: system-scope
        // release on the device, acquire here)
        const seq_t want = (seq_t)(c->done + 1);
        unsigned spins = 0;
        for (int s = 0; s < Bz; s++) {
            volatile seq_t *f = c->h_done + (size_t)slot * c->B + s;
            hipError_t q = hipSuccess;
            const SpinStop why = spin_on_flags(c, want, f, nullptr, spins, &q);
            if (why == SpinStop::STREAM_ERROR) {
                c->set_error(std::string("tracking stream: ") + hipGetErrorString(q));
                break;
            }
            if (why == SpinStop::STREAM_IDLE && __atomic_load_n(f, __ATOMIC_ACQUIRE) != want) {  // stream empty but no flag: cannot happen
                c->set_error("tracking stream finished without a result record");
                break;
            }
        }
        if (c->prof) HIPCHK(c, hipStreamSynchronize(c->stream));  // the per-kernel timing events are read below
    }
    c->last_slot = slot;
    c->last_par = (int)(c->done % NPAR);
    c->done++;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) c->set_error(std::string("kernel chain: ") + hipGetErrorString(e));
    if (c->prof && c->done == c->enq) {  // profiling is meaningful when frames are collected one at a time
        for (int i = 0; i < Context::PROF_SLOTS; i++)
            if (c->ev_used[i]) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, c->ev[i][0], c->ev[i][1]) == hipSuccess) {
                    c->prof_ms[i] += ms;
                    c->prof_calls[i]++;
                }
            }
    }
    bool cut = false;
    for (int s = 0; s < Bz; s++)
        if (c->h_ctl[(size_t)slot * c->B + s].overflow) {
            char buf[128];
            std::snprintf(buf, sizeof(buf), "capacity overflow mask 0x%x in sequence %d", c->h_ctl[(size_t)slot * c->B + s].overflow, s);
            c->set_error(buf);
            cut = true;
        }
    if (cut) c->ovf_done = (long long)c->done;
    else if (c->capacity_report() && c->ovf_read_done >= c->ovf_done) c->err.clear();  // an earlier frame's report, read since: this frame fits
    if (c->B > 1 && c->score_pieces_auto && !c->events_only) {  // see Context::score_pieces
        const Ctl &r0 = c->h_ctl[(size_t)slot * c->B];
        const long long t0 = r0.dbg[32], t1 = r0.dbg[35], t2 = r0.dbg[33];
        if (t0 > 0 && t0 <= t1 && t1 <= t2 && t2 - t0 < 1000000) {  // (a consistent triple of one gate, < 10 ms)
            const double d = 0.01 * (double)((t2 - t1) - (t1 - t0));
            c->gate_balance_us = 0.8 * c->gate_balance_us + 0.2 * d;
            if (c->gate_balance_us > 15.0) c->score_pieces = 2;
            else if (c->gate_balance_us < -15.0) c->score_pieces = 1;
        }
    }
    for (int s = 0; s < Bz; s++)
    {
        const Ctl &r = c->h_ctl[(size_t)slot * c->B + s];
        if (r.gate_fatal != c->gate_fatal_seen) {
            c->gate_fatal_seen = r.gate_fatal;
            c->set_error("a stream waited 2 s for another one (features / buffer hand-over): a frame was SKIPPED (its pose is the previous frame's, the "
                         "tracking state is unchanged); under a tool that serialises kernel dispatches (rocprofv3 --pmc) set LVT_AMD_ORDERING=events"
                         + std::string(c->ordering_forced || c->events_only ? "" : " -- the handle moves to event ordering from the next frame on"));
            if (!c->ordering_forced && !c->events_only) c->want_events = true;
        } else if (r.gate_timeouts != c->gate_timeouts_seen) {
            c->gate_timeouts_seen = r.gate_timeouts;
            // not a wrong result (the frame was tracked without the early stream / with row lists built on the tracking stream), but
            // milliseconds were lost: the streams do not run concurrently (shared hardware queue, or a tool that serialises the dispatches)
            c->set_error(std::string("a stream gate timed out (results unaffected; the streams do not run concurrently: LVT_AMD_ORDERING=events avoids the waits)")
                         + (c->ordering_forced || c->events_only ? "" : " -- the handle moves to event ordering from the next frame on"));
            if (!c->ordering_forced && !c->events_only) c->want_events = true;
        }
    }
}
// the held asynchronous host frame (Context::pend) enters the launch chain; np: the images its k_cells launch pulls for the frame behind it
static void flush_pending(Context *c, const NextPull *np = nullptr) {
    if (!c->pend.valid) return;
    Context::PendingFrame &q = c->pend;
    q.valid = false;
    if (!q.pulled) hipLaunchKernelGGL(k_stage_in, dim3(128, 2), dim3(256), 0, c->stream_f, q.src[0], q.src[1], q.dst[0], q.dst[1], q.row_bytes, q.rows, q.pitch);
    frame_args(c, next_slot(c)) = q.f;
    if (np) c->next_pull = *np, c->fused_pulls++;
    enqueue_frame(c);
    c->next_pull = NextPull{};
}
static void drain(Context *c) {
    flush_pending(c);
    while (c->done < c->enq) collect_oldest(c);
    c->early_pending = false;
}
// synchronous calls: wait for the frame just enqueued -- its pose (k_pnp) or, when the frame has none of its own (first frame, LOST,
// skipped), its full record.  Returns true when R / t were taken from the early pose; the frame then stays un-collected until the next
// entry point drains (by then its tail has long finished).
static bool wait_pose_or_frame(Context *c, double R[3][3], double t[3]) {
    HostTimer ht(&c->host_wait_us);
    const int slot = (int)((c->enq - 1) % RING);
    const seq_t want = (seq_t)c->enq;
    volatile seq_t *fp = c->h_pose_done + (size_t)slot * c->B, *fd = c->h_done + (size_t)slot * c->B;
    if (!c->early_pose || c->prof || c->B != 1) {
        drain(c);
        return false;
    }
    unsigned spins = 0;
    hipError_t q = hipSuccess;
    if (spin_on_flags(c, want, fp, fd, spins, &q) == SpinStop::FLAG_A) {
        const PoseRec &p = c->h_pose[(size_t)slot * c->B];
        if (R)
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[i][j] = p.R[3 * i + j];
        if (t)
            for (int i = 0; i < 3; i++) t[i] = p.t[i];
        c->early_pending = true;
        return true;
    }
    drain(c);  // the full record is there, or the stream has stopped: collect_oldest diagnoses it
    return false;
}
static void make_room(Context *c) {  // at most RING-1 frames un-collected before a new one is enqueued
    flush_pending(c);
    while (c->enq - c->done >= RING - 1) collect_oldest(c);
}
static const Ctl &last_ctl(Context *c, int s = 0) { return c->h_ctl[(size_t)c->last_slot * c->B + s]; }

static void result_out(Context *c, int s, double R[3][3], double t[3]) {
    const Ctl &h = last_ctl(c, s);
    if (R)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) R[i][j] = h.out_R[3 * i + j];
    if (t)
        for (int i = 0; i < 3; i++) t[i] = h.out_t[i];
}

// the tail of every synchronous call: the frame in the ring's next slot is enqueued, collected right away -- k_triangulate delivers its record itself -- and its pose
// returned.  sync_call goes back to false on every way out: left standing by a HIP error, it would have the handle's next asynchronous frame claim a delivery it does not make.
static void track_sync(Context *c, double R[3][3], double t[3]) {
    {
        struct Scope {
            bool &flag;
            explicit Scope(bool &f) : flag(f) { flag = true; }
            ~Scope() { flag = false; }
        } sync(c->sync_call);
        enqueue_frame(c);
    }
    if (!wait_pose_or_frame(c, R, t)) result_out(c, 0, R, t);
}

// (the frame's size: the handle's own, or its rectifiers' source size -- Context::frame_W)
static bool size_ok(Context *c, int rows, int cols) { return rows == c->frame_H(0) && cols == c->frame_W(0); }
// a reduced RGB-D sequence takes its depth plane through a depth camera: without one the plane has no size of its own (the frame's? the sequence's?)
static bool reduced_without_depth_camera(const Context *c, int s) { return c->sensor == 2 && c->has_reduce(s) && !c->has_depth_cam(s); }
static const char *kReducedNoDepthCamera = "an RGB-D frame on a sequence with a reduction and no depth camera: the depth plane has no size of its own (set one with lvt_amd_set_depth_camera; a plane registered to the large image: identity extrinsics and the large image's pinhole)";
// pitch of a caller's device plane of sequence s: a rectified frame feeds k_score's word loads (a multiple of 16); a RAW frame (rectifiers attached) is read
// byte-wise by k_rectify_frames: any pitch that holds a row; so is a COLOUR frame by k_gray_frames (a row is cols * bpp bytes) and the gray frame of an
// EQUALISED sequence by k_clahe_lut / k_clahe_apply; a LARGE frame (a reduction in force) is read by k_reduce_frames, whose byte path takes any base and pitch
// (a MONO16 sequence's planes are read as 16-bit words: an odd address is refused here, an odd pitch by device_pitch_ok)
static bool sensor_address_ok(const Context *c, int s, const void *a, const void *b) {
    return !(c->has_sensor(s) && c->sens[(size_t)s].format == SENSOR_MONO16) || ((((uintptr_t)a | (uintptr_t)b) & 1) == 0);
}
static bool device_pitch_ok(const Context *c, int s, int pitch, int cols) {
    if (c->converts(s)) return (long long)pitch >= (long long)cols * c->bpp_of(s) && !(c->has_sensor(s) && c->sens[(size_t)s].format == SENSOR_MONO16 && (pitch & 1));
    return (c->has_rect(s) || c->has_equal(s) || c->has_reduce(s)) ? pitch >= cols : (pitch & 15) == 0;
}

template <typename T>
static void d2h(Context *c, T *dst, const T *src, size_t n) {
    if (n && dst) HIPCHK(c, hipMemcpy(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost));
}
static int read_scalar(Context *c, const int *d) {
    int v = 0;
    HIPCHK(c, hipMemcpy(&v, d, sizeof(int), hipMemcpyDeviceToHost));
    return v;
}

}  // namespace lvt

#include "lvt_pool.h"

namespace lvt {
// what the introspection entry points read: a sequence of a context, the feature-buffer parity and the record of its last collected frame.
// A pooled handle's view holds the pool's lock (no step can start underneath the device reads) after every step in flight has been collected.
struct View {
    Context *c = nullptr;
    int s = 0, par = 0;
    const Ctl *rec = nullptr;
    std::unique_lock<std::mutex> lk;
    DeviceGuard *guard = nullptr;
    ~View() { delete guard; }
};
static bool view_of(lvt_handle h, View &v) {
    if (is_slot(h)) {
        PoolSlot *S = static_cast<PoolSlot *>(h);
        slot_drain(S);
        v.lk = std::unique_lock<std::mutex>(S->pool->mu);
        pool_quiesce(S->pool, v.lk);
        v.c = S->pool->ctx, v.s = S->slot, v.par = S->last.par, v.rec = &S->last.rec;
    } else if (is_ctx(h)) {
        Context *c = static_cast<Context *>(h);
        v.guard = new DeviceGuard(c);
        drain(c);
        v.c = c, v.s = 0, v.par = c->last_par, v.rec = &last_ctl(c);
        return true;
    } else
        return false;
    v.guard = new DeviceGuard(v.c);
    return true;
}
// ---- automatic seats (round 6) -------------------------------------------------------------------------------------------------------------
// The reference lets a process hold several lvt_systems (lvt_c.cpp:33-62); here independent handles with a launch chain each share the process's hardware
// queues badly (8 of them deliver LESS than one), while seats of one lock-step chain scale (lvt_pool.h).  So the REFERENCE's create call, lvt_create, hands
// out a small forwarding record (lvt_amd_create / lvt_amd_create_on_device -- the extension API with its per-stage read-back, most of which a seat does not
// offer -- keep handing out what the caller asked for): a stereo handle starts on a chain of its own, and when a SECOND handle with the same parameters is created on the device while the first has not been
// used yet (nothing but create / get_device / get_ordering / last_error was called on it), both -- and every later one -- become seats of the device's
// pool.  A handle that has already tracked keeps its kind (moving a tracker's state between chains is not attempted), so a process that creates its handles
// first and tracks afterwards -- one thread per sequence, the usual shape -- gets the pool without an environment variable; a lone handle never pays for it.
// LVT_AMD_AUTO_POOL=0 turns this off (every handle solo, as before round 6); LVT_AMD_POOL=1 still forces seats from the first handle on.
constexpr uint64_t AUTO_MAGIC = 0x4C56544155544F31ull;
struct AutoHandle {
    uint64_t magic = AUTO_MAGIC;
    lvt_amd_params prm;
    int device = 0;
    std::mutex mu;
    lvt_handle impl = nullptr;  // Context * or PoolSlot *
    bool started = false;       // the tracker behind the handle has been used: it keeps its kind
};
static std::mutex g_auto_mu;
static std::vector<AutoHandle *> g_auto;
static inline bool is_auto(lvt_handle h) { return h && *static_cast<const uint64_t *>(h) == AUTO_MAGIC; }
static inline lvt_handle resolve_handle(lvt_handle h, bool starts = true) {
    if (!is_auto(h)) return h;
    AutoHandle *A = static_cast<AutoHandle *>(h);
    std::lock_guard<std::mutex> g(A->mu);
    if (starts) A->started = true;
    return A->impl;
}
static bool auto_pool_enabled() {
    const char *e = std::getenv("LVT_AMD_AUTO_POOL");
    return !e || std::atoi(e) != 0;
}
static void destroy_impl(lvt_handle h) {
    if (is_slot(h)) {
        pool_leave(static_cast<PoolSlot *>(h));
    } else if (h) {
        DeviceGuard guard(static_cast<Context *>(h));
        delete static_cast<Context *>(h);
    }
}
// a stereo handle of the default create calls (device < 0: the calling thread's current device)
static lvt_handle auto_create(const lvt_amd_params &p, int device) {
    int cur = 0;
    if (device < 0 && hipGetDevice(&cur) == hipSuccess) device = cur;
    std::lock_guard<std::mutex> G(g_auto_mu);
    bool pool = false;
    for (AutoHandle *X : g_auto) {
        if (X->device != device || !same_params(X->prm, p)) continue;
        std::lock_guard<std::mutex> g(X->mu);
        if (is_slot(X->impl)) {
            pool = true;
        } else if (!X->started) {  // an unused solo handle: it takes a seat (its chain is given back)
            if (PoolSlot *S = pool_join(p, 1, device)) {
                destroy_impl(X->impl);
                X->impl = S;
                pool = true;
            }
        }
    }
    AutoHandle *A = new AutoHandle();
    A->prm = p, A->device = device;
    if (pool) A->impl = static_cast<lvt_handle>(pool_join(p, 1, device));  // (no seat left: a chain of its own)
    if (!A->impl) A->impl = static_cast<lvt_handle>(create_context(p, 1, 1, device));
    if (!A->impl) {
        delete A;
        return nullptr;
    }
    g_auto.push_back(A);
    return static_cast<lvt_handle>(A);
}
static void auto_destroy(AutoHandle *A) {
    {
        std::lock_guard<std::mutex> G(g_auto_mu);
        for (size_t i = 0; i < g_auto.size(); i++)
            if (g_auto[i] == A) {
                g_auto.erase(g_auto.begin() + (long)i);
                break;
            }
    }
    lvt_handle impl;
    {
        std::lock_guard<std::mutex> g(A->mu);
        impl = A->impl, A->impl = nullptr, A->started = true;
    }
    destroy_impl(impl);
    A->magic = 0;
    delete A;
}
// LVT_AMD_POOL=1: every handle the create calls make is pooled.  (A mixed mode -- the first handle of a device on its own launch chain, the later ones
// pooled -- was measured and removed: 2 / 4 / 8 handles 6.8k / 13.1k / 25.3k frames/s against 12.0k / 22.8k / 43.6k all pooled: the solo handle's
// polling gates and the pool's chain hold each other up on the shared hardware queues.)
static bool pool_wanted(int) {
    const char *e = std::getenv("LVT_AMD_POOL");
    return e && std::atoi(e) != 0;
}

// ---- refusals -------------------------------------------------------------------------------------------------------------------------------
// An entry point resolves its handle, checks everything, and only then enqueues.  A refusal is reported as "who: why" on the context or the seat -- the texts are the
// entry points' own, callers match on them -- and returns -1.  A handle that is neither a context, a seat nor an automatic handle (NULL included) has nowhere to
// report to: the call returns (-1 where it returns an int), outputs untouched, without a HIP call.
static int refuse(lvt_handle h, const char *who, const std::string &why) {
    const std::string msg = std::string(who) + ": " + why;
    if (is_slot(h)) {
        PoolSlot *S = static_cast<PoolSlot *>(h);
        std::lock_guard<std::mutex> g(S->pool->mu);
        S->err = msg;
    } else if (is_ctx(h))
        static_cast<Context *>(h)->set_error(msg);
    return -1;
}
// The calling thread's last refusal from a call that has no handle to report to -- a stage entry, a snapshot import or describe, the odometry accumulator's
// relocalisation policy: lvt_amd_last_error(NULL) reads it.  Only refuse_call writes it.
static thread_local std::string g_call_refusal;
static int refuse_call(const char *who, const std::string &why) {
    g_call_refusal = std::string(who) + ": " + why;
    return -1;
}
// what an entry point says to a pooled handle / a handle of the other sensor / a batch handle where it takes solo ones (nullptr: refused without a report)
struct Refusals {
    const char *pooled, *sensor, *batch;
};
// the context behind a (resolved) handle for an entry point of `sensor` (0: either) that takes solo handles (B == 1, not mixed) or, `batch`, any; nullptr: refused
static Context *frame_context(lvt_handle h, const char *who, int sensor, bool batch, const Refusals &why = {nullptr, nullptr, nullptr}) {
    if (is_slot(h)) {
        if (why.pooled) refuse(h, who, why.pooled);
        return nullptr;
    }
    if (!is_ctx(h)) return nullptr;
    Context *c = static_cast<Context *>(h);
    if (sensor && c->sensor != sensor) {
        if (why.sensor) refuse(h, who, why.sensor);
        return nullptr;
    }
    if (!batch && (c->B != 1 || c->mixed)) {
        if (why.batch) refuse(h, who, why.batch);
        return nullptr;
    }
    return c;
}

// ---- host planes ----------------------------------------------------------------------------------------------------------------------------
// the borrowed buffers are copied into pinned memory by the CPU and the GPU pulls them from there -- unless the caller's
// buffer already IS pinned host memory (hipHostMalloc / hipHostRegister, aligned to `align`): then the GPU reads it in place
// (k_stage_in / k_stage_copy never load outside [p, p + bytes): any base address and byte count qualify -- 1241 x 376 bytes are
//  8 mod 16 -- except a depth image that is not even aligned to its element)
static const uint8_t *device_view(const void *p, size_t align) {
    hipPointerAttribute_t a;
    if (((uintptr_t)p & (align - 1)) == 0 && hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeHost && a.devicePointer)
        return static_cast<const uint8_t *>(a.devicePointer);
    (void)hipGetLastError();  // (an ordinary malloc'ed pointer is "invalid value" to the query: not an error of this call)
    return nullptr;
}
// first use of a staging buffer: [image | image] or [image | depth f32] for images of img_bytes (n_rows * n_cols * bpp) and, RGB-D, depth planes of depth_px pixels
// (a change of the pixel format releases the buffers: stage_release)
static void stage_reserve(Context *c, HostStage &st, size_t img_bytes, size_t depth_px) {
    if (st.h) return;
    st.second = (img_bytes + 15) & ~(size_t)15;
    const size_t second_bytes = depth_px ? ((sizeof(float) * depth_px + 15) & ~(size_t)15) : st.second;
    HIPCHK(c, hipHostMalloc((void **)&st.h, st.second + second_bytes, hipHostMallocDefault));
    HIPCHK(c, hipHostGetDevicePointer((void **)&st.dev, st.h, 0));
}
static void stage_release(Context *c) {  // (no frame in flight: nothing reads them)
    for (HostStage *st : {&c->stage[0], &c->stage_ring[0]})
        for (int i = 0, n = (st == &c->stage[0]) ? NPAR : RING; i < n; i++)
            if (st[i].h) {
                (void)hipHostFree(st[i].h);
                st[i] = HostStage{};
            }
}
// The frame's size of sequence 0 changed (rectifiers of another source size attached or detached; no frame in flight): everything of the host entry points
// that was sized by it goes back and is reserved again, at the new size, by the next frame -- the staging, the colour planes, the raw planes.
static void frame_planes_release(Context *c) {
    stage_release(c);
    for (int i = 0; i < NPAR; i++)
        for (int e = 0; e < 2; e++) c->dfree(c->d_col[i][e]), c->dfree(c->d_raw[i][e]), c->d_col[i][e] = c->d_raw[i][e] = nullptr;
    for (int i = 0; i < RING; i++)
        for (int e = 0; e < 2; e++) c->dfree(c->d_col_ring[i][e]), c->dfree(c->d_raw_ring[i][e]), c->d_col_ring[i][e] = c->d_raw_ring[i][e] = nullptr;
}
// a host plane as the device reads it: its view (device_view) when it is page-locked, otherwise its copy at offset `off` of the staging buffer; counted either way
static const uint8_t *host_plane(Context *c, const uint8_t *view, const void *src, size_t bytes, const HostStage &st, size_t off) {
    if (view) {
        c->planes_in_place++;
        return view;
    }
    std::memcpy(st.h + off, src, bytes);
    c->planes_staged++;
    return st.dev + off;
}
}  // namespace lvt

using namespace lvt;

#include "lvt_stage_entries.h"
#include "lvt_frame_props.h"

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

LVT_API void lvt_amd_default_params(lvt_amd_params *p) { default_params(p); }
LVT_API int lvt_amd_params_from_file(const char *f, lvt_amd_params *p) { return params_from_file(f, p) ? 1 : 0; }

LVT_API lvt_handle lvt_amd_create_pooled(const lvt_amd_params *p, int sensor_type, int device) {
    try {
        return static_cast<lvt_handle>(pool_join(*p, sensor_type, device));
    } catch (...) {
    }
    return nullptr;
}

LVT_API lvt_handle lvt_amd_create(const lvt_amd_params *p, int sensor_type) {
    try {
        if (pool_wanted(-1))
            if (PoolSlot *S = pool_join(*p, sensor_type, -1)) return static_cast<lvt_handle>(S);
        return static_cast<lvt_handle>(create_context(*p, sensor_type, 1));
    } catch (...) {
    }
    return nullptr;
}

LVT_API lvt_handle lvt_amd_create_on_device(const lvt_amd_params *p, int sensor_type, int device) {
    try {
        if (pool_wanted(device))
            if (PoolSlot *S = pool_join(*p, sensor_type, device)) return static_cast<lvt_handle>(S);
        return static_cast<lvt_handle>(create_context(*p, sensor_type, 1, device));
    } catch (...) {
    }
    return nullptr;
}
LVT_API int lvt_amd_get_device(lvt_handle h) {
    if (is_auto(h)) return static_cast<AutoHandle *>(h)->device;  // (fixed at creation)
    if (is_slot(h)) return static_cast<PoolSlot *>(h)->pool->device;
    return h ? static_cast<Context *>(h)->device : -1;
}

LVT_API lvt_handle lvt_create(const char *config_file_name, int sensor_type) {
    try {
        lvt_amd_params p;
        default_params(&p);
        if (params_from_file(config_file_name, &p) && (sensor_type == 1 || sensor_type == 2)) {
            if (pool_wanted(-1))
                if (PoolSlot *S = pool_join(p, sensor_type, -1)) return static_cast<lvt_handle>(S);
            if (sensor_type == 1 && auto_pool_enabled()) return auto_create(p, -1);
            return static_cast<lvt_handle>(create_context(p, sensor_type, 1));
        }
    } catch (...) {
    }
    return nullptr;
}

LVT_API void lvt_destroy(lvt_handle h) {
    if (is_auto(h)) {
        try {
            auto_destroy(static_cast<AutoHandle *>(h));
        } catch (...) {
        }
        return;
    }
    if (is_slot(h)) {
        try {
            pool_leave(static_cast<PoolSlot *>(h));
        } catch (...) {
        }
        return;
    }
    if (h && std::getenv("LVT_AMD_HOST_TIMING")) {
        const Context *c = static_cast<Context *>(h);
        if (c->host_enq_n > 0)
            std::fprintf(stderr, "lvt_amd host timing: %ld frames enqueued, %.1f us each; %ld collected, %.1f us each (blocking)\n", c->host_enq_n,
                         c->host_enq_us / c->host_enq_n, c->host_wait_n, c->host_wait_us / std::max(c->host_wait_n, 1L));
    }
    try {
        DeviceGuard guard(static_cast<Context *>(h));
        delete static_cast<Context *>(h);
    } catch (...) {
    }
}

LVT_API void lvt_amd_reset(lvt_handle h) {
    h = resolve_handle(h);
    if (is_slot(h)) {
        try {
            View v;
            if (view_of(h, v)) reset_state(v.c, v.s);
            PoolSlot *S = static_cast<PoolSlot *>(h);
            std::memset(&S->last.rec, 0, sizeof(Ctl));
            S->last.rec.state = S->last.rec.out_status = 1;
            S->last.rec.out_R[0] = S->last.rec.out_R[4] = S->last.rec.out_R[8] = 1.0;
            S->last.rec.last_pose.q[0] = S->last.rec.predicted.q[0] = 1.0;
        } catch (...) {
        }
        return;
    }
    try {
        DeviceGuard guard(static_cast<Context *>(h));
        reset_state(static_cast<Context *>(h));
    } catch (...) {
    }
}

LVT_API void lvt_amd_set_stream(lvt_handle h, void *hip_stream) {
    h = resolve_handle(h);
    if (!is_ctx(h)) return;  // (a pooled handle runs on the pool's streams)
    Context *c = static_cast<Context *>(h);
    DeviceGuard guard(c);
    try {
        drain(c);  // the frames in flight are collected on the stream they were enqueued on ...
        HIPCHK(c, hipStreamSynchronize(c->stream));  // ... and what k_triangulate does behind a record's delivery has ended: nothing of this handle runs on the old stream
        if (!c->ev_caller) HIPCHK(c, hipEventCreateWithFlags(&c->ev_caller, hipEventDisableTiming));  // (refused: the handle stays on the stream it had)
        if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
        // hip_stream == NULL is the legacy default stream (what torch.cuda.current_stream().cuda_stream is on torch's default stream), for a batch as well: see create_context
        c->stream = static_cast<hipStream_t>(hip_stream);
        c->own_stream = false;
    } catch (...) {
    }
}

LVT_API const char *lvt_amd_last_error(lvt_handle h) {
    if (is_auto(h)) {  // answered under the record's lock: a handle that has not been used yet may be given a seat by another thread's lvt_create at any time
        AutoHandle *A = static_cast<AutoHandle *>(h);
        std::lock_guard<std::mutex> g(A->mu);
        static thread_local std::string acopy;
        acopy = lvt_amd_last_error(A->impl);
        return acopy.c_str();
    }
    if (!h) return g_call_refusal.empty() ? "no handle (creation failed: bad parameters, or no HIP device -- there is no CPU fallback)" : g_call_refusal.c_str();
    if (is_slot(h)) {
        PoolSlot *S = static_cast<PoolSlot *>(h);
        std::lock_guard<std::mutex> g(S->pool->mu);
        static thread_local std::string copy;
        copy = S->err;
        return copy.c_str();
    }
    Context *c = static_cast<Context *>(h);
    if (c->early_pending) {  // the last synchronous call returned on its pose: the frame's own reports (capacity overflow, a gate that
                             // timed out, a skipped frame) arrive with its full record -- collect it before answering
        DeviceGuard guard(c);
        try {
            drain(c);
        } catch (...) {
        }
    }
    if (c->capacity_report()) c->ovf_read_done = (long long)c->done;
    return c->err.c_str();
}

LVT_API void lvt_amd_get_host_stats(lvt_handle h, long long out[8]) {
    h = resolve_handle(h);
    Context *c = static_cast<Context *>(h);
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (!c) return;
    if (is_slot(h)) {  // out[0] frames this handle deposited, out[1] lock-step steps the pool launched, out[2] slot frames folded into them, out[3] live handles of the pool
        PoolSlot *S = static_cast<PoolSlot *>(h);
        std::lock_guard<std::mutex> g(S->pool->mu);
        out[0] = S->submitted, out[1] = S->pool->steps, out[2] = S->pool->slot_frames, out[3] = S->pool->live, out[7] = 2;
        return;
    }
    out[0] = (long long)c->enq + (c->pend.valid ? 1 : 0), out[1] = (long long)c->done, out[2] = c->planes_in_place, out[3] = c->planes_staged;
    out[4] = c->async_frames, out[5] = c->fused_pulls, out[6] = c->score_pieces, out[7] = c->events_only ? 1 : 0;
}

LVT_API void lvt_amd_profile_enable(lvt_handle h, int enable) {
    h = resolve_handle(h);
    if (!is_ctx(h)) return;
    Context *c = static_cast<Context *>(h);
    DeviceGuard guard(c);
    try {
        drain(c);
        if (enable) {
            for (auto &e : c->ev)
                for (auto &x : e)
                    if (!x) HIPCHK(c, hipEventCreate(&x));
            for (int i = 0; i < Context::PROF_SLOTS; i++) c->prof_ms[i] = 0, c->prof_calls[i] = 0;
        }
        c->prof = enable != 0;
    } catch (...) {
    }
}
LVT_API int lvt_amd_profile_read(lvt_handle h, int slot, char *name, int name_cap, double *total_ms, long *calls) {
    h = resolve_handle(h);
    if (!is_ctx(h)) return 0;
    Context *c = static_cast<Context *>(h);
    DeviceGuard guard(c);
    if (slot < 0 || slot >= Context::PROF_SLOTS || !kProfNames[slot][0]) return 0;
    if (slot == 4 && c->n_rect == 0 && c->prof_calls[4] == 0) return 0;  // (a handle without rectifiers has no such launch)
    if (slot == 14 && c->n_colour == 0 && c->prof_calls[14] == 0) return 0;  // (... and one without a colour sequence no k_gray_frames)
    if (slot == 15 && !c->pose_info && c->prof_calls[15] == 0) return 0;  // (... one that never enabled pose uncertainty no k_pose_info)
    if ((slot == 22 || slot == 23) && c->prof_calls[22] + c->prof_calls[23] == 0) return 0;  // (... and one that never took or applied a snapshot neither state kernel)
    if ((slot == 17 || slot == 21) && c->n_depth_cam == 0 && c->prof_calls[slot] == 0) return 0;  // (... and one without a depth camera no registration launches)
    if ((slot == 24 || slot == 25) && c->n_equal == 0 && c->prof_calls[slot] == 0) return 0;  // (... and one without an equalisation record neither of its launches)
    if (slot == 26 && c->n_mask == 0 && c->prof_calls[26] == 0) return 0;  // (... and one that never set a mask no k_mask_features)
    if (slot == 27 && c->n_guard == 0 && c->prof_calls[27] == 0) return 0;  // (... and one that never set a depth guard no k_depth_guard)
    if (slot == 28 && c->n_label == 0 && c->prof_calls[28] == 0) return 0;  // (... and one that never set a label-mask record no k_label_mask)
    if (slot == 29 && c->n_reduce == 0 && c->prof_calls[29] == 0) return 0;  // (... and one that never set a reduction no k_reduce_frames)
    if (slot == 30 && c->n_sensor == 0 && c->prof_calls[30] == 0) return 0;  // (... and one that never set a sensor format no k_sensor_frames)
    if ((slot == 31 || slot == 32) && c->n_sensor_auto == 0 && c->prof_calls[slot] == 0) return 0;  // (... and one without an auto window no k_sensor_hist / k_sensor_levels)
    std::snprintf(name, name_cap, "%s", kProfNames[slot]);
    *total_ms = c->prof_ms[slot];
    *calls = c->prof_calls[slot];
    return 1;
}

// lvt_amd_track_device (R, t handed back) and lvt_amd_track_device_async
static void track_device(lvt_handle h, const void *d_left, const void *d_right, int n_rows, int n_cols, int pitch_bytes, bool sync, double R[3][3], double t[3]) {
    static const char *who = "lvt_amd_track_device";
    h = resolve_handle(h);
    try {
        if (is_slot(h)) {
            PoolSlot *S = static_cast<PoolSlot *>(h);
            if (sync) slot_drain(S);
            if (slot_submit(S, static_cast<const uint8_t *>(d_left), static_cast<const uint8_t *>(d_right), n_rows, n_cols, pitch_bytes, false) != 0 || !sync) return;
            (void)slot_collect(S);
            slot_result(S, R, t);
            return;
        }
        // (an RGB-D frame needs a depth plane: lvt_amd_track_rgbd_device[_async])
        Context *c = frame_context(h, who, 1, true, {nullptr, "a stereo entry point on an RGB-D handle (the frame was NOT enqueued; use lvt_amd_track_rgbd_device)", nullptr});
        if (!c) return;
        DeviceGuard guard(c);
        if (!size_ok(c, n_rows, n_cols) || !device_pitch_ok(c, 0, pitch_bytes, n_cols) || !sensor_address_ok(c, 0, d_left, d_right)) {
            refuse(h, who, "image size / pitch mismatch");
            return;  // outputs untouched, like the reference on an exception
        }
        if (sync) {
            drain(c);
        } else {
            if (c->early_pending) drain(c);  // (a synchronous call's frame whose pose has already been returned: not this caller's to collect)
            make_room(c);
        }
        frame_args(c, next_slot(c)) = stereo_args(d_left, d_right, pitch_bytes);
        if (sync) track_sync(c, R, t);
        else enqueue_frame(c);
    } catch (...) {
    }
}
LVT_API void lvt_amd_track_device_async(lvt_handle h, const void *d_left, const void *d_right, int n_rows, int n_cols, int pitch_bytes) {
    track_device(h, d_left, d_right, n_rows, n_cols, pitch_bytes, false, nullptr, nullptr);
}

// ---- lock-step batch: B independent sequences advance through ONE launch chain (gridDim.z = B) ------------
LVT_API lvt_handle lvt_amd_batch_create(const lvt_amd_params *p, int sensor_type, int n_sequences) {
    try {
        if (n_sequences < 1 || n_sequences > 256) return nullptr;
        return static_cast<lvt_handle>(create_context(*p, sensor_type, n_sequences));
    } catch (...) {
    }
    return nullptr;
}
// B sequences, sequence s with parameters p[s]: see Context::mixed
LVT_API lvt_handle lvt_amd_batch_create_mixed(const lvt_amd_params *p, int sensor_type, int n_sequences) {
    try {
        if (!p || n_sequences < 1 || n_sequences > 256) return nullptr;
        return static_cast<lvt_handle>(create_context(p, true, sensor_type, n_sequences, -1));
    } catch (...) {
    }
    return nullptr;
}
// the work tables a mixed batch of these parameters would launch its k_cells / k_score from (build_mixed_tables; no GPU needed): counts[0 / 1] = entries of the
// cells / score table, of which min(count, cap) are written.  0: a parameter set lvt_amd_batch_create_mixed refuses.
LVT_API int lvt_amd_batch_mixed_tables(const lvt_amd_params *p, int sensor_type, int n_sequences, unsigned *cells, int cells_cap, unsigned *score, int score_cap,
                                       int counts[2]) {
    try {
        if (!p || n_sequences < 1 || n_sequences > 256 || (sensor_type != 1 && sensor_type != 2)) return 0;
        std::vector<Params> ps(n_sequences);
        for (int s = 0; s < n_sequences; s++)
            if (!derive_params(p[s], sensor_type, ps[s])) return 0;
        std::vector<uint32_t> ct, st;
        if (!build_mixed_tables(ps, ct, st)) return 0;
        if (counts) counts[0] = (int)ct.size(), counts[1] = (int)st.size();
        for (int i = 0; cells && i < cells_cap && i < (int)ct.size(); i++) cells[i] = ct[i];
        for (int i = 0; score && i < score_cap && i < (int)st.size(); i++) score[i] = st[i];
        return 1;
    } catch (...) {
    }
    return 0;
}
LVT_API int lvt_amd_batch_get_params(lvt_handle h, int seq, lvt_amd_params *out) {
    h = resolve_handle(h, false);
    if (!is_ctx(h) || !out) return 0;
    Context *c = static_cast<Context *>(h);
    if (seq < 0 || seq >= c->B || c->in_prms.empty()) return 0;
    *out = c->in_prms[c->mixed ? seq : 0];
    return 1;
}
LVT_API int lvt_amd_batch_size(lvt_handle h) {
    h = resolve_handle(h, false);
    return is_ctx(h) ? static_cast<Context *>(h)->B : 0;
}

// one lock-step step with per-sequence image geometry; d_left[s] == NULL: sequence s has no frame in it (FrameArgs::absent, the pooled seats' mechanism).
// Everything is checked before anything is enqueued.
LVT_API int lvt_amd_batch_track_device_async_mixed(lvt_handle h, const void *const *d_left, const void *const *d_right, const int *n_rows, const int *n_cols,
                                                   const int *pitch_bytes) {
    static const char *who = "lvt_amd_batch_track_device_async_mixed";
    h = resolve_handle(h);
    Context *c = frame_context(h, who, 0, true);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        if (!d_left || !d_right || !n_rows || !n_cols || !pitch_bytes) return refuse(h, who, "NULL argument");
        if (c->sensor != 1) return refuse(h, who, "a stereo entry point on an RGB-D batch (nothing was enqueued; use lvt_amd_batch_track_rgbd_device_async)");
        int present = 0;
        for (int s = 0; s < c->B; s++) {
            if (!d_left[s]) continue;
            present++;
            const int fW = c->frame_W(s), fH = c->frame_H(s);  // (a sequence with rectifiers: their source's size)
            if (!d_right[s] || n_rows[s] != fH || n_cols[s] != fW || !device_pitch_ok(c, s, pitch_bytes[s], n_cols[s]) || pitch_bytes[s] < n_cols[s] || !sensor_address_ok(c, s, d_left[s], d_right[s])) {
                char buf[200];
                std::snprintf(buf, sizeof(buf), "sequence %d: image size / pitch mismatch (%d x %d, pitch %d; expected %d x %d, pitch %s)",
                              s, n_cols[s], n_rows[s], pitch_bytes[s], fW, fH, c->has_sensor(s) ? "at least a row of the sensor's plane (MONO16: even, at an even address)" : c->fmt_of(s) != PIX_GRAY8 ? "at least a row of colour pixels" : (c->has_rect(s) || c->has_equal(s) || c->has_reduce(s)) ? "at least the width" : "a multiple of 16");
                return refuse(h, who, buf);
            }
        }
        if (!present) return refuse(h, who, "no sequence has a frame in this step");
        make_room(c);
        for (int s = 0; s < c->B; s++) frame_args(c, next_slot(c), s) = d_left[s] ? stereo_args(d_left[s], d_right[s], pitch_bytes[s]) : absent_args();
        enqueue_frame(c);
        return 0;
    } catch (...) {
    }
    return -1;
}

LVT_API void lvt_amd_batch_track_device_async(lvt_handle h, const void *const *d_left, const void *const *d_right, int n_rows, int n_cols,
                                              int pitch_bytes) {
    static const char *who = "lvt_amd_batch_track_device";
    h = resolve_handle(h);
    Context *c = frame_context(h, who, 1, true, {nullptr, "a stereo entry point on an RGB-D batch (nothing was enqueued; use lvt_amd_batch_track_rgbd_device_async)", nullptr});
    if (!c) return;
    DeviceGuard guard(c);
    try {
        if (c->mixed) {
            refuse(h, who, "a mixed batch takes its frames through lvt_amd_batch_track_device_async_mixed");
            return;
        }
        bool pitch_ok = true;  // (one pitch for the whole step: it must suit the raw and the rectified sequences alike)
        bool sizes_ok = true;  // (... and one size: a sequence whose rectifiers have another source size than the rest needs the mixed call)
        for (int s = 0; s < c->B; s++) {
            pitch_ok = pitch_ok && device_pitch_ok(c, s, pitch_bytes, n_cols) && sensor_address_ok(c, s, d_left[s], d_right[s]);
            sizes_ok = sizes_ok && n_rows == c->frame_H(s) && n_cols == c->frame_W(s);
        }
        if (!sizes_ok || !pitch_ok) {
            refuse(h, who, "image size / pitch mismatch");
            return;
        }
        make_room(c);
        for (int s = 0; s < c->B; s++) frame_args(c, next_slot(c), s) = stereo_args(d_left[s], d_right[s], pitch_bytes);
        enqueue_frame(c);
    } catch (...) {
    }
}
// poses of the oldest un-collected batch frame: R = B x 9 doubles (row-major 3x3 each), t = B x 3, status = B ints
LVT_API void lvt_amd_batch_wait(lvt_handle h, double *R, double *t, int *status) {
    h = resolve_handle(h);
    if (!is_ctx(h)) return;
    Context *c = static_cast<Context *>(h);
    DeviceGuard guard(c);
    try {
        if (c->done < c->enq) collect_oldest(c);
        for (int s = 0; s < c->B; s++) {
            const Ctl &k = last_ctl(c, s);
            if (R) for (int i = 0; i < 9; i++) R[9 * s + i] = k.out_R[i];
            if (t) for (int i = 0; i < 3; i++) t[3 * s + i] = k.out_t[i];
            if (status) status[s] = k.state;
        }
    } catch (...) {
    }
}
LVT_API void lvt_amd_batch_get_counts(lvt_handle h, int seq, int out[LVT_AMD_C__COUNT]) {
    h = resolve_handle(h);
    if (!is_ctx(h)) return;
    Context *c = static_cast<Context *>(h);
    DeviceGuard guard(c);
    try {
        drain(c);
        if (seq < 0 || seq >= c->B) return;
        for (int i = 0; i < LVT_AMD_C__COUNT; i++) out[i] = last_ctl(c, seq).counts[i];
    } catch (...) {
    }
}

LVT_API int lvt_amd_wait_status(lvt_handle h, double R[3][3], double t[3]) {  // lvt_amd_wait + the tracking state AFTER that frame (1 / 2 / 3; -1: error)
    h = resolve_handle(h);
    try {
        if (is_slot(h)) {
            PoolSlot *S = static_cast<PoolSlot *>(h);
            (void)slot_collect(S);
            slot_result(S, R, t);
            return S->last.rec.state;
        }
        Context *c = frame_context(h, "lvt_amd_wait", 0, true);
        if (!c) return -1;
        DeviceGuard guard(c);
        if (c->early_pending) drain(c);
        if (c->enq - c->done <= 1) flush_pending(c);  // (a held host frame: kept back only while the device has other frames to work on)
        if (c->done < c->enq) collect_oldest(c);  // FIFO: the oldest frame not yet collected
        result_out(c, 0, R, t);
        return last_ctl(c).state;
    } catch (...) {
    }
    return -1;
}
LVT_API void lvt_amd_wait(lvt_handle h, double R[3][3], double t[3]) { (void)lvt_amd_wait_status(h, R, t); }

// lvt_amd_wait_status with the pose as the tracker holds it (quaternion w x y z + position) instead of R, t: what lvt_system::track returns
LVT_API int lvt_amd_wait_pose(lvt_handle h, double q_wxyz[4], double p[3]) {
    h = resolve_handle(h);
    double R[3][3], t[3];
    const int st = lvt_amd_wait_status(h, R, t);
    if (st < 0) return st;
    const Ctl *rec = nullptr;
    if (is_slot(h)) rec = &static_cast<PoolSlot *>(h)->last.rec;
    else if (is_ctx(h)) rec = &last_ctl(static_cast<Context *>(h));
    if (!rec) return -1;
    for (int k = 0; k < 4; k++) q_wxyz[k] = rec->last_pose.q[k];
    for (int k = 0; k < 3; k++) p[k] = rec->last_pose.p[k];
    return st;
}

LVT_API void lvt_amd_track_device(lvt_handle h, const void *d_left, const void *d_right, int n_rows, int n_cols, int pitch_bytes,
                                  double R[3][3], double t[3]) {
    track_device(h, d_left, d_right, n_rows, n_cols, pitch_bytes, true, R, t);
}

// the context's own colour planes (Context::d_col / d_col_ring), allocated when first needed and sized for 4 bytes per pixel: the format may change later
static void colour_planes(Context *c, uint8_t *(&d)[2], int eyes) {
    for (int e = 0; e < eyes; e++)
        if (!d[e]) d[e] = c->dalloc<uint8_t>((size_t)((c->frame_W(0) * 4 + 63) / 64 * 64) * c->frame_H(0) + 64);
}
// the context's own raw planes of a RESIZED handle (Context::d_raw / d_raw_ring), allocated when first needed at the source's size
static void raw_planes(Context *c, uint8_t *(&d)[2], int eyes = 2) {
    for (int e = 0; e < eyes; e++)
        if (!d[e]) d[e] = c->dalloc<uint8_t>((size_t)c->frame_pitch(0) * c->frame_H(0) + 64);
}
// the context's own depth planes of the synchronous host calls (Context::d_depth) hold dpix pixels: allocated at creation for the image's size, again when a
// depth camera with a larger plane has been set (no frame is in flight then)
static void depth_planes(Context *c, size_t dpix) {
    if (c->depth_cap >= dpix) return;
    drain(c);  // (once per larger camera)
    for (int par = 0; par < NPAR; par++) {
        c->dfree(c->d_depth[par]);  // (the smaller planes: nothing in flight reads them)
        c->d_depth[par] = c->dalloc<float>(dpix + 4);
    }
    c->depth_cap = dpix;
}
// (dfmt / dscale: element format of an RGB-D frame's depth plane `second` and metres per raw unit of a 16-bit one; cl / cr: external corner lists, nullptr: none)
static void upload_and_track(Context *c, const unsigned char *left, const void *second, bool rgbd, int n_rows, int n_cols,
                             const float *cl, int ncl, const float *cr, int ncr, double R[3][3], double t[3], int dfmt = DEPTH_F32, float dscale = 0.f) {
    const size_t desz = (dfmt == DEPTH_U16) ? sizeof(uint16_t) : sizeof(float);
    if (!size_ok(c, n_rows, n_cols)) {
        refuse(c, "lvt_track", "image size differs from the configured img_width/img_height");
        return;
    }
    if (rgbd && reduced_without_depth_camera(c, 0)) {
        refuse(c, "lvt_amd_track_rgbd", std::string(kReducedNoDepthCamera) + " (nothing was enqueued)");
        return;
    }
    // (the previous synchronous call may have returned on its early pose: its frame's tail -- staged update, triangulation -- runs
    //  while this call copies the new images into the staging buffer of THIS frame's feature buffer; the drain comes after)
    flush_pending(c);  // a held lvt_amd_track_async frame goes out FIRST: it takes a frame number, and this frame's buffers (images, corner lists) are chosen by number
    const int par = (int)(c->enq % NPAR);
    hipStream_t sf = c->stream_f;
    // a COLOUR handle: the image is a byte image n_cols * bpp wide; it is pulled into the context's colour planes and enqueue_frame converts it from there
    const int bpp = c->bpp_of(0), row_bytes = n_cols * bpp;
    const size_t npix = (size_t)n_rows * n_cols, nbytes = npix * bpp;
    const bool raw = !c->converts(0) && c->resized(0);  // (gray raw frames of another size than the tracker's: planes of their own)
    const bool conv = c->converts(0);  // (a colour or a sensor format: a Bayer mosaic has bpp == 1 and still converts)
    if (conv) colour_planes(c, c->d_col[par], rgbd ? 1 : 2);
    if (raw) raw_planes(c, c->d_raw[par], rgbd ? 1 : 2);
    uint8_t *const *dimg = conv ? c->d_col[par] : raw ? c->d_raw[par] : c->d_img[par];
    const int ipitch = conv ? c->colour_pitch() : c->frame_pitch(0);
    // (a handle with a depth camera: the depth plane is the sensor's, the camera's size -- staged, pulled and handed on unchanged)
    const size_t dpix = rgbd ? c->depth_px() : 0;
    const int dcols = c->depth_cols();
    if (rgbd) depth_planes(c, dpix);
    const HostStage &stg = c->stage[par];
    stage_reserve(c, c->stage[par], nbytes, dpix);
    // (this call only returns after the frame has been tracked, so a page-locked buffer read in place outlives every read)
    const uint8_t *v0 = device_view(left, 1), *v1 = device_view(second, rgbd ? desz : 1);
    // The pulls are launched BEFORE the previous frame is collected: this frame's image planes (parity `par`) and staging buffer were last used NPAR
    // frames ago, and what may still be running -- the tail of the previous synchronous call, which returned on its early pose -- reads neither.
    // Two pageable images: the left one is pulled while the CPU still copies the right one.
    const bool split = !rgbd && !v0 && !v1;
    const uint8_t *s0 = host_plane(c, v0, left, nbytes, stg, 0), *s1 = v1;  // (an RGB-D frame's second plane goes later: before_gather)
    if (split) hipLaunchKernelGGL(k_stage_in, dim3(128, 1), dim3(256), 0, sf, s0, s0, dimg[0], dimg[0], row_bytes, n_rows, ipitch);
    if (!rgbd) s1 = host_plane(c, v1, second, nbytes, stg, stg.second);
    if (split) hipLaunchKernelGGL(k_stage_in, dim3(128, 1), dim3(256), 0, sf, s1, s1, dimg[1], dimg[1], row_bytes, n_rows, ipitch);
    else hipLaunchKernelGGL(k_stage_in, dim3(128, rgbd ? 1 : 2), dim3(256), 0, sf, s0, s1, dimg[0], dimg[1], row_bytes, n_rows, ipitch);
    drain(c);
    FrameArgs f = stereo_args(dimg[0], dimg[(rgbd && (conv || raw)) ? 0 : 1], ipitch);  // (an RGB-D handle has one colour plane, and one raw plane)
    if (rgbd) {
        // The depth plane (1.2 MB: ~60 us of CPU copy into the staging buffer when the caller's buffer is pageable, ~45 us of PCIe pull)
        // is not needed before k_gather's depth filter.  Both happen once the detection kernels are enqueued -- the copy on the
        // host while the GPU runs them, the pull on the early stream (idle until this frame's features exist) beside them -- and
        // the feature stream waits for the pull in front of k_gather.  (A 16-bit plane: half those bytes, both ways; it stays 16-bit in d_depth.)
        f = with_depth(f, c->d_depth[par], dcols * (int)desz, dfmt, dscale);
        // (runs inside enqueue_frame: everything it needs travels by value, nothing is read that enqueue_frame advances)
        c->before_gather = [c, v1, second, dpix, par, sf, dfmt, desz]() {
            const uint8_t *src = host_plane(c, v1, second, desz * dpix, c->stage[par], c->stage[par].second);
            hipStream_t sd = c->events_only ? sf : c->stream_e;
            launch_stage_copy(sd, src, c->d_depth[par], dpix, dfmt);
            if (sd != sf) {
                (void)hipEventRecord(c->ev_depth, sd);
                c->depth_wait = true;
            }
        };
    }
    if (cl) {  // (the context's own lists, d_ext[par])
        f = with_corners(f, ncl, ncr);
        if (ncl) HIPCHK(c, hipMemcpyAsync(c->d_ext[par][0], cl, sizeof(float) * 2 * (size_t)ncl, hipMemcpyHostToDevice, sf));
        if (ncr) HIPCHK(c, hipMemcpyAsync(c->d_ext[par][1], cr, sizeof(float) * 2 * (size_t)ncr, hipMemcpyHostToDevice, sf));
    }
    frame_args(c, next_slot(c)) = f;
    track_sync(c, R, t);
}

// Asynchronous counterpart of upload_and_track (lvt_amd_track_async / lvt_amd_track_rgbd_async): borrowed HOST images, the frame is enqueued and the
// call returns; the pose comes out of the same FIFO as lvt_amd_track_device_async's (lvt_amd_wait / lvt_amd_wait_status).  Pageable buffers are copied
// into this slot's pinned staging buffer during the call; page-locked ones are pulled where they lie (and must stay valid until the frame is collected).
// Stereo: the frame is HELD (Context::pend) until the next one arrives -- its k_cells launch then carries the workgroups that pull that next frame's
// images (24 us of PCIe reads beside 66 us of corner cells: on no stream's chain; SURVEY 8e "pinned H2D staging double-buffered") -- or until
// lvt_amd_wait* finds the device about to run dry / any other entry point needs the launch chain.  A frame nobody pulled for pulls its own images at the
// head of its feature stage (k_stage_in), as every RGB-D frame does.
// Returns 0 when the frame was enqueued, -1 when it was rejected (nothing enqueued; lvt_amd_last_error says why).
static int upload_async(Context *c, const unsigned char *left, const void *second, bool rgbd, int n_rows, int n_cols, int dfmt = DEPTH_F32, float dscale = 0.f) {
    static const char *who = "lvt_amd_track_async";
    const size_t desz = (dfmt == DEPTH_U16) ? sizeof(uint16_t) : sizeof(float);
    if (c->B != 1 || (rgbd ? c->sensor != 2 : c->sensor != 1)) return refuse(c, who, "wrong sensor type for this entry point (or a batch handle)");
    if (!left || !second || !size_ok(c, n_rows, n_cols))
        return refuse(c, who, "image size differs from the configured img_width/img_height (the frame was NOT enqueued)");
    if (rgbd && reduced_without_depth_camera(c, 0)) return refuse(c, who, std::string(kReducedNoDepthCamera) + " (nothing was enqueued)");
    if (c->early_pending) drain(c);
    if (rgbd) flush_pending(c);
    const int held = c->pend.valid ? 1 : 0;  // (the held frame owns slot enq % RING)
    while (c->enq + held - c->done >= RING - 1) collect_oldest(c);
    const int slot = (int)((c->enq + held) % RING);
    // (a COLOUR handle: byte images n_cols * bpp wide into the context's colour planes, as in upload_and_track; the fused pull carries them like gray ones)
    const int bpp = c->bpp_of(0), row_bytes = n_cols * bpp;
    const size_t npix = (size_t)n_rows * n_cols, nbytes = npix * bpp, plane = (size_t)c->pitch * c->prm.H;
    const bool conv = c->converts(0), raw = !conv && c->resized(0);  // (as in upload_and_track)
    if (conv) colour_planes(c, c->d_col_ring[slot], rgbd ? 1 : 2);
    if (raw) raw_planes(c, c->d_raw_ring[slot], rgbd ? 1 : 2);
    const int ipitch = conv ? c->colour_pitch() : c->frame_pitch(0);
    const size_t dpix = rgbd ? c->depth_px() : 0;  // (a handle with a depth camera: the sensor's plane, the camera's size)
    const int dcols = c->depth_cols();
    if (!raw && !c->d_img_ring[0][0]) {  // first asynchronous host-buffer call
        for (int r = 0; r < RING; r++)
            for (int e = 0; e < (rgbd ? 1 : 2); e++) c->d_img_ring[r][e] = c->dalloc<uint8_t>(plane + 64);
    }
    if (rgbd && c->depth_ring_cap < dpix) {  // (first call, or a depth camera with a larger plane was set since: no frame is in flight then)
        drain(c);  // (once per larger camera; enq stays: an RGB-D handle holds no frame back)
        for (int r = 0; r < RING; r++) {
            c->dfree(c->d_depth_ring[r]);
            c->d_depth_ring[r] = c->dalloc<float>(dpix + 4);
        }
        c->depth_ring_cap = dpix;
    }
    const uint8_t *v0 = device_view(left, 1), *v1 = device_view(second, rgbd ? desz : 1);
    HostStage &stg = c->stage_ring[slot];
    if (!v0 || !v1) stage_reserve(c, stg, nbytes, dpix);
    hipStream_t sp = c->stream_f;
    uint8_t *const *dring = conv ? c->d_col_ring[slot] : raw ? c->d_raw_ring[slot] : c->d_img_ring[slot];
    uint8_t *d0 = dring[0], *d1 = dring[1];
    const uint8_t *s0 = host_plane(c, v0, left, nbytes, stg, 0);
    if (!rgbd) {
        const uint8_t *s1 = host_plane(c, v1, second, nbytes, stg, stg.second);
        // the frame held so far goes out now, and its k_cells launch pulls THIS frame's images beside its cells
        const bool carried = c->pend.valid && c->fuse_pull;
        if (c->pend.valid) {
            const NextPull np{{s0, s1}, {d0, d1}, row_bytes, n_rows, ipitch};
            flush_pending(c, carried ? &np : nullptr);
        }
        Context::PendingFrame &q = c->pend;
        q.valid = true, q.pulled = carried;
        q.src[0] = s0, q.src[1] = s1, q.dst[0] = d0, q.dst[1] = d1;
        q.row_bytes = row_bytes, q.rows = n_rows, q.pitch = ipitch;
        q.f = stereo_args(d0, d1, ipitch);
        c->async_frames++;
        if (!c->fuse_pull) flush_pending(c);
        return 0;
    }
    hipLaunchKernelGGL(k_stage_in, dim3(128, 1), dim3(256), 0, sp, s0, s0, d0, d0, row_bytes, n_rows, ipitch);
    launch_stage_copy(sp, host_plane(c, v1, second, desz * dpix, stg, stg.second), c->d_depth_ring[slot], dpix, dfmt);
    frame_args(c, slot) = rgbd_args(d0, ipitch, c->d_depth_ring[slot], dcols * (int)desz, dfmt, dscale);
    c->async_frames++;
    enqueue_frame(c);
    return 0;
}

LVT_API int lvt_amd_track_async(lvt_handle h, const unsigned char *left, const unsigned char *right, int n_rows, int n_cols) {
    h = resolve_handle(h);
    try {
        if (is_slot(h)) return slot_submit(static_cast<PoolSlot *>(h), left, right, n_rows, n_cols, 0, true);
        Context *c = frame_context(h, "lvt_amd_track_async", 0, true);
        if (!c) return -1;
        DeviceGuard guard(c);
        return upload_async(c, left, right, false, n_rows, n_cols);
    } catch (...) {
    }
    return -1;
}
LVT_API int lvt_amd_track_rgbd_async(lvt_handle h, const unsigned char *gray, const float *depth, int n_rows, int n_cols) {
    h = resolve_handle(h);
    Context *c = frame_context(h, "lvt_amd_track_async", 0, true);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        return upload_async(c, gray, depth, true, n_rows, n_cols);
    } catch (...) {
    }
    return -1;
}

LVT_API void lvt_track(lvt_handle h, unsigned char *left, unsigned char *right, int n_rows, int n_cols, double R[3][3], double t[3]) {
    h = resolve_handle(h);
    try {
        if (is_slot(h)) {
            PoolSlot *S = static_cast<PoolSlot *>(h);
            slot_drain(S);
            if (slot_submit(S, left, right, n_rows, n_cols, 0, true) != 0) return;  // outputs untouched, like the reference on an exception
            (void)slot_collect(S);
            slot_result(S, R, t);
            return;
        }
        Context *c = frame_context(h, "lvt_track", 1, true);  // the reference cannot run RGB-D through this entry either
        if (!c) return;
        DeviceGuard guard(c);
        upload_and_track(c, left, right, false, n_rows, n_cols, nullptr, 0, nullptr, 0, R, t);
    } catch (...) {
    }
}

LVT_API void lvt_amd_track_rgbd(lvt_handle h, const unsigned char *gray, const float *depth, int n_rows, int n_cols, double R[3][3],
                                double t[3]) {
    h = resolve_handle(h);
    Context *c = frame_context(h, "lvt_amd_track_rgbd", 2, true);
    if (!c) return;
    DeviceGuard guard(c);
    try {
        upload_and_track(c, gray, depth, true, n_rows, n_cols, nullptr, 0, nullptr, 0, R, t);
    } catch (...) {
    }
}

// ---- RGB-D beyond the two host fp32 calls: planes already in HBM, 16-bit depth, lock-step batches -------------------------------------------
// Every call checks everything before it enqueues anything: 0 = enqueued / tracked, -1 = refused, NOTHING enqueued, the reason in lvt_amd_last_error.
static int rgbd_refuse(lvt_handle h, const char *who, const std::string &why) { return refuse(h, who, why + " (nothing was enqueued)"); }
// the handle must be a solo (B == 1) or batch (B > 1 or mixed) RGB-D context
static Context *rgbd_context(lvt_handle h, const char *who, bool batch) {
    return frame_context(h, who, 2, batch, {"a pooled handle (pooled handles are stereo only) (nothing was enqueued)", "an RGB-D entry point on a stereo handle (nothing was enqueued)",
                                            "a batch handle takes its frames through lvt_amd_batch_track_rgbd_device_async (nothing was enqueued)"});
}
static bool depth_format_ok(lvt_handle h, const char *who, int fmt, float scale) {
    if (fmt != DEPTH_F32 && fmt != DEPTH_U16) {
        rgbd_refuse(h, who, "unknown depth format " + std::to_string(fmt));
        return false;
    }
    if (fmt == DEPTH_U16 && !(std::isfinite(scale) && scale > 0.f)) {
        rgbd_refuse(h, who, "depth_scale of a 16-bit depth plane must be finite and > 0");
        return false;
    }
    return true;
}
// one sequence's device planes against its parameters; "" when they pass (dcols: the width of its depth plane -- its depth camera's, else the image's)
// (fW x fH: the sequence's frame size -- its own, or its reduction's; large: a reduction is in force, and k_reduce_frames reads the gray plane in place)
static std::string rgbd_planes_check(int fW, int fH, bool large, const void *d_gray, int gray_pitch, const void *d_depth, int depth_pitch, int fmt, int n_rows, int n_cols, int bpp, int dcols, int sfmt = SENSOR_NONE) {
    const int esz = (fmt == DEPTH_U16) ? 2 : 4;
    char buf[240];
    if (!d_gray || !d_depth) return "NULL gray or depth plane";
    if (n_rows != fH || n_cols != fW) {
        std::snprintf(buf, sizeof(buf), "image size %d x %d, expected %d x %d", n_cols, n_rows, fW, fH);
        return buf;
    }
    if (sfmt != SENSOR_NONE) {  // a sensor's plane: k_sensor_frames reads it in place -- any address, any pitch that holds a row (MONO16: both even)
        if ((long long)gray_pitch < (long long)n_cols * bpp) {
            std::snprintf(buf, sizeof(buf), "sensor plane: pitch (%d) must hold a row of %d bytes", gray_pitch, n_cols * bpp);
            return buf;
        }
        if (sfmt == SENSOR_MONO16 && (((uintptr_t)d_gray | (uintptr_t)(unsigned)gray_pitch) & 1)) {
            std::snprintf(buf, sizeof(buf), "sensor plane: a MONO16 plane needs an even address and an even pitch (%d)", gray_pitch);
            return buf;
        }
    } else if (large && bpp == 1) {  // a large gray frame: any address, any pitch that holds a row
        if (gray_pitch < n_cols) {
            std::snprintf(buf, sizeof(buf), "gray plane: pitch (%d) must hold a row of %d bytes", gray_pitch, n_cols);
            return buf;
        }
    } else if (bpp > 1) {  // a colour sequence: k_gray_frames reads the plane byte-wise -- any address, any pitch that holds a row
        if ((long long)gray_pitch < (long long)n_cols * bpp) {
            std::snprintf(buf, sizeof(buf), "colour plane: pitch (%d) must hold a row of %d bytes", gray_pitch, n_cols * bpp);
            return buf;
        }
    } else if (((uintptr_t)d_gray & 15) || (gray_pitch & 15) || gray_pitch < n_cols) {
        std::snprintf(buf, sizeof(buf), "gray plane: pointer and pitch (%d) must be multiples of 16, pitch >= %d", gray_pitch, n_cols);
        return buf;
    }
    if (((uintptr_t)d_depth % esz) || depth_pitch <= 0 || (depth_pitch % esz) || (long long)depth_pitch < (long long)dcols * esz) {
        std::snprintf(buf, sizeof(buf), "depth plane: pointer and pitch (%d bytes) must be multiples of the %d-byte element, pitch >= %d", depth_pitch, esz, dcols * esz);
        return buf;
    }
    return "";
}

// lvt_amd_track_rgbd_device (R, t handed back) and lvt_amd_track_rgbd_device_async
static int track_rgbd_device(lvt_handle h, const void *d_gray, int gray_pitch_bytes, const void *d_depth, int depth_pitch_bytes, int depth_format, float depth_scale,
                             int n_rows, int n_cols, bool sync, double R[3][3], double t[3]) {
    static const char *who = "lvt_amd_track_rgbd_device";
    h = resolve_handle(h);
    Context *c = rgbd_context(h, who, false);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        if (!depth_format_ok(h, who, depth_format, depth_scale)) return -1;
        if (reduced_without_depth_camera(c, 0)) return rgbd_refuse(h, who, kReducedNoDepthCamera);
        const std::string why = rgbd_planes_check(c->frame_W(0), c->frame_H(0), c->has_reduce(0), d_gray, gray_pitch_bytes, d_depth, depth_pitch_bytes, depth_format, n_rows, n_cols, c->bpp_of(0), c->depth_cols(), c->has_sensor(0) ? c->sens[0].format : SENSOR_NONE);
        if (!why.empty()) return rgbd_refuse(h, who, why);
        if (sync) {
            drain(c);
        } else {
            if (c->early_pending) drain(c);
            make_room(c);
        }
        frame_args(c, next_slot(c)) = rgbd_args(d_gray, gray_pitch_bytes, d_depth, depth_pitch_bytes, depth_format, depth_scale);
        if (sync) track_sync(c, R, t);
        else enqueue_frame(c);
        return 0;
    } catch (...) {
    }
    return -1;
}
LVT_API int lvt_amd_track_rgbd_device_async(lvt_handle h, const void *d_gray, int gray_pitch_bytes, const void *d_depth, int depth_pitch_bytes, int depth_format,
                                            float depth_scale, int n_rows, int n_cols) {
    return track_rgbd_device(h, d_gray, gray_pitch_bytes, d_depth, depth_pitch_bytes, depth_format, depth_scale, n_rows, n_cols, false, nullptr, nullptr);
}
LVT_API int lvt_amd_track_rgbd_device(lvt_handle h, const void *d_gray, int gray_pitch_bytes, const void *d_depth, int depth_pitch_bytes, int depth_format,
                                      float depth_scale, int n_rows, int n_cols, double R[3][3], double t[3]) {
    return track_rgbd_device(h, d_gray, gray_pitch_bytes, d_depth, depth_pitch_bytes, depth_format, depth_scale, n_rows, n_cols, true, R, t);
}

// HOST buffers with 16-bit depth (what the sensor delivers: TUM's PNGs are uint16 at 1/5000 m), tightly packed like lvt_amd_track_rgbd's: the staging copy
// and the PCIe pull keep their place behind the detection kernels, at half the bytes
static Context *rgbd16_context(lvt_handle h, const char *who, const void *gray, const void *depth16, float depth_scale, int n_rows, int n_cols) {
    Context *c = rgbd_context(h, who, false);
    if (!c) return nullptr;
    if (!depth_format_ok(h, who, DEPTH_U16, depth_scale)) return nullptr;
    if (!gray || !depth16 || ((uintptr_t)depth16 & 1)) {
        rgbd_refuse(h, who, "NULL buffer, or a depth buffer that is not 2-byte aligned");
        return nullptr;
    }
    if (!size_ok(c, n_rows, n_cols)) {
        rgbd_refuse(h, who, "image size differs from the configured img_width/img_height");
        return nullptr;
    }
    return c;
}
LVT_API int lvt_amd_track_rgbd16(lvt_handle h, const unsigned char *gray, const uint16_t *depth16, float depth_scale, int n_rows, int n_cols, double R[3][3],
                                 double t[3]) {
    h = resolve_handle(h);
    Context *c = rgbd16_context(h, "lvt_amd_track_rgbd16", gray, depth16, depth_scale, n_rows, n_cols);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        upload_and_track(c, gray, depth16, true, n_rows, n_cols, nullptr, 0, nullptr, 0, R, t, DEPTH_U16, depth_scale);
        return 0;
    } catch (...) {
    }
    return -1;
}
LVT_API int lvt_amd_track_rgbd16_async(lvt_handle h, const unsigned char *gray, const uint16_t *depth16, float depth_scale, int n_rows, int n_cols) {
    h = resolve_handle(h);
    Context *c = rgbd16_context(h, "lvt_amd_track_rgbd16_async", gray, depth16, depth_scale, n_rows, n_cols);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        return upload_async(c, gray, depth16, true, n_rows, n_cols, DEPTH_U16, depth_scale);
    } catch (...) {
    }
    return -1;
}

// one lock-step step of an RGB-D batch, uniform or mixed: arrays of B; d_gray[s] == NULL: sequence s sits this step out (FrameArgs::absent)
LVT_API int lvt_amd_batch_track_rgbd_device_async(lvt_handle h, const void *const *d_gray, const void *const *d_depth, const int *n_rows, const int *n_cols,
                                                  const int *gray_pitch_bytes, const int *depth_pitch_bytes, int depth_format, float depth_scale) {
    static const char *who = "lvt_amd_batch_track_rgbd_device_async";
    h = resolve_handle(h);
    Context *c = rgbd_context(h, who, true);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        if (!d_gray || !d_depth || !n_rows || !n_cols || !gray_pitch_bytes || !depth_pitch_bytes) return rgbd_refuse(h, who, "NULL argument");
        if (!depth_format_ok(h, who, depth_format, depth_scale)) return -1;
        int present = 0;
        for (int s = 0; s < c->B; s++) {
            if (!d_gray[s]) continue;
            present++;
            if (reduced_without_depth_camera(c, s)) return rgbd_refuse(h, who, "sequence " + std::to_string(s) + ": " + kReducedNoDepthCamera);
            const std::string why = rgbd_planes_check(c->frame_W(s), c->frame_H(s), c->has_reduce(s), d_gray[s], gray_pitch_bytes[s], d_depth[s], depth_pitch_bytes[s], depth_format, n_rows[s], n_cols[s], c->bpp_of(s),
                                                      c->has_depth_cam(s) ? c->depth_cam[(size_t)s].width : n_cols[s], c->has_sensor(s) ? c->sens[(size_t)s].format : SENSOR_NONE);
            if (!why.empty()) return rgbd_refuse(h, who, "sequence " + std::to_string(s) + ": " + why);
        }
        if (!present) return rgbd_refuse(h, who, "no sequence has a frame in this step");
        make_room(c);
        for (int s = 0; s < c->B; s++)
            frame_args(c, next_slot(c), s) = d_gray[s] ? rgbd_args(d_gray[s], gray_pitch_bytes[s], d_depth[s], depth_pitch_bytes[s], depth_format, depth_scale) : absent_args();
        enqueue_frame(c);
        return 0;
    } catch (...) {
    }
    return -1;
}

LVT_API void lvt_track_with_external_corners(lvt_handle h, unsigned char *left, unsigned char *right, int n_rows, int n_cols,
                                             double corners_left[][2], int n_corners_left, double corners_right[][2],
                                             int n_corners_right, double R[3][3], double t[3]) {
    h = resolve_handle(h);
    if (!is_ctx(h) && !is_slot(h)) return;
    try {
        if (n_corners_left < 0 || n_corners_right < 0) return;
        char cut[160] = "";
        if (n_corners_left > EXT_MAX || n_corners_right > EXT_MAX)  // (the reference takes any number; here the lists are cut -- never silently)
            std::snprintf(cut, sizeof(cut), "lvt_track_with_external_corners: %d / %d corners, only the first %d of a list are used", n_corners_left,
                          n_corners_right, EXT_MAX);
        const int ncl = std::min(n_corners_left, EXT_MAX), ncr = std::min(n_corners_right, EXT_MAX);
        std::vector<float> cl(2 * (size_t)ncl + 2), cr(2 * (size_t)ncr + 2);
        for (int i = 0; i < ncl; i++) {  // doubles narrowed to float (lvt_c.cpp:104-117)
            cl[2 * i] = (float)corners_left[i][0];
            cl[2 * i + 1] = (float)corners_left[i][1];
        }
        for (int i = 0; i < ncr; i++) {
            cr[2 * i] = (float)corners_right[i][0];
            cr[2 * i + 1] = (float)corners_right[i][1];
        }
        if (is_slot(h)) {  // a pooled handle: the lists are deposited with the frame and ride its lock-step step (lvt_pool.h)
            PoolSlot *S = static_cast<PoolSlot *>(h);
            slot_drain(S);
            const float *const lists[2] = {cl.data(), cr.data()};
            const int counts[2] = {ncl, ncr};
            if (slot_submit(S, left, right, n_rows, n_cols, 0, true, lists, counts) != 0) return;
            if (cut[0]) {
                std::lock_guard<std::mutex> g(S->pool->mu);
                S->err = cut;
            }
            (void)slot_collect(S);
            slot_result(S, R, t);
            return;
        }
        Context *c = frame_context(h, "lvt_track_with_external_corners", 1, true);
        if (!c) return;
        DeviceGuard guard(c);
        if (c->has_rect(0)) {  // the images would be raw, the corners in rectified coordinates the caller does not have
            refuse(h, "lvt_track_with_external_corners", "refused on a handle with rectifiers attached (the frame was NOT tracked; detach them with lvt_amd_set_rectifiers(h, NULL, NULL))");
            return;
        }
        if (c->has_reduce(0)) {  // likewise: the corners would be in the large frame's coordinates, or the reduced image's -- the call cannot know
            refuse(h, "lvt_track_with_external_corners", "refused on a handle with a reduction in force (the frame was NOT tracked; clear it with lvt_amd_set_reduction, factor 1)");
            return;
        }
        if (cut[0]) c->set_error(cut);
        upload_and_track(c, left, right, false, n_rows, n_cols, cl.data(), ncl, cr.data(), ncr, R, t);
    } catch (...) {
    }
}

LVT_API int lvt_get_status(lvt_handle h) {
    h = resolve_handle(h);
    try {
        if (is_slot(h)) {
            PoolSlot *S = static_cast<PoolSlot *>(h);
            slot_drain(S);
            return S->last.rec.state;
        }
        Context *c = frame_context(h, "lvt_get_status", 0, true);
        if (!c) return -1;
        DeviceGuard guard(c);
        drain(c);
        return last_ctl(c).state;
    } catch (...) {
    }
    return -1;
}

// ---- introspection (of the most recently COLLECTED frame; drains the pipeline first) -----------------
LVT_API void lvt_amd_get_counts(lvt_handle h, int out[LVT_AMD_C__COUNT]) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return;
        for (int i = 0; i < LVT_AMD_C__COUNT; i++) out[i] = v.rec->counts[i];
    } catch (...) {
    }
}

LVT_API int lvt_amd_get_features(lvt_handle h, int eye, float *xy, float *resp, uint8_t *desc, int cap) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return -1;
        Context *c = v.c;
        const Feat &F = c->h_seqs[v.s].fb[v.par].feat[eye ? 1 : 0];
        const int n = read_scalar(c, F.n), m = std::min(n, cap);
        std::vector<float> x(m), y(m);
        d2h(c, x.data(), F.x, m);
        d2h(c, y.data(), F.y, m);
        if (xy)
            for (int i = 0; i < m; i++) xy[2 * i] = x[i], xy[2 * i + 1] = y[i];
        d2h(c, resp, F.resp, m);
        d2h(c, desc, reinterpret_cast<const uint8_t *>(F.desc), (size_t)m * 32);
        return n;
    } catch (...) {
    }
    return -1;
}

LVT_API int lvt_amd_get_matches(lvt_handle h, int *feat_idx, double *xyz, int cap) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return -1;
        Context *c = v.c;
        const int n = v.rec->n_matches, m = std::min(n, cap);
        d2h(c, feat_idx, c->h_seqs[v.s].pnp_feat, m);
        d2h(c, xyz, c->h_seqs[v.s].pnp_X, (size_t)m * 3);
        return n;
    } catch (...) {
    }
    return -1;
}

LVT_API int lvt_amd_get_row_matches(lvt_handle h, int *pairs, int cap) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return -1;
        Context *c = v.c;
        const int n = v.rec->counts[C_N_ROW_MATCHES], m = std::min(n, cap);
        std::vector<int> l(m), r(m);
        d2h(c, l.data(), c->h_seqs[v.s].pair_l, m);
        d2h(c, r.data(), c->h_seqs[v.s].pair_r, m);
        for (int i = 0; i < m; i++) pairs[2 * i] = l[i], pairs[2 * i + 1] = r[i];
        return n;
    } catch (...) {
    }
    return -1;
}

static int get_points(Context *c, const MapSoA *bufs, const int *d_cur, const int *d_n, double *xyz, int *counter, int *age, uint8_t *desc,
                      int cap) {
    const int cur = read_scalar(c, d_cur), n = read_scalar(c, d_n), m = std::min(n, cap);
    const MapSoA &P = bufs[cur];
    d2h(c, xyz, P.pos, (size_t)m * 3);
    d2h(c, counter, P.counter, m);
    d2h(c, age, P.age, m);
    d2h(c, desc, reinterpret_cast<const uint8_t *>(P.desc), (size_t)m * 32);
    return n;
}
LVT_API int lvt_amd_get_map(lvt_handle h, double *xyz, int *counter, int *age, uint8_t *desc, int cap) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return -1;
        Context *c = v.c;
        const Seq &S = c->h_seqs[v.s];
        return get_points(c, S.map, S.map_cur, S.map_n, xyz, counter, age, desc, cap);
    } catch (...) {
    }
    return -1;
}
LVT_API int lvt_amd_get_staged(lvt_handle h, double *xyz, int *counter, uint8_t *desc, int cap) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return -1;
        Context *c = v.c;
        const Seq &S = c->h_seqs[v.s];
        return get_points(c, S.staged, S.staged_cur, S.staged_n, xyz, counter, nullptr, desc, cap);
    } catch (...) {
    }
    return -1;
}
// The candidate lists of the last frame as their builders left them (tests/test_gpu_candidate_lists.py holds them to a reference, list by list): only the
// builders store to Seq::cand / ncand, scand / sncand and rcand / rncand (candidates_body and k_hamming_batched_lists), and proj / vis, sproj / svis are written
// by the projections in front of them, so all of it is final once the frame is collected.  Host only: copies, no launch.  The early stream may still be running
// behind a collected frame (a k_triangulate that built its row lists itself does not wait for the early stream's), so every stream of the handle is
// synchronised first.  A single-sequence handle only (a batch's lists are the same kernels fetching their Seq differently).
LVT_API int lvt_amd_get_candidate_lists(lvt_handle h, int which, unsigned *keys, int *counts, float *proj, signed char *vis, int cap, lvt_amd_list_info *info) {
    h = resolve_handle(h);
    if (!is_ctx(h) || which < LVT_AMD_LISTS_MAP || which > LVT_AMD_LISTS_ROW) return -1;
    Context *c = static_cast<Context *>(h);
    if (c->B != 1) return -1;
    DeviceGuard guard(c);
    try {
        drain(c);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream_f));
        HIPCHK(c, hipStreamSynchronize(c->stream_e));
        const Seq &S = c->h_seqs[0];
        const Ctl &rec = last_ctl(c);
        const int par = c->last_par;
        int fbw[LFB_WORDS] = {0, 0, 0, 0};
        d2h(c, fbw, S.lists_fb, (size_t)LFB_WORDS);
        // what the frame built: nothing before the first frame is collected; map lists on a frame that tracked against a map; staged lists behind a pose, where points
        // are staged at all; row lists on every stereo frame whose features the frame kept (a LOST frame's epilogue hides them: its count is 0)
        const bool tracked = c->done > 0 && rec.active && !rec.first_frame;
        int n = 0;
        if (which == LVT_AMD_LISTS_MAP && tracked) n = rec.counts[C_MAP_SIZE_AT_MATCH];
        if (which == LVT_AMD_LISTS_STAGED && tracked && !rec.lost_now && S.prm.staged_th > 0) n = fbw[LFB_STAGED_N];
        if (which == LVT_AMD_LISTS_ROW && c->done > 0 && c->sensor == 1) n = rec.counts[C_N_LEFT];
        const int lim = which == LVT_AMD_LISTS_MAP ? MAP_MAX : which == LVT_AMD_LISTS_STAGED ? STAGED_MAX : NF_MAX;
        n = std::min(std::max(n, 0), lim);
        if (info) {
            info->kc = KC;
            info->stood_down_map = fbw[LFB_MAP], info->stood_down_row = fbw[LFB_ROW];
            info->pass2 = tracked ? rec.do_pass2 : 0;
            info->n_early = tracked ? fbw[LFB_EARLY_N] : 0;
            info->binned = c->binned_lists ? 1 : 0;
            info->n = n;
            info->reserved = 0;
        }
        if (n > cap) return -1;
        const uint32_t *dk = which == LVT_AMD_LISTS_MAP ? S.cand : which == LVT_AMD_LISTS_STAGED ? S.scand : S.rcand + (size_t)par * NF_MAX * KC;
        const int *dn = which == LVT_AMD_LISTS_MAP ? S.ncand : which == LVT_AMD_LISTS_STAGED ? S.sncand : S.rncand + (size_t)par * NF_MAX;
        d2h(c, keys, dk, (size_t)n * KC);
        d2h(c, counts, dn, (size_t)n);
        if (which != LVT_AMD_LISTS_ROW) {
            d2h(c, proj, which == LVT_AMD_LISTS_MAP ? S.proj : S.sproj, (size_t)n * 2);
            d2h(c, reinterpret_cast<int8_t *>(vis), which == LVT_AMD_LISTS_MAP ? S.vis : S.svis, (size_t)n);
        }
        return n;
    } catch (...) {
    }
    return -1;
}
// pose + state of the frame the last tracking call returned, WITHOUT waiting for that frame's tail: a synchronous call that returned on
// the pose k_pnp handed over reads it from the same pinned record (quaternion as the tracker holds it, not re-derived from R)
LVT_API int lvt_amd_get_last_pose(lvt_handle h, double q[4], double p[3]) {
    h = resolve_handle(h);
    if (is_slot(h)) {
        try {
            View v;
            if (!view_of(h, v)) return -1;
            for (int k = 0; k < 4; k++) q[k] = v.rec->last_pose.q[k];
            for (int k = 0; k < 3; k++) p[k] = v.rec->last_pose.p[k];
            return v.rec->state;
        } catch (...) {
        }
        return -1;
    }
    Context *c = static_cast<Context *>(h);
    if (!c) return -1;
    if (c->early_pending && c->enq > 0) {
        const PoseRec &r = c->h_pose[(size_t)((c->enq - 1) % RING) * c->B];
        for (int k = 0; k < 4; k++) q[k] = r.q[k];
        for (int k = 0; k < 3; k++) p[k] = r.p[k];
        return r.status;
    }
    DeviceGuard guard(c);
    try {
        drain(c);
        for (int k = 0; k < 4; k++) q[k] = last_ctl(c).last_pose.q[k];
        for (int k = 0; k < 3; k++) p[k] = last_ctl(c).last_pose.p[k];
        return last_ctl(c).state;
    } catch (...) {
    }
    return -1;
}
LVT_API void lvt_amd_get_pose(lvt_handle h, double q[4], double p[3]) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return;
        for (int k = 0; k < 4; k++) q[k] = v.rec->last_pose.q[k];
        for (int k = 0; k < 3; k++) p[k] = v.rec->last_pose.p[k];
    } catch (...) {
    }
}
LVT_API void lvt_amd_get_predicted_pose(lvt_handle h, double q[4], double p[3]) {
    h = resolve_handle(h);
    try {
        View v;
        if (!view_of(h, v)) return;
        for (int k = 0; k < 4; k++) q[k] = v.rec->predicted.q[k];
        for (int k = 0; k < 3; k++) p[k] = v.rec->predicted.p[k];
    } catch (...) {
    }
}
LVT_API void lvt_amd_get_debug(lvt_handle h, long long out[32]) {
    h = resolve_handle(h);
    if (!is_ctx(h)) return;
    Context *c = static_cast<Context *>(h);
    DeviceGuard guard(c);
    try {
        drain(c);
        for (int i = 0; i < 32; i++) out[i] = last_ctl(c).dbg[i];
    } catch (...) {
    }
}
LVT_API int lvt_amd_get_ordering(lvt_handle h) {  // 0: polling gates + early stream, 1: event barriers only, 2: a pooled handle (a seat of the device's shared lock-step chain)
    if (is_auto(h)) {  // (under the record's lock, see lvt_amd_last_error)
        AutoHandle *A = static_cast<AutoHandle *>(h);
        std::lock_guard<std::mutex> g(A->mu);
        return lvt_amd_get_ordering(A->impl);
    }
    if (is_slot(h)) return 2;
    return h && static_cast<Context *>(h)->events_only ? 1 : 0;
}
LVT_API void lvt_amd_get_timeline(lvt_handle h, long long out[16]) {  // of the frame collected last; a frame whose synchronous call
    h = resolve_handle(h);
    if (!is_ctx(h)) return;
    Context *c = static_cast<Context *>(h);                            // returned on its pose is collected first, nothing else is drained
    DeviceGuard guard(c);
    try {
        if (c->early_pending) drain(c);
    } catch (...) {
    }
    for (int i = 0; i < 16; i++) out[i] = last_ctl(c).dbg[32 + i];
}
LVT_API int lvt_amd_get_plane(lvt_handle h, int eye, int what, void *dst, int cap_bytes, int *pitch_out) {
    h = resolve_handle(h);
    if (!is_ctx(h)) return -1;
    Context *c = static_cast<Context *>(h);
    DeviceGuard guard(c);
    try {
        drain(c);
        const FrameBuf &FB = c->h_seqs[0].fb[c->last_par];
        const size_t n = (size_t)c->pitch * c->prm.H;
        const int e = eye ? 1 : 0;
        const void *src = (what == 0) ? (const void *)FB.score[e] : (const void *)FB.boxsum[e];
        size_t esz = (what == 0) ? 1 : 2;
        if (what == 5 || what == 6) {  // the equalised image of the last frame (u8, rows x pitch) / the tables it was made with (tiles_x * tiles_y x 256 bytes)
            if (c->done == 0 || !c->has_equal(0) || !c->ring_equalised[c->last_slot]) return 0;
            const int ee = c->sensor == 1 ? e : 0;
            const size_t bytes = what == 5 ? n : (size_t)c->equal[0].tiles_x * c->equal[0].tiles_y * 256;
            if ((size_t)cap_bytes < bytes) return -1;
            HIPCHK(c, hipMemcpy(dst, what == 5 ? c->d_eq[(size_t)c->last_par * 2 + ee] : c->d_eq_lut[(size_t)ee], bytes, hipMemcpyDeviceToHost));
            if (pitch_out) *pitch_out = what == 5 ? c->pitch : 256;
            return (int)bytes;
        }
        if (what == 7) {  // the eye's mask as the tracker holds it (u8, rows x pitch, the padding columns zero); 0 bytes without one.  A property: needs no frame
            if (!c->has_mask(0, e)) return 0;
            if ((size_t)cap_bytes < n) return -1;
            HIPCHK(c, hipMemcpy(dst, c->d_mask[(size_t)e], n, hipMemcpyDeviceToHost));
            if (pitch_out) *pitch_out = c->pitch;
            return (int)n;
        }
        if (what == 8) {  // the plane k_label_mask built for the eye of the last frame (u8, rows x pitch, the padding columns zero); 0 bytes where none was built
            if (c->done == 0 || !c->built_label(c->last_slot, 0, e)) return 0;
            if ((size_t)cap_bytes < n) return -1;
            HIPCHK(c, hipMemcpy(dst, c->d_lmask[(size_t)c->last_par * 2 + e], n, hipMemcpyDeviceToHost));
            if (pitch_out) *pitch_out = c->pitch;
            return (int)n;
        }
        if (what == 9) {  // the reduced image of the last (large) frame, ahead of the remap (u8, the BASE size: base_H rows x base_pitch); 0 bytes without a reduction
            if (c->done == 0 || !c->has_reduce(0) || !c->ring_reduced[c->last_slot]) return 0;
            const size_t bytes = (size_t)c->base_pitch(0) * c->base_H(0);
            if ((size_t)cap_bytes < bytes) return -1;
            HIPCHK(c, hipMemcpy(dst, c->d_red[(size_t)c->last_par * 2 + (c->sensor == 1 ? e : 0)], bytes, hipMemcpyDeviceToHost));
            if (pitch_out) *pitch_out = c->base_pitch(0);
            return (int)bytes;
        }
        if (what >= 2 && what <= 4) {  // a frame property's plane: 0 bytes unless the last frame went through that stage
            if (c->done == 0) return 0;
            if (what == 2) {  // the rectified image of the last (raw) frame
                if (!c->has_rect(0)) return 0;
                src = c->d_rect[(size_t)c->last_par * 2 + e], esz = 1;
            } else if (what == 3) {  // the converted gray image of the last (colour) frame, before rectification
                if (!c->converts(0) || !c->ring_converted[c->last_slot]) return 0;
                src = c->d_gray[(size_t)c->last_par * 2 + (c->sensor == 1 ? e : 0)], esz = 1;
                if (c->resized(0)) {  // (converted BEFORE the remap: the raw frame's size, its own pitch)
                    const size_t gbytes = (size_t)c->frame_pitch(0) * c->frame_H(0);
                    if ((size_t)cap_bytes < gbytes) return -1;
                    HIPCHK(c, hipMemcpy(dst, src, gbytes, hipMemcpyDeviceToHost));
                    if (pitch_out) *pitch_out = c->frame_pitch(0);
                    return (int)gbytes;
                }
            } else {  // the registered depth plane of the last frame (fp32, pitch words per row)
                if (!c->has_depth_cam(0) || !c->ring_registered[c->last_slot]) return 0;
                src = c->d_reg[(size_t)c->last_par], esz = sizeof(float);
            }
        }
        const size_t bytes = n * esz;
        if ((size_t)cap_bytes < bytes) return -1;
        HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        if (pitch_out) *pitch_out = c->pitch;
        return (int)bytes;
    } catch (...) {
    }
    return -1;
}

// (the stage entries -- lvt_amd_pnp*, lvt_amd_motion_predict, lvt_amd_hamming_match_batched*, lvt_amd_pose_info_eval, lvt_amd_reloc_match_device / _solve /
// _correspond: lvt_stage_entries.h)

// ---- EuRoC pre-step: rectification -------------------------------------------------------------------------------------
// iR = (Pnew * R)^-1: 3x3 product in k-ascending order, closed-form inverse (cv::gemm / cv::invert for 3x3 doubles)
static void inverse_PR(const double Pnew[9], const double R[9], double out[9]) {
    double AR[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += Pnew[3 * i + k] * R[3 * k + j];
            AR[3 * i + j] = s;
        }
    const double *S = AR;
    double ir[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double d = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (d != 0.) {
        d = 1. / d;
        ir[0] = (S[4] * S[8] - S[5] * S[7]) * d, ir[1] = (S[2] * S[7] - S[1] * S[8]) * d, ir[2] = (S[1] * S[5] - S[2] * S[4]) * d;
        ir[3] = (S[5] * S[6] - S[3] * S[8]) * d, ir[4] = (S[0] * S[8] - S[2] * S[6]) * d, ir[5] = (S[2] * S[3] - S[0] * S[5]) * d;
        ir[6] = (S[3] * S[7] - S[4] * S[6]) * d, ir[7] = (S[1] * S[6] - S[0] * S[7]) * d, ir[8] = (S[0] * S[4] - S[1] * S[3]) * d;
    }
    for (int k = 0; k < 9; k++) out[k] = ir[k];
}
// a rectifier of a sw x sh source and a dw x dh destination with everything allocated and no map built yet; nullptr: no device, or no memory
static Rectifier *rectifier_alloc(int sw, int sh, int dw, int dh) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return nullptr;  // no CPU fallback
    Rectifier *r = new (std::nothrow) Rectifier;
    if (!r) return nullptr;
    r->w = dw, r->h = dh, r->pitch = ((dw + 63) / 64) * 64, r->sw = sw, r->sh = sh;
    const size_t n = (size_t)dw * dh;
    if (hipGetDevice(&r->device) != hipSuccess || hipMalloc((void **)&r->d_fix, n * sizeof(int2)) != hipSuccess ||
        hipMalloc((void **)&r->d_map1, n * 4) != hipSuccess || hipMalloc((void **)&r->d_map2, n * 4) != hipSuccess ||
        hipMalloc((void **)&r->d_src, (size_t)sw * sh) != hipSuccess || hipMalloc((void **)&r->d_dst, (size_t)r->pitch * dh) != hipSuccess) {
        lvt_amd_rectifier_destroy(r);
        return nullptr;
    }
    return r;
}

LVT_API lvt_amd_rectifier lvt_amd_rectifier_create(const double K[9], const double D[5], const double R[9], const double Pnew[9], int width,
                                                   int height) {
    if (!K || !D || !R || !Pnew || width <= 0 || height <= 0) return nullptr;
    Rectifier *r = rectifier_alloc(width, height, width, height);
    if (!r) return nullptr;
    const size_t n = (size_t)width * height;
    r->lens.model = LVT_AMD_LENS_RADTAN, r->lens.width = width, r->lens.height = height;
    for (int k = 0; k < 9; k++) r->lens.K[k] = K[k];
    for (int k = 0; k < 5; k++) r->lens.D[k] = D[k];
    RectifyArgs a;
    inverse_PR(Pnew, R, a.ir);
    a.fx = K[0], a.fy = K[4], a.u0 = K[2], a.v0 = K[5];
    a.k1 = D[0], a.k2 = D[1], a.p1 = D[2], a.p2 = D[3], a.k3 = D[4];
    a.w = width, a.h = height;
    hipLaunchKernelGGL(k_rectify_map, dim3((height + 63) / 64), dim3(64), 0, 0, a, r->d_map1, r->d_map2);
    hipLaunchKernelGGL(k_rectify_fix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, r->d_map1, r->d_map2, r->d_fix, n);
    if (hipDeviceSynchronize() != hipSuccess) {
        lvt_amd_rectifier_destroy(r);
        return nullptr;
    }
    return r;
}

// "" when the arguments pass; the checks in the contract's order ("LENS MODELS", include/lvt_amd_ext.h)
static std::string lens_check(const lvt_amd_lens *lens, const double R[9], const double Pnew[9], int dw, int dh) {
    if (!lens || !R || !Pnew) return "NULL argument";
    if (lens->model != LVT_AMD_LENS_RADTAN && lens->model != LVT_AMD_LENS_FISHEYE) return "unknown lens model " + std::to_string(lens->model);
    if (lens->width < 1 || lens->width > 8192 || lens->height < 1 || lens->height > 8192)
        return "a source of " + std::to_string(lens->width) + " x " + std::to_string(lens->height) + " pixels (1 ... 8192 each way)";
    if (dw < 1 || dw > 8192 || dh < 1 || dh > 8192) return "a destination of " + std::to_string(dw) + " x " + std::to_string(dh) + " pixels (1 ... 8192 each way)";
    bool finite = true;
    for (double v : lens->K) finite = finite && std::isfinite(v);
    for (int k = 0; k < (lens->model == LVT_AMD_LENS_FISHEYE ? 4 : 12); k++) finite = finite && std::isfinite(lens->D[k]);  // (FISHEYE: D[4 ...] is not read)
    if (!finite) return "a lens with a non-finite field of K or D";
    for (int k = 0; k < 9; k++) finite = finite && std::isfinite(R[k]) && std::isfinite(Pnew[k]);
    if (!finite) return "a non-finite field of R or Pnew";
    return "";
}
LVT_API lvt_amd_rectifier lvt_amd_rectifier_create_lens(const lvt_amd_lens *lens, const double R[9], const double Pnew[9], int dst_width, int dst_height) {
    static const char *who = "lvt_amd_rectifier_create_lens";
    const std::string why = lens_check(lens, R, Pnew, dst_width, dst_height);
    if (!why.empty()) {
        refuse_call(who, why + " (nothing was created)");
        return nullptr;
    }
    Rectifier *r = rectifier_alloc(lens->width, lens->height, dst_width, dst_height);
    if (!r) {
        refuse_call(who, "no HIP device, or no memory for the maps (nothing was created)");
        return nullptr;
    }
    r->lens = *lens;
    if (lens->model == LVT_AMD_LENS_FISHEYE)
        for (int k = 4; k < 12; k++) r->lens.D[k] = 0;  // (ignored: the record reads back as what was used)
    LensArgs a;
    inverse_PR(Pnew, R, a.ir);
    a.fx = lens->K[0], a.fy = lens->K[4], a.u0 = lens->K[2], a.v0 = lens->K[5];
    for (int k = 0; k < 12; k++) a.d[k] = r->lens.D[k];
    a.w = dst_width, a.h = dst_height;
    const size_t n = (size_t)dst_width * dst_height;
    if (lens->model == LVT_AMD_LENS_FISHEYE) hipLaunchKernelGGL(k_rectify_map_fisheye, dim3((dst_height + 63) / 64), dim3(64), 0, 0, a, r->d_map1, r->d_map2);
    else hipLaunchKernelGGL(k_rectify_map_radtan, dim3((dst_height + 63) / 64), dim3(64), 0, 0, a, r->d_map1, r->d_map2);
    hipLaunchKernelGGL(k_rectify_fix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, r->d_map1, r->d_map2, r->d_fix, n);
    if (hipDeviceSynchronize() != hipSuccess) {
        lvt_amd_rectifier_destroy(r);
        refuse_call(who, "building the maps failed on the device (nothing was created)");
        return nullptr;
    }
    return r;
}
LVT_API int lvt_amd_rectifier_get_info(lvt_amd_rectifier h, lvt_amd_lens *lens_out, int dst_size[2]) {
    Rectifier *r = static_cast<Rectifier *>(h);
    if (!r || !lens_out || !dst_size) return -1;
    *lens_out = r->lens;
    dst_size[0] = r->w, dst_size[1] = r->h;
    return 0;
}

LVT_API void lvt_amd_rectifier_destroy(lvt_amd_rectifier h) {
    Rectifier *r = static_cast<Rectifier *>(h);
    if (!r) return;
    (void)hipFree(r->d_map1), (void)hipFree(r->d_map2), (void)hipFree(r->d_fix), (void)hipFree(r->d_src), (void)hipFree(r->d_dst);
    delete r;
}

LVT_API int lvt_amd_rectify_device(lvt_amd_rectifier h, const void *d_src, int src_pitch, void *d_dst, int dst_pitch, void *hip_stream) {
    Rectifier *r = static_cast<Rectifier *>(h);
    if (!r || !d_src || !d_dst || src_pitch < r->sw || dst_pitch < r->w || (dst_pitch & 3)) return -1;
    hipLaunchKernelGGL(k_rectify, dim3((dst_pitch / 4 + 255) / 256, r->h), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                       static_cast<const uint8_t *>(d_src), r->sw, r->sh, src_pitch, r->d_map1, r->d_map2, r->w, r->h, static_cast<uint8_t *>(d_dst), dst_pitch);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

LVT_API int lvt_amd_rectify(lvt_amd_rectifier h, const unsigned char *src, unsigned char *dst) {
    Rectifier *r = static_cast<Rectifier *>(h);
    if (!r || !src || !dst) return -1;
    const size_t n = (size_t)r->sw * r->sh;  // (the source is the lens's size, tightly packed)
    if (hipMemcpy(r->d_src, src, n, hipMemcpyHostToDevice) != hipSuccess) return -1;
    if (lvt_amd_rectify_device(r, r->d_src, r->sw, r->d_dst, r->pitch, nullptr) != 0) return -1;
    return hipMemcpy2D(dst, (size_t)r->w, r->d_dst, (size_t)r->pitch, (size_t)r->w, (size_t)r->h, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

LVT_API int lvt_amd_rectifier_get_maps(lvt_amd_rectifier h, float *map1, float *map2) {
    Rectifier *r = static_cast<Rectifier *>(h);
    if (!r || !map1 || !map2) return -1;
    const size_t n = (size_t)r->w * r->h * 4;
    return (hipMemcpy(map1, r->d_map1, n, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(map2, r->d_map2, n, hipMemcpyDeviceToHost) == hipSuccess) ? 0 : -1;
}

// (the properties of a handle -- rectifiers, pixel format, depth camera, pose info -- and their entry points: lvt_frame_props.h)
// host only: the rotation part moved from camera axes to fixed world axes, M cov M^T with M = blockdiag(I, R)
LVT_API void lvt_amd_pose_info_to_ros(const double cov[36], const double R[3][3], double cov_ros[36]) {
    if (!cov || !R || !cov_ros) return;
    double M[36] = {};
    for (int i = 0; i < 3; i++) {
        M[6 * i + i] = 1.0;
        for (int j = 0; j < 3; j++) M[6 * (3 + i) + 3 + j] = R[i][j];
    }
    sandwich6(M, cov, cov_ros);
}

// ---- relocalisation: the defaults and the slice length (the stages alone on caller data, and what they share with a handle's call: lvt_stage_entries.h) ----
LVT_API void lvt_amd_reloc_default_config(lvt_amd_reloc_config *cfg) {
    if (!cfg) return;
    *cfg = lvt_amd_reloc_config{};
    cfg->n_hypotheses = 256, cfg->gate_px2 = 16.0f, cfg->min_disparity = 1.0f, cfg->min_inliers = 30, cfg->seed = 0, cfg->dry_run = 0;
}
LVT_API int lvt_amd_reloc_slice_length(int n_map) { return reloc_slice_length(std::max(n_map, 0)); }

// ---- snapshots: one sequence's state saved, restored, moved between handles and seats (k_state.hip) -------------------------------------------
// Everything is checked before anything changes: a refusal returns -1 / NULL, leaves handle and snapshot as they were and says why in lvt_amd_last_error
// (lvt_amd_snapshot_import / _describe have no handle: lvt_amd_last_error(NULL) then speaks of the calling thread's last refused import or describe).
}  // extern "C"
namespace lvt {
constexpr uint64_t SNAPOBJ_MAGIC = 0x4C56545F534E4150ull;
struct Snapshot {
    uint64_t magic = SNAPOBJ_MAGIC;
    int device = 0;
    uint8_t *d_blob = nullptr;  // SnapHeader::total bytes
    SnapHeader hdr{};           // host copy of the blob's header
    Ctl ctl;                    // host copy of its Ctl section (chain words zero), fetched when first needed
    bool have_ctl = false;
};
struct DevScope {  // DeviceGuard for an object that is no Context
    int prev = -1;
    explicit DevScope(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DevScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
static Snapshot *snap_of(lvt_amd_snapshot s) {
    Snapshot *p = static_cast<Snapshot *>(s);
    return (p && p->magic == SNAPOBJ_MAGIC) ? p : nullptr;
}
static void snap_free(Snapshot *p) {
    if (!p) return;
    if (p->d_blob) {
        DevScope g(p->device);
        (void)hipFree(p->d_blob);
    }
    p->magic = 0;
    delete p;
}
static bool snap_fetch_ctl(Snapshot *p) {
    if (p->have_ctl) return true;
    DevScope g(p->device);
    if (hipMemcpy(&p->ctl, p->d_blob + p->hdr.off[SEC_CTL], sizeof(Ctl), hipMemcpyDeviceToHost) != hipSuccess) return false;
    return p->have_ctl = true;
}
// a header (and, with_payload, the n bytes it heads) this library can take; "" or the reason
static std::string snap_validate(const void *bytes, long long n, bool with_payload) {
    if (!bytes || n < (long long)sizeof(SnapHeader)) return "too short for a snapshot header (" + std::to_string(bytes ? n : 0) + " bytes)";
    SnapHeader h;
    std::memcpy(&h, bytes, sizeof(h));
    if (h.magic != SNAP_MAGIC) return "not a snapshot (wrong magic)";
    if (h.version != SNAP_VERSION) return "snapshot version " + std::to_string(h.version) + ", this library reads version " + std::to_string(SNAP_VERSION);
    if (h.header_bytes != (int)sizeof(SnapHeader) || h.ctl_bytes != (int)sizeof(Ctl))
        return "a snapshot of another build (header / Ctl of " + std::to_string(h.header_bytes) + " / " + std::to_string(h.ctl_bytes) + " bytes, here " +
               std::to_string(sizeof(SnapHeader)) + " / " + std::to_string(sizeof(Ctl)) + ")";
    if (h.nf_max != NF_MAX || h.map_max != MAP_MAX || h.staged_max != STAGED_MAX) return "a snapshot of a build with other capacities";
    if (h.sensor != 1 && h.sensor != 2) return "unknown sensor type " + std::to_string(h.sensor);
    if (h.map_n < 0 || h.map_n > MAP_MAX || h.staged_n < 0 || h.staged_n > STAGED_MAX || (h.map_cur & ~1) || (h.staged_cur & ~1)) return "point counts out of range";
    int off[SNAP_SECTIONS];
    const long long total = snap_layout(h.map_n, h.staged_n, off);
    if (std::memcmp(off, h.off, sizeof(off)) != 0 || h.total != total) return "section offsets that do not belong to its point counts";
    if (!with_payload) return "";
    if (n < total) return "truncated: " + std::to_string(n) + " bytes of " + std::to_string(total);
    if (snap_checksum(static_cast<const uint8_t *>(bytes) + sizeof(SnapHeader), (size_t)(total - (long long)sizeof(SnapHeader))) != h.checksum) return "checksum mismatch (damaged payload)";
    return "";
}
static void snap_info(const SnapHeader &h, const Ctl &k, int device, lvt_amd_snapshot_info *out) {
    out->version = h.version, out->sensor_type = h.sensor, out->state = k.state, out->frame_number = k.frame_number;
    out->map_n = h.map_n, out->staged_n = h.staged_n, out->src_map_cur = h.map_cur, out->src_staged_cur = h.staged_cur, out->device = device, out->bytes = h.total;
}

// the context behind a (resolved) handle for a snapshot call; batch_call: the calls that take every sequence / name one of a batch.  nullptr: refused
static Context *snap_context(lvt_handle h, const char *who, bool batch_call) {
    Context *c = frame_context(h, who, 0, true, {"a pooled or automatic seat (its state lives in a chain shared with other handles) (nothing was changed)", nullptr, nullptr});
    if (!c) return nullptr;
    if (batch_call && c->B == 1 && !c->mixed) {
        refuse_unchanged(h, who, "a batch call on a handle that is not a batch");
        return nullptr;
    }
    return c;
}
static bool snap_seq_ok(Context *c, const char *who, int seq) {
    if (seq >= 0 && seq < c->B) return true;
    refuse_unchanged(c, who, "no sequence " + std::to_string(seq) + " in this handle" + (c->B == 1 ? " (seq is 0 for a solo handle)" : ""));
    return false;
}
static StateSeq state_desc(Context *c, int s, uint8_t *blob, const SnapHeader &h) {
    const Seq &S = c->h_seqs[s];
    StateSeq d{};
    d.ctl = c->d_ctl[s];
    for (int k = 0; k < 2; k++) {
        d.map[k] = PointsRef{S.map[k].pos, S.map[k].desc, S.map[k].counter, S.map[k].age};
        d.staged[k] = PointsRef{S.staged[k].pos, S.staged[k].desc, S.staged[k].counter, S.staged[k].age};
    }
    d.map_cur = S.map_cur, d.map_n = S.map_n, d.staged_cur = S.staged_cur, d.staged_n = S.staged_n;
    d.blob = blob;
    std::memcpy(d.off, h.off, sizeof(d.off));
    d.map_n_blob = h.map_n, d.staged_n_blob = h.staged_n, d.map_cur_blob = h.map_cur, d.staged_cur_blob = h.staged_cur;
    uintptr_t bits = (uintptr_t)blob;  // sections move as 16-byte vectors: both ends of every copy lie on 16-byte boundaries
    for (int k = 0; k < 2; k++)
        for (const PointsRef &r : {d.map[k], d.staged[k]}) bits |= (uintptr_t)r.pos | (uintptr_t)r.desc | (uintptr_t)r.counter | (uintptr_t)r.age;
    if (bits & 15) {
        c->set_error("snapshot: a state array that is not 16-byte aligned");
        throw std::runtime_error(c->err);
    }
    return d;
}
// one launch per STATE_PACK sequences on the handle's stream, then the stream is synchronised (profiling: the launches' time between two events)
static void state_launch(Context *c, bool pack, const std::vector<StateSeq> &ds, const ChainWords &cw) {
    const int slot = pack ? 22 : 23;
    if (c->prof) (void)hipEventRecord(c->ev[slot][0], c->stream);
    size_t i0 = 0;  // sequences sent so far
    unsigned work = 0;
    TablePacker pk(&StateTable::s, [&](const StateTable &tab, int n, bool) {
        const dim3 grid(std::min((work + 255u) / 256u, 256u), n);
        if (pack) hipLaunchKernelGGL(k_state_pack, grid, dim3(256), 0, c->stream, tab, c->d_snap_status + 4 * i0);
        else hipLaunchKernelGGL(k_state_unpack, grid, dim3(256), 0, c->stream, tab, chain_arg(cw));
        i0 += (size_t)n, work = 0;
    });
    for (const StateSeq &d : ds) *pk.add(1) = d, work = std::max(work, state_work(d.map_n_blob, d.staged_n_blob));
    pk.flush();
    if (c->prof) (void)hipEventRecord(c->ev[slot][1], c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    float ms = 0;
    if (c->prof && hipEventElapsedTime(&ms, c->ev[slot][0], c->ev[slot][1]) == hipSuccess) c->prof_ms[slot] += ms, c->prof_calls[slot]++;
}
// snapshots of the sequences `seqs` of a drained context: one pack launch (per STATE_PACK sequences) and ONE small read-back for all of them.  The blobs are sized
// from the host's record of the last frame (its map / staged counters); the kernel reports what it found on the device, and the read-back confirms the sizes --
// should they ever differ, the blobs are sized again from the device's figures.
static void take_snapshots(Context *c, const std::vector<int> &seqs, std::vector<Snapshot *> &out) {
    if (!c->d_snap_status) {
        c->d_snap_status = c->dalloc<int>(4 * (size_t)c->B);
        // dalloc clears on the null stream, which the (non-blocking) tracking stream does not wait for: a clear that lands behind the first pack launch
        // would wipe what it reported, and both sizing attempts would fail ("point counts changed")
        HIPCHK(c, hipStreamSynchronize(nullptr));
    }
    const size_t n = seqs.size();
    std::vector<int> found(4 * n, 0);
    out.assign(n, nullptr);
    try {
        for (int attempt = 0; attempt < 2; attempt++) {
            std::vector<StateSeq> ds;
            for (size_t i = 0; i < n; i++) {
                const int s = seqs[i];
                Snapshot *p = out[i] = new Snapshot();
                SnapHeader &h = p->hdr;
                std::memset(&h, 0, sizeof(h));
                h.magic = SNAP_MAGIC, h.version = SNAP_VERSION, h.header_bytes = (int)sizeof(SnapHeader), h.ctl_bytes = (int)sizeof(Ctl);
                h.nf_max = NF_MAX, h.map_max = MAP_MAX, h.staged_max = STAGED_MAX, h.sensor = c->sensor;
                const int mn = attempt ? found[4 * i + 1] : last_ctl(c, s).counts[C_MAP_SIZE], sn = attempt ? found[4 * i + 3] : last_ctl(c, s).counts[C_STAGED_SIZE];
                h.map_n = std::min(std::max(mn, 0), MAP_MAX), h.staged_n = std::min(std::max(sn, 0), STAGED_MAX);
                h.prm = c->in_prms[c->mixed ? s : 0];
                h.total = snap_layout(h.map_n, h.staged_n, h.off);
                p->device = c->device;
                HIPCHK(c, hipMalloc((void **)&p->d_blob, (size_t)h.total));
                ds.push_back(state_desc(c, s, p->d_blob, h));
            }
            state_launch(c, true, ds, ChainWords{});
            HIPCHK(c, hipMemcpy(found.data(), c->d_snap_status, sizeof(int) * 4 * n, hipMemcpyDeviceToHost));
            bool fits = true;
            for (size_t i = 0; i < n; i++) {
                SnapHeader &h = out[i]->hdr;
                h.map_cur = found[4 * i] & 1, h.staged_cur = found[4 * i + 2] & 1;
                fits = fits && h.map_n == std::min(std::max(found[4 * i + 1], 0), MAP_MAX) && h.staged_n == std::min(std::max(found[4 * i + 3], 0), STAGED_MAX);
            }
            if (fits) break;
            if (attempt) {
                c->set_error("snapshot: the sequence's point counts changed while it was packed");
                throw std::runtime_error(c->err);
            }
            for (Snapshot *&p : out) snap_free(p), p = nullptr;
        }
        for (Snapshot *p : out) HIPCHK(c, hipMemcpy(p->d_blob, &p->hdr, sizeof(SnapHeader), hipMemcpyHostToDevice));
    } catch (...) {
        for (Snapshot *&p : out) snap_free(p), p = nullptr;
        throw;
    }
}
// why snapshot p cannot become sequence s of c; "": it can
static std::string apply_objection(Context *c, int s, const Snapshot *p) {
    if (p->device != c->device)
        return "a snapshot on device " + std::to_string(p->device) + ", the handle owns device " + std::to_string(c->device) + " (between devices: export, then import)";
    if (p->hdr.sensor != c->sensor) return "a snapshot of sensor type " + std::to_string(p->hdr.sensor) + " on a handle of sensor type " + std::to_string(c->sensor);
    if (!same_params(p->hdr.prm, c->in_prms[c->mixed ? s : 0])) return "the snapshot's parameters differ from the sequence's";
    return "";
}
// snaps[i] != nullptr becomes sequence seqs[i]; everything has been checked
static void apply_snapshots(Context *c, const std::vector<int> &seqs, const std::vector<Snapshot *> &snaps) {
    const ChainWords cw = chain_of(fresh_ctl(c));
    std::vector<StateSeq> ds;
    for (size_t i = 0; i < seqs.size(); i++) {
        if (!snap_fetch_ctl(snaps[i])) {
            c->set_error("snapshot: its record could not be read back");
            throw std::runtime_error(c->err);
        }
        ds.push_back(state_desc(c, seqs[i], snaps[i]->d_blob, snaps[i]->hdr));
    }
    state_launch(c, false, ds, cw);
    for (size_t i = 0; i < seqs.size(); i++) {  // the host ring answers from the snapshot at once, as it answers from a fresh record after a reset
        Ctl k = snaps[i]->ctl;
        set_chain(k, cw);
        for (int r = 0; r < RING; r++) c->h_ctl[r * c->B + seqs[i]] = k;
        pose_info_clear(c, seqs[i]);
    }
}
// (h: resolved; the entry points below come through with_auto_handle)
static int snapshot_apply(lvt_handle h, const char *who, bool batch_call, int seq, const lvt_amd_snapshot *list) {
    Context *c = snap_context(h, who, batch_call);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        std::vector<int> seqs;
        std::vector<Snapshot *> snaps;
        if (!batch_call && !snap_seq_ok(c, who, seq)) return -1;
        if (!list) return refuse_unchanged(h, who, "no snapshot");
        for (int i = 0; i < (batch_call ? c->B : 1); i++) {
            const int s = batch_call ? i : seq;
            if (batch_call && !list[i]) continue;  // (left alone)
            Snapshot *p = snap_of(list[i]);
            const std::string tag = c->B > 1 ? "sequence " + std::to_string(s) + ": " : "";
            if (!p) return refuse_unchanged(h, who, tag + "not a snapshot");
            const std::string why = apply_objection(c, s, p);
            if (!why.empty()) return refuse_unchanged(h, who, tag + why);
            seqs.push_back(s), snaps.push_back(p);
        }
        if (frames_in_flight(c)) return refuse_unchanged(h, who, "frames in flight: apply after every frame has been collected");
        if (!seqs.empty()) apply_snapshots(c, seqs, snaps);
        return 0;
    } catch (...) {
    }
    return -1;
}
// ---- relocalisation on a handle (k_reloc.hip; include/lvt_amd_ext.h, "RELOCALISATION") ----------------------------------------------------------------
// Modelled on snapshot_apply: an explicit call between frames on a quiet handle, everything checked before anything changes, all launches on the tracking
// stream, ONE stream synchronisation and one read-back (the call's work record).  The per-frame chain is not touched.
static void reloc_buffers(Context *c) {
    if (c->reloc.work) return;
    RelocBufs &b = c->reloc;
    b.keys = c->dalloc<uint2>((size_t)(MAP_MAX / RELOC_SLICE_MAX) * NF_MAX);
    b.claim = c->dalloc<uint32_t>(MAP_MAX);
    b.corr_feat = c->dalloc<int>(NF_MAX), b.with_pc = c->dalloc<int>(NF_MAX), b.inl = c->dalloc<int>(NF_MAX), b.counts = c->dalloc<int>(RELOC_HYP_MAX);
    b.X = c->dalloc<double>(3 * NF_MAX), b.Pc = c->dalloc<double>(3 * NF_MAX), b.eX = c->dalloc<double>(3 * NF_MAX), b.eErr = c->dalloc<double>(2 * NF_MAX + 2);
    b.uv = c->dalloc<float>(2 * NF_MAX), b.eObs = c->dalloc<float>(2 * NF_MAX);
    b.has_pc = c->dalloc<uint8_t>(NF_MAX), b.eLevel = c->dalloc<int8_t>(NF_MAX);
    HIPCHK(c, hipMemset(b.claim, 0xFF, sizeof(uint32_t) * MAP_MAX));  // RELOC_NO_KEY: every call leaves the table as it found it
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_reloc_refine), hipFuncAttributeMaxDynamicSharedMemorySize, PNP_DYN_BYTES));
    b.work = c->dalloc<RelocWork>(1);
    HIPCHK(c, hipStreamSynchronize(nullptr));  // (the clears run on the NULL stream, which the tracking stream does not wait for)
}
// (h: resolved; the entry points come through with_auto_handle)
static int relocalise(lvt_handle h, const char *who, bool batch_call, int seq, const lvt_amd_reloc_config *cfg_in, lvt_amd_reloc_result *out) {
    Context *c = snap_context(h, who, batch_call);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        if (!batch_call && (c->B != 1 || c->mixed)) return refuse_unchanged(h, who, "a batch handle: lvt_amd_batch_relocalise names the sequence");
        if (!snap_seq_ok(c, who, seq)) return -1;
        if (!out) return refuse_unchanged(h, who, "no record to return the result in");
        lvt_amd_reloc_config cfg;
        lvt_amd_reloc_default_config(&cfg);
        if (cfg_in) cfg = *cfg_in;
        const std::string fault = reloc_config_fault(cfg);
        if (!fault.empty()) return refuse(h, who, fault);
        if (frames_in_flight(c)) return refuse_unchanged(h, who, "frames in flight: relocalise after every frame has been collected");
        if (c->done == 0) return refuse_unchanged(h, who, "the handle has not seen a frame");
        const std::string tag = c->B > 1 ? "sequence " + std::to_string(seq) + ": " : "";
        if (last_ctl(c, seq).counts[C_MAP_SIZE] <= 0) return refuse_unchanged(h, who, tag + "an empty map");
        reloc_buffers(c);
        const Seq &S = c->h_seqs[seq];
        const Params &prm = S.prm;
        const FrameBuf &FB = S.fb[c->last_par];
        RelocSeq rs{};
        for (int e = 0; e < 2; e++) rs.x[e] = FB.feat[e].x, rs.y[e] = FB.feat[e].y, rs.desc[e] = FB.feat[e].desc, rs.n_feat[e] = FB.feat[e].n, rs.map_pos[e] = S.map[e].pos;
        rs.depth = FB.feat[0].depth, rs.map_n = S.map_n, rs.map_cur = S.map_cur, rs.fc = FB.fc;
        const RelocBufs &b = c->reloc;
        RelocWork w{};
        w.success = std::max(cfg.min_inliers, prm.min_matches);
        const ChainWords cw = chain_of(fresh_ctl(c));
        const RelocCorr rc{b.X, b.uv, b.Pc, b.with_pc, 0, 0};
        const RelocCam cam{(double)prm.fx, (double)prm.fy, (double)prm.cx, (double)prm.cy};
        hipStream_t st = c->stream;
        HIPCHK(c, hipMemcpyAsync(b.work, &w, sizeof w, hipMemcpyHostToDevice, st));
        reloc_launch_correspond(st, rs, S.map[0].desc, S.map[1].desc, b, prm, cfg.min_disparity);
        hipLaunchKernelGGL(k_reloc_score, dim3((cfg.n_hypotheses + 3) / 4), dim3(RELOC_THREADS), 0, st, rc, (const RelocWork *)b.work, cam, (uint64_t)cfg.seed,
                           (double)cfg.gate_px2, cfg.n_hypotheses, b.counts);
        hipLaunchKernelGGL(k_reloc_select, dim3(1), dim3(RELOC_THREADS), 0, st, rc, cam, (uint64_t)cfg.seed, (double)cfg.gate_px2, cfg.n_hypotheses, (const int *)b.counts,
                           b.work, b.inl, b.eX, b.eObs);
        hipLaunchKernelGGL(k_reloc_refine, dim3(1), dim3(PNP_THREADS), PNP_DYN_BYTES, st, prm, b.work, (const double *)b.eX, (const float *)b.eObs, b.eErr, b.eLevel);
        hipLaunchKernelGGL(k_reloc_commit, dim3(1), dim3(64), 0, st, c->d_ctl[seq], (const RelocWork *)b.work, cw, cfg.dry_run);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&w, b.work, sizeof w, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        if (w.res.status == RELOC_NO_FEATURES) return refuse_unchanged(h, who, tag + "the last frame was skipped, absent or poisoned: it has no features");
        if (w.res.status != 0 && w.res.status != 3) {  // the pose is zero unless the refinement ran
            for (int k = 0; k < 4; k++) w.res.q_wxyz[k] = 0;
            for (int k = 0; k < 3; k++) w.res.p[k] = w.res.t[k] = 0;
            for (int k = 0; k < 9; k++) w.res.R[k / 3][k % 3] = 0;
        }
        *out = w.res;
        if (w.res.status != 0) return 1;
        if (!cfg.dry_run) {  // the host ring answers from the new state at once, as it answers from a snapshot after an apply
            Ctl k = last_ctl(c, seq);
            reloc_commit_ctl(k, w.res, cw);
            for (int r = 0; r < RING; r++) c->h_ctl[r * c->B + seq] = k;
            pose_info_clear(c, seq);
        }
        return 0;
    } catch (...) {
    }
    return -1;
}
}  // namespace lvt
extern "C" {

LVT_API lvt_amd_snapshot lvt_amd_snapshot_take(lvt_handle h, int seq) {
    static const char *who = "lvt_amd_snapshot_take";
    h = resolve_handle(h);
    Context *c = snap_context(h, who, false);
    if (!c) return nullptr;
    DeviceGuard guard(c);
    try {
        if (!snap_seq_ok(c, who, seq)) return nullptr;
        drain(c);
        std::vector<Snapshot *> out;
        take_snapshots(c, {seq}, out);
        return out[0];
    } catch (...) {
    }
    return nullptr;
}
LVT_API int lvt_amd_batch_snapshot_take(lvt_handle h, lvt_amd_snapshot *out) {
    static const char *who = "lvt_amd_batch_snapshot_take";
    h = resolve_handle(h);
    Context *c = snap_context(h, who, true);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        if (!out) return refuse_unchanged(h, who, "no array to return the snapshots in");
        drain(c);
        std::vector<int> seqs(c->B);
        for (int s = 0; s < c->B; s++) seqs[s] = s;
        std::vector<Snapshot *> got;
        take_snapshots(c, seqs, got);
        for (int s = 0; s < c->B; s++) out[s] = got[s];
        return 0;
    } catch (...) {
    }
    return -1;
}
LVT_API int lvt_amd_snapshot_apply(lvt_handle h, int seq, lvt_amd_snapshot s) {
    return with_auto_handle(h, [&](lvt_handle t) { return snapshot_apply(t, "lvt_amd_snapshot_apply", false, seq, &s); });
}
LVT_API int lvt_amd_batch_snapshot_apply(lvt_handle h, const lvt_amd_snapshot *s) {
    return with_auto_handle(h, [&](lvt_handle t) { return snapshot_apply(t, "lvt_amd_batch_snapshot_apply", true, 0, s); });
}
LVT_API int lvt_amd_relocalise(lvt_handle h, const lvt_amd_reloc_config *cfg, lvt_amd_reloc_result *out) {
    return with_auto_handle(h, [&](lvt_handle t) { return relocalise(t, "lvt_amd_relocalise", false, 0, cfg, out); });
}
LVT_API int lvt_amd_batch_relocalise(lvt_handle h, int seq, const lvt_amd_reloc_config *cfg, lvt_amd_reloc_result *out) {
    return with_auto_handle(h, [&](lvt_handle t) { return relocalise(t, "lvt_amd_batch_relocalise", true, seq, cfg, out); });
}
LVT_API int lvt_amd_batch_reset(lvt_handle h, int seq) {
    static const char *who = "lvt_amd_batch_reset";
    h = resolve_handle(h);
    Context *c = snap_context(h, who, true);
    if (!c) return -1;
    DeviceGuard guard(c);
    try {
        if (!snap_seq_ok(c, who, seq)) return -1;
        reset_state(c, seq);  // (drains first)
        return 0;
    } catch (...) {
    }
    return -1;
}
LVT_API int lvt_amd_snapshot_get_info(lvt_amd_snapshot s, lvt_amd_snapshot_info *out) {
    Snapshot *p = snap_of(s);
    if (!p || !out || !snap_fetch_ctl(p)) return -1;
    snap_info(p->hdr, p->ctl, p->device, out);
    return 0;
}
LVT_API int lvt_amd_snapshot_get_params(lvt_amd_snapshot s, lvt_amd_params *out) {
    Snapshot *p = snap_of(s);
    if (!p || !out) return -1;
    *out = p->hdr.prm;
    return 0;
}
LVT_API long long lvt_amd_snapshot_export(lvt_amd_snapshot s, void *host_buf, long long cap) {
    Snapshot *p = snap_of(s);
    if (!p || !host_buf || cap < p->hdr.total) return -1;
    DevScope g(p->device);
    if (hipMemcpy(host_buf, p->d_blob, (size_t)p->hdr.total, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    SnapHeader h;
    std::memcpy(&h, host_buf, sizeof(h));
    h.checksum = p->hdr.checksum = 0;
    if (std::memcmp(&h, &p->hdr, sizeof(h)) != 0 || !snap_validate(&h, sizeof(h), false).empty()) return -1;  // (the blob's header is not the one it was given)
    h.checksum = snap_checksum(static_cast<const uint8_t *>(host_buf) + sizeof(SnapHeader), (size_t)(h.total - (long long)sizeof(SnapHeader)));
    std::memcpy(host_buf, &h, sizeof(h));
    return h.total;
}
LVT_API lvt_amd_snapshot lvt_amd_snapshot_import(const void *bytes, long long n, int device) {
    const std::string why = snap_validate(bytes, n, true);
    if (!why.empty()) return refuse_call("lvt_amd_snapshot_import", why), nullptr;
    int cur = 0;
    if (device < 0 && hipGetDevice(&cur) == hipSuccess) device = cur;
    Snapshot *p = new Snapshot();
    std::memcpy(&p->hdr, bytes, sizeof(SnapHeader));
    std::memcpy(&p->ctl, static_cast<const uint8_t *>(bytes) + p->hdr.off[SEC_CTL], sizeof(Ctl));
    p->have_ctl = true, p->device = device;
    p->hdr.checksum = 0;  // (a blob in device memory carries none: export writes it)
    bool ok;
    {
        DevScope g(device);
        ok = hipMalloc((void **)&p->d_blob, (size_t)p->hdr.total) == hipSuccess && hipMemcpy(p->d_blob, bytes, (size_t)p->hdr.total, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(p->d_blob, &p->hdr, sizeof(SnapHeader), hipMemcpyHostToDevice) == hipSuccess;
    }
    if (!ok) {
        refuse_call("lvt_amd_snapshot_import", hipGetErrorString(hipGetLastError()));
        snap_free(p);
        return nullptr;
    }
    g_call_refusal.clear();
    return p;
}
LVT_API int lvt_amd_snapshot_describe(const void *bytes, long long n, lvt_amd_snapshot_info *out, lvt_amd_params *prm) {  // host code only
    const std::string why = snap_validate(bytes, n, true);
    if (!why.empty()) return refuse_call("lvt_amd_snapshot_describe", why);
    SnapHeader h;
    Ctl k;
    std::memcpy(&h, bytes, sizeof(h));
    std::memcpy(&k, static_cast<const uint8_t *>(bytes) + h.off[SEC_CTL], sizeof(Ctl));
    if (out) snap_info(h, k, -1, out);
    if (prm) *prm = h.prm;
    g_call_refusal.clear();
    return 0;
}
LVT_API void lvt_amd_snapshot_destroy(lvt_amd_snapshot s) { snap_free(snap_of(s)); }

// ---- odometry accumulator (lvt_ros.cpp:215-311 without ROS) -----------------------------------------------
LVT_API lvt_amd_odometry lvt_amd_odometry_create(lvt_handle h, const double base_to_sensor[12], int reset_pose_on_lost) {
    h = resolve_handle(h);
    try {
        Odometry *o = new Odometry();
        o->tracker = h;
        o->reset_pose_on_lost = reset_pose_on_lost != 0;
        if (base_to_sensor)
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) o->base_to_sensor.R[3 * i + j] = base_to_sensor[4 * i + j];
                o->base_to_sensor.p[i] = base_to_sensor[4 * i + 3];
            }
        return o;
    } catch (...) {
        return nullptr;
    }
}
LVT_API void lvt_amd_odometry_destroy(lvt_amd_odometry o) { delete static_cast<Odometry *>(o); }
LVT_API void lvt_amd_odometry_reset(lvt_amd_odometry op) {  // reset_vo (lvt_ros.cpp:184-198)
    Odometry *o = static_cast<Odometry *>(op);
    if (!o) return;
    if (o->tracker) lvt_amd_reset(o->tracker);
    o->restart_deltas();
    o->base_to_odom = Rigid();
}
// cfg NULL: the default config; max_lost_frames <= 0: the policy is off (the reference's reset on every LOST frame).  0 / -1 (a bad config field)
LVT_API int lvt_amd_odometry_set_relocalisation(lvt_amd_odometry op, const lvt_amd_reloc_config *cfg, int max_lost_frames) {
    Odometry *o = static_cast<Odometry *>(op);
    if (!o) return -1;
    lvt_amd_reloc_config c;
    lvt_amd_reloc_default_config(&c);
    if (cfg) c = *cfg;
    std::string fault = reloc_config_fault(c);
    // (a dry run would publish the relocalised pose while the tracker stays LOST, and the failures that lead to the reset would never be counted)
    if (fault.empty() && c.dry_run) fault = "dry_run is 1: the accumulator's relocalisation commits, dry_run must be 0 (nothing was changed)";
    if (!fault.empty()) return refuse_call("lvt_amd_odometry_set_relocalisation", fault);
    o->reloc_cfg = c, o->max_lost_frames = std::max(max_lost_frames, 0), o->lost_run = 0;
    return 0;
}
LVT_API int lvt_amd_odometry_push_pose(lvt_amd_odometry op, const double R[3][3], const double t[3], int status, double stamp_sec,
                                       double pose_out[7], double twist_out[6]) {
    Odometry *o = static_cast<Odometry *>(op);
    if (!o || !R || !t) return -1;
    if (o->have_time && o->last_time > stamp_sec) return 0;  // older than the last published frame: ignored (lvt_ros.cpp:224-229)
    o->pushed_relocalised = false;
    if (status != 3) o->lost_run = 0;
    if (status == 3 && o->max_lost_frames > 0) {  // the relocalisation policy: the map is kept, last_R / last_p stay those of the last tracked frame
        lvt_amd_reloc_result r;
        if (o->tracker && lvt_amd_relocalise(o->tracker, &o->reloc_cfg, &r) == 0) {  // the published delta spans the gap: the trajectory stays continuous
            o->lost_run = 0;
            o->pushed_relocalised = true;
            return o->push(&r.R[0][0], r.t, stamp_sec, pose_out, twist_out) ? 1 : 0;
        }
        if (++o->lost_run < o->max_lost_frames) return 0;  // nothing is published, nothing is reset
        o->lost_run = 0;                                   // ... that many failures in a row: the reference's reset, below
    }
    if (status == 3) {  // LOST: reset the tracker, optionally the accumulated pose; nothing is published (lvt_ros.cpp:241-253)
        if (o->tracker) lvt_amd_reset(o->tracker);
        if (o->reset_pose_on_lost) {
            o->base_to_odom = Rigid();
            o->restart_deltas();
        }
        return 0;
    }
    return o->push(&R[0][0], t, stamp_sec, pose_out, twist_out) ? 1 : 0;
}
LVT_API int lvt_amd_odometry_update(lvt_amd_odometry op, unsigned char *left, unsigned char *right, int n_rows, int n_cols, double stamp_sec,
                                    double pose_out[7], double twist_out[6]) {
    Odometry *o = static_cast<Odometry *>(op);
    if (!o || !o->tracker || !left || !right) return -1;
    if (o->have_time && o->last_time > stamp_sec) return 0;  // (checked before tracking, like the node)
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
    lvt_track(o->tracker, left, right, n_rows, n_cols, R, t);
    return lvt_amd_odometry_push_pose(op, R, t, lvt_get_status(o->tracker), stamp_sec, pose_out, twist_out);
}
// ... with the covariance of the published pose: the perturbation map is taken from the accumulator's state BEFORE the push (lvt_odometry.h), the push itself is
// lvt_amd_odometry_push_pose's
LVT_API int lvt_amd_odometry_push_pose_cov(lvt_amd_odometry op, const double R[3][3], const double t[3], int status, double stamp_sec,
                                           const double cov_in[36], double pose_out[7], double twist_out[6], double cov_out[36]) {
    Odometry *o = static_cast<Odometry *>(op);
    if (cov_out)
        for (int k = 0; k < 36; k++) cov_out[k] = 0.0;
    if (!o || !R || !t) return -1;
    double M[36];
    o->perturbation_map(&R[0][0], M);
    const int rc = lvt_amd_odometry_push_pose(op, R, t, status, stamp_sec, pose_out, twist_out);
    // (a frame the policy relocalised: M and cov_in belong to the LOST frame handed in, not to the pose that was published -- cov_out stays zero)
    if (rc == 1 && cov_in && cov_out && !o->pushed_relocalised) sandwich6(M, cov_in, cov_out);
    return rc;
}
LVT_API int lvt_amd_odometry_update_cov(lvt_amd_odometry op, unsigned char *left, unsigned char *right, int n_rows, int n_cols, double stamp_sec,
                                        double pose_out[7], double twist_out[6], double cov_out[36]) {
    Odometry *o = static_cast<Odometry *>(op);
    if (cov_out)
        for (int k = 0; k < 36; k++) cov_out[k] = 0.0;
    if (!o || !o->tracker || !left || !right) return -1;
    if (o->have_time && o->last_time > stamp_sec) return 0;  // (checked before tracking, like the node)
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
    lvt_track(o->tracker, left, right, n_rows, n_cols, R, t);
    const int status = lvt_get_status(o->tracker);
    lvt_amd_pose_info rec;
    const bool have = lvt_amd_get_pose_info(o->tracker, 0, &rec) == 1 && rec.status == 1;
    return lvt_amd_odometry_push_pose_cov(op, R, t, status, stamp_sec, have ? rec.cov : nullptr, pose_out, twist_out, cov_out);
}

}  // extern "C"
