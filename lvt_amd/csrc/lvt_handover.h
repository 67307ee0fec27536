// lvt_handover.h -- how the feature (F), early (E) and tracking (T) streams of one context and the host hand a frame to each other: 64-bit sequence
// words, polled.  Frame `seq` (1-based: the frame enqueued as number `enq` has seq = enq + 1) is handed over when a word reaches seq.  Every word only grows.
//
// | word                | written by, when                                                   | waited on by                          | limit              | at the limit                                             |
// |---------------------|--------------------------------------------------------------------|---------------------------------------|--------------------|----------------------------------------------------------|
// | FeatCtl::feat_seq   | publish_features: the last workgroup of k_brief / k_brief_img      | k_gate (E), first wait                | GATE_STAND_DOWN    | gate_timeouts++; E stands down, T does all the work      |
// |                     | (single sequence), k_feat_done (batch) -- the buffer's features    | gate_late_poll (T), second wait       | GATE_FATAL         | gate_fatal++, Ctl::skip: the frame is SKIPPED (last      |
// |                     | are complete, or the frame is published without any (skip_seq)     |                                       |                    | pose, state kept, reported; never LOST)                  |
// |                     |                                                                    | seq_reached: k_candidates<ROW>, k_row_done, k_hamming_batched_lists<ROW> leave, nothing is waited for |
// | FeatCtl::poison     | gate_buf_wait at its limit, feat_begin for an absent seat; cleared | every feature kernel reads it at its head and leaves the buffer alone (stream order, no wait)         |
// |                     | by publish_features                                                |                                       |                    |                                                          |
// | FeatCtl::skip_seq   | publish_features, in front of feat_seq, when the frame is poisoned | frame_without_features: k_gate (stands down, not counted), gate_late_poll and the ungated             |
// |                     |                                                                    | k_match_map (Ctl::skip); read behind feat_seq or a stream event, never waited for                     |
// | FeatCtl::row_seq    | k_row_done (E) behind k_candidates<ROW>, if the features were      | k_triangulate (T), thread 0           | ROW_LISTS_FALLBACK | gate_timeouts++, C_ROW_FALLBACK: the workgroup builds    |
// |                     | complete                                                           |                                       |                    | the lists itself (costs time, never the track)           |
// | Ctl::pnp_seq        | k_pnp (T), on both ways out: the pose and early_done are final     | k_gate (E), second wait, for seq - 1  | GATE_STAND_DOWN    | gate_timeouts++; E stands down                           |
// | Ctl::early_state    | early_word(seq, phase): early_claim (k_gate), early_finish         | gate_late_poll (T), first wait, until | GATE_LATE_CANCEL   | gate_timeouts++; unclaimed: early_cancel (a late early   |
// |                     | (k_early_mid), early_cancel (gate_late_poll); fresh_ctl (host)     | early_settled                         |                    | kernel finds it taken); claimed: the clock starts again  |
// | Ctl::gate_ok        | k_gate: seq if its claim holds, else 0 (plain store)               | early_points_claimed: k_early_map, k_early_mid, k_hamming_batched_lists<MAP> (E, stream order)        |
// | Ctl::early_ran_seq  | k_early_mid: it has resolved [0, early_done) (plain store)         | early_points_ran: k_match_map, k_track_mid (T, behind the first wait of gate_late_poll)               |
// | Ctl::track_done_seq | k_triangulate (T), last: the frame's feature buffer is free        | gate_buf_wait (F: k_gate_buf,         | GATE_FATAL         | gate_fatal++, FeatCtl::poison: the feature kernels leave |
// |                     |                                                                    | k_feat_begin_pack), for seq - NPAR    |                    | the buffer alone, the frame is published without features|
// | Ctl::late_gate_seq  | workgroup 0 of a gated k_match_map, behind gate_late_poll          | its other workgroups                  | none               | (wait_seq_unbounded: workgroup 0's waits are bounded)    |
//
// LVT_AMD_ORDERING=events replaces k_gate_buf, k_gate and gate_late_poll by stream events; the publishers stay.  The finished record travels to the host at
// system scope (deliver_record, k_track.hip), the host's own bounded spin is spin_on_flags (lvt_host.hip).
#pragma once
#include "lvt_dev.h"
namespace lvt {
// ---- time: wall_clock64() counts at 100 MHz
constexpr unsigned long long WALL_HZ = 100000000ull;
__host__ __device__ constexpr unsigned long long ticks_ms(unsigned long long n) { return n * (WALL_HZ / 1000); }
constexpr unsigned long long GATE_STAND_DOWN = ticks_ms(20);    // reached when a tool serialises the dispatches of all queues (rocprofv3 --pmc): the gate holds the only slot
constexpr unsigned long long GATE_LATE_CANCEL = ticks_ms(60);   // T gives E up: E's own gate has two waits of GATE_STAND_DOWN
constexpr unsigned long long GATE_FATAL = ticks_ms(2000);       // a stream is wedged (or serialised): nothing valid to work on
constexpr unsigned long long ROW_LISTS_FALLBACK = ticks_ms(5);  // the row lists are normally ~70 us old when k_triangulate asks
constexpr unsigned long long SPLIT_HELPER = ticks_ms(2);        // k_cells' main workgroup takes the whole cell (a wait of its own shape, k_features.hip)
static_assert(GATE_STAND_DOWN == 2000000ull && GATE_LATE_CANCEL == 6000000ull && GATE_FATAL == 200000000ull && ROW_LISTS_FALLBACK == 500000ull && SPLIT_HELPER == 200000ull, "100-MHz ticks");
static_assert(GATE_LATE_CANCEL > 2 * GATE_STAND_DOWN && GATE_FATAL > GATE_LATE_CANCEL, "T cancels the early work only after both waits of k_gate have given up; a frame is skipped long after that");

// ---- Ctl::early_state: who owns frame seq's early work, early_word(seq, phase)
// claimed: E's kernels are running; finished: with results; nothing: E stood down, or T cancelled it (an early kernel that arrives later finds the claim taken) -- the idle value
enum EarlyPhase : unsigned { EARLY_CLAIMED = 1, EARLY_FINISHED = 2, EARLY_NOTHING = 3 };
__host__ __device__ constexpr seq_t early_word(seq_t seq, EarlyPhase ph) { return 4u * seq + ph; }
__host__ __device__ constexpr bool early_claimable(seq_t cur, seq_t seq) { return cur < early_word(seq, EARLY_CLAIMED); }
__host__ __device__ constexpr bool early_settled(seq_t cur, seq_t seq) { return cur >= early_word(seq, EARLY_FINISHED); }
__host__ __device__ constexpr bool early_laws(seq_t s) {  // monotone in (seq, phase); the two predicates agree with each other across seq and seq + 1
    const seq_t c = early_word(s, EARLY_CLAIMED), f = early_word(s, EARLY_FINISHED), n = early_word(s, EARLY_NOTHING), c1 = early_word(s + 1, EARLY_CLAIMED);
    return c < f && f < n && n < c1 && early_claimable(n - 4, s) && !early_settled(n - 4, s) && !early_claimable(c, s) && !early_settled(c, s) &&  // idle: open; claimed: neither
           !early_claimable(f, s) && early_settled(f, s) && !early_claimable(n, s) && early_settled(n, s) &&     // over, either way ...
           early_claimable(f, s + 1) && early_claimable(n, s + 1) && !early_settled(n, s + 1) && early_settled(c1, s);  // ... and seq + 1 is open
}
static_assert(early_laws(1) && early_laws(7) && early_laws(1ull << 61), "early_state");

// ---- waiting and publishing (one thread)
__device__ __forceinline__ seq_t load_seq(const seq_t &word) { return __hip_atomic_load(&word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ bool seq_reached(const seq_t &word, seq_t seq) { return load_seq(word) >= seq; }
// false: `limit` ticks after t0 the word was still below `want`; *seen: the last value loaded
__device__ __forceinline__ bool wait_seq(const seq_t &word, seq_t want, unsigned long long limit, unsigned long long t0 = wall_clock64(), seq_t *seen = nullptr) {
    for (;;) {
        const seq_t cur = load_seq(word);
        if (seen) *seen = cur;
        if (cur >= want) return true;
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > limit) return false;
    }
}
// for the follower workgroups of a gated k_match_map alone.  Ends because workgroup 0, co-resident with them (16 workgroups), publishes the word behind waits that are all bounded.
__device__ __forceinline__ void wait_seq_unbounded(const seq_t &word, seq_t want) { while (load_seq(word) < want) __builtin_amdgcn_s_sleep(8); }
// release: everything written for the waiting stream is final
__device__ __forceinline__ void publish_seq(seq_t &word, seq_t v) { __threadfence(), atomicExch(&word, v); }
__device__ __forceinline__ bool frame_without_features(const FeatCtl &fc, seq_t seq) { return load_seq(fc.skip_seq) == seq; }
// map points [0, n) of frame seq that the early kernels are to handle (0: first frame, LOST, the previous frame did not reach its pose refinement, or the gate stood down) ...
// (a pointer, not a reference: a reference parameter is known dereferenceable, the load of early_done then moves in front of the comparison -- k_track_mid spilled 7 more VGPRs)
__device__ __forceinline__ int early_points_claimed(const Ctl *ctl, seq_t seq) { return (ctl->gate_ok == seq) ? ctl->early_done : 0; }
// ... and that they did handle: the late kernels trust early_done only with k_early_mid's confirmation
__device__ __forceinline__ int early_points_ran(const Ctl *ctl, seq_t seq) { return (ctl->early_ran_seq == seq) ? max(ctl->early_done, 0) : 0; }
// the feature stage's last act for frame seq (one thread, behind every write of the stage)
__device__ __forceinline__ void publish_features(const Seq &S, FeatCtl &fc, seq_t seq) {
    if (fc.poison) fc.skip_seq = seq, fc.poison = 0;  // no features (gate_buf_wait gave up, or an absent seat): say so to the gates of the other streams, then release the flag
    S.ctl->dbg[47] = (long long)wall_clock64();       // (written from the feature stream: the frame it belongs to may differ)
    publish_seq(fc.feat_seq, seq);
}

// ---- the three transitions of early_state
// k_gate: claim the frame (ok) or record that nothing will be done; false: it stands down, also when the tracking stream has cancelled the frame meanwhile
__device__ __forceinline__ bool early_claim(Ctl &ctl, seq_t seq, bool ok) {
    const seq_t mine = early_word(seq, ok ? EARLY_CLAIMED : EARLY_NOTHING);
    seq_t cur = load_seq(ctl.early_state);
    for (;;) {
        if (!early_claimable(cur, seq)) return false;
        const seq_t seen = atomicCAS(&ctl.early_state, cur, mine);
        if (seen == cur) return ok;
        cur = seen;
    }
}
__device__ __forceinline__ void early_finish(Ctl &ctl, seq_t seq) { atomicCAS(&ctl.early_state, early_word(seq, EARLY_CLAIMED), early_word(seq, EARLY_FINISHED)); }
__device__ __forceinline__ bool early_cancel(Ctl &ctl, seq_t cur, seq_t seq) { return early_claimable(cur, seq) && atomicCAS(&ctl.early_state, cur, early_word(seq, EARLY_NOTHING)) == cur; }
// ---- the two composed gates
// F (k_gate_buf, k_feat_begin_pack; one thread per sequence): the tracking chain of frame `want` has released feature buffer `par`.  At the limit the buffer still belongs to an older frame.
__device__ __forceinline__ void gate_buf_wait(const Seq &S, seq_t want, int par) {
    if (!wait_seq(S.ctl->track_done_seq, want, GATE_FATAL)) {
        S.fb[par].fc->poison = 1;
        atomicAdd(&S.ctl->gate_fatal, 1);
        __threadfence();
    }
}
// T (k_gate_late, workgroup 0 of a gated k_match_map; one thread): the early stream has finished with frame seq (early_settled), and the frame's features are there
__device__ __forceinline__ void gate_late_poll(Ctl &ctl, FeatCtl &fc, seq_t seq) {
    seq_t cur;
    while (!wait_seq(ctl.early_state, early_word(seq, EARLY_FINISHED), GATE_LATE_CANCEL, wall_clock64(), &cur)) {
        atomicAdd(&ctl.gate_timeouts, 1);
        if (early_cancel(ctl, cur, seq)) break;  // (claimed: its kernels are running, wait on)
    }
    // this stream has no barrier of its own on the frame's features (the early stream normally vouches for them): make sure
    if (!wait_seq(fc.feat_seq, seq, GATE_FATAL)) {
        ctl.skip = 1;
        atomicAdd(&ctl.gate_fatal, 1);
    }
    if (frame_without_features(fc, seq)) ctl.skip = 1;
}
}  // namespace lvt
