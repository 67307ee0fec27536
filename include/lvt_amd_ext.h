/*
 * lvt_amd_ext.h -- ADDITIVE entry points of the MI355X-native library (nothing here is required of an
 * existing lvt_c caller).  They expose (a) the reference's C++-only API surface over the C-ABI
 * (lvt_system::create with an in-memory lvt_parameters, reset, RGB-D track), (b) zero-copy tracking on
 * images already resident in HBM -- stereo pairs and RGB-D frames (fp32 or 16-bit depth), one handle or a lock-step batch --, (c) read-back of per-frame intermediate results for stage-by-stage
 * parity tests, (d) the batched Hamming matcher micro-benchmark, (e) the EuRoC rectification pre-step and the odometry
 * accumulator either side of the path.
 *
 * Behaviour worth knowing:
 *  - lvt_track / lvt_amd_wait block by spinning on a completion flag in pinned host memory (one busy core, no interrupt latency).
 *  - Host images handed to lvt_track are copied into a pinned staging buffer; page-locked, 16-byte aligned caller buffers
 *    (hipHostMalloc / hipHostRegister) are read in place.
 *  - Environment, read by lvt_create: LVT_AMD_ORDERING=events orders the library's three streams with event barriers instead of
 *    polling gate kernels (needed under tools that serialise kernel dispatches, e.g. rocprofv3 --pmc; ~15 % slower).
 *    Unset, the first live handle of a process polls and single-sequence handles created beside it use events
 *    (lvt_amd_get_ordering); LVT_AMD_ORDERING=polling forces the gates.  A polling handle whose gate runs into its time limit (the streams
 *    do not run side by side) reports it through lvt_amd_last_error and orders with events from the next frame on, unless polling was forced.
 *  - lvt_amd_last_error reports capacity overflows, gate time-outs and "a stream waited 2 s" failures (which set LOST).
 */
#ifndef LVT_AMD_EXT_H__
#define LVT_AMD_EXT_H__

#include "lvt_c.h"
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mirrors struct lvt_parameters (reference lvt/src/lvt_parameters.h:29-64), hot-path fields only */
typedef struct lvt_amd_params {
    float fx, fy, cx, cy;
    float baseline;
    int img_width, img_height;
    float k1, k2, p1, p2, k3;
    float near_plane_distance, far_plane_distance;
    float triangulation_ratio_test_threshold;
    float tracking_ratio_test_threshold;
    float descriptor_matching_threshold;
    int min_num_matches_for_tracking;
    int tracking_radius;
    int detection_cell_size;
    int max_keypoints_per_cell;
    int agast_threshold;
    int untracked_threshold;
    int staged_threshold;
    int triangulation_policy;
} lvt_amd_params;

/* reference lvt_parameters.cpp:29-52 */
LVT_API void lvt_amd_default_params(lvt_amd_params *p);
/* reference lvt_parameters.cpp:54-93; returns 1 on success, 0 if the file cannot be opened */
LVT_API int lvt_amd_params_from_file(const char *config_file_name, lvt_amd_params *p);
/* reference lvt_system::create (lvt_system.cpp:70-127): the path the example binaries use, where the
 * intrinsics are filled in after the YAML is read (kitti_example.cpp:98-106) */
LVT_API lvt_handle lvt_amd_create(const lvt_amd_params *p, int sensor_type);
/* A handle OWNS the HIP device that was current when it was created (lvt_create, lvt_amd_create, lvt_amd_batch_create) or the one
 * named here: every entry point makes that device current for the call and restores the caller's, so one process can drive one
 * handle per GPU from any of its threads.  lvt_amd_get_device: the owning device, -1 for a NULL handle. */
LVT_API lvt_handle lvt_amd_create_on_device(const lvt_amd_params *p, int sensor_type, int device);
LVT_API int lvt_amd_get_device(lvt_handle h);
/* POOLED handles: independent handles of one device folded into ONE lock-step launch chain by a per-device submission thread (lvt_pool.h).  Independent
 * handles with a launch chain each share the process's hardware queues badly -- 2 / 4 / 8 of them reach 0.95 x / 1.47 x / 0.65 x of one handle's frame
 * rate; as seats of a shared chain they reach what a lock-step batch of that size does.  A pooled handle takes ALL FIVE reference entry points (lvt_track,
 * lvt_track_with_external_corners -- the corner lists ride the frame's step --, lvt_get_status, lvt_create with LVT_AMD_POOL=1, lvt_destroy),
 * lvt_amd_track_device[_async], lvt_amd_track_async, lvt_amd_wait[_status], lvt_amd_reset and the per-frame introspection calls, from any thread (one
 * thread per handle at a time, as for every handle); its results are those of a solo handle fed the same frames.  Stereo only; every handle of a pool has
 * the same parameters; at most 16 per device; 4 frames deposited or in flight per handle (a fifth deposit waits for the oldest to complete -- never for the
 * caller's own lvt_amd_wait: results not read yet do not count; beyond 7 un-read frames the oldest result is dropped, as on a solo handle).  A step that
 * cannot be enqueued hands its frames back with lvt_amd_wait_status() == -1 and the reason in lvt_amd_last_error.  Returns NULL when there is no seat or the
 * parameters differ from the pool's.
 * Streams: a lock-step batch of 2 - 28 sequences -- hence every pool -- runs its feature stage on a CU-masked stream (7/8 of the CUs, spread over the XCDs
 * by the driver's round-robin; LVT_AMD_FEATURE_CUS=0 turns the mask off).  HIP can only create such a stream with default flags: work a caller puts on the NULL
 * stream synchronises with it (correct, but serialised) -- callers that overlap their own GPU work with tracking should use non-default streams.
 * LVT_AMD_POOL=1 makes lvt_create / lvt_amd_create / lvt_amd_create_on_device hand out pooled handles (falling back to solo ones);
 * lvt_amd_get_ordering() == 2 says a handle is pooled.  A lone synchronous caller pays two thread hand-overs and the batch code path (the chain is launched as
 * wide as the highest seat in use, and the first seat of a device allocates the 16-sequence batch context -- about sixteen handles' worth of device memory):
 * pooling is for processes that track several sequences at once.
 * AUTOMATIC SEATS (round 6): the reference's own create call, lvt_create, decides by itself.  A stereo handle starts on a launch chain of its own; when a second
 * lvt_create with the same parameters arrives on the device while the first handle has not been used yet (nothing but lvt_amd_get_device / _get_ordering /
 * _last_error was called on it), both -- and every later one -- become seats of the device's pool.  A handle that has tracked keeps its kind (a tracker's
 * state is not moved between chains); RGB-D handles and handles beyond the 16 seats stay solo.  So a process that creates its handles first and tracks afterwards,
 * one thread per sequence, gets the pool without an environment variable (2 / 4 / 8 / 16 handles: 1.25 / 2.27 / 4.33 / 6.74 x of one handle's frame rate instead of
 * 0.94 / - / 0.71 / -), and a lone handle never pays for it.  lvt_amd_create / lvt_amd_create_on_device hand out exactly what they are asked for (their per-stage
 * read-back is mostly a solo handle's).  LVT_AMD_AUTO_POOL=0 turns the automatic seats off. */
LVT_API lvt_handle lvt_amd_create_pooled(const lvt_amd_params *p, int sensor_type, int device /* -1: the current device */);
/* reference lvt_system::reset (lvt_system.cpp:44-68) */
LVT_API void lvt_amd_reset(lvt_handle h);
/* reference lvt_system::track, RGB-D branch (lvt_system.cpp:177-183): gray u8 + depth f32 (metres),
 * both tightly packed host buffers.  (Unreachable through the reference's own C-ABI) */
LVT_API void lvt_amd_track_rgbd(lvt_handle h, const unsigned char *gray, const float *depth, int n_rows,
                                int n_cols, double R[3][3], double t[3]);
/* lvt_track on images already resident in HBM (device pointers, row pitch in bytes, pitch % 16 == 0,
 * pointers 16-byte aligned).  No host<->device image traffic. */
LVT_API void lvt_amd_track_device(lvt_handle h, const void *d_left, const void *d_right, int n_rows,
                                  int n_cols, int pitch_bytes, double R[3][3], double t[3]);
/* asynchronous form: enqueue the frame on the handle's stream and return; the pose is fetched with
 * lvt_amd_wait().  Lets one host thread keep several sequences/GPUs busy. */
LVT_API void lvt_amd_track_device_async(lvt_handle h, const void *d_left, const void *d_right, int n_rows,
                                        int n_cols, int pitch_bytes);
/* asynchronous lvt_track / lvt_amd_track_rgbd on HOST buffers (the reference's own boundary hands over borrowed host images, lvt_c.cpp:64-89; its
 * callers decode frame t+1 while frame t tracks, kitti_example.cpp:113-138): the frame is enqueued and the call returns, the pose comes out of the same
 * FIFO (lvt_amd_wait / lvt_amd_wait_status), at most 6 frames may be un-collected (a further call first blocks on the oldest one).
 *  - pageable buffers are copied into a pinned staging ring during the call: they are the caller's again when it returns;
 *  - page-locked buffers (hipHostMalloc / hipHostRegister) are pulled over PCIe WHERE THEY LIE: they must stay valid and unchanged until that frame
 *    has been collected (lvt_amd_get_host_stats out[2] / out[3] count the planes that went either way).
 * A stereo frame is HELD until the next one arrives or somebody waits for it (lvt_amd_wait* release it when the device would otherwise run dry, every
 * other entry point releases it first): the held frame's corner-cell launch then carries the workgroups that pull the NEXT frame's images over PCIe
 * beside its cells, and the pull is on no stream's chain (out[5] of lvt_amd_get_host_stats counts the frames whose images came that way;
 * LVT_AMD_FUSED_PULL=0: every frame pulls its own images at the head of its feature stage, as RGB-D frames and held frames nobody followed do).
 * Returns 0 when the frame was enqueued; -1 when it was rejected -- wrong image size, NULL buffer, wrong sensor type, a batch handle -- and then
 * NOTHING was enqueued (frames in flight are unaffected, lvt_amd_last_error says why). */
LVT_API int lvt_amd_track_async(lvt_handle h, const unsigned char *left, const unsigned char *right, int n_rows, int n_cols);
LVT_API int lvt_amd_track_rgbd_async(lvt_handle h, const unsigned char *gray, const float *depth, int n_rows, int n_cols);
LVT_API void lvt_amd_wait(lvt_handle h, double R[3][3], double t[3]);
/* the same, returning the tracking state after THAT frame (1 not initialised, 2 tracking, 3 lost; -1 error) -- lvt_get_status would
 * drain the whole pipeline first */
LVT_API int lvt_amd_wait_status(lvt_handle h, double R[3][3], double t[3]);
/* the same with the pose as the tracker holds it (quaternion w x y z + position: what lvt_system::track returns) */
LVT_API int lvt_amd_wait_pose(lvt_handle h, double q_wxyz[4], double p[3]);
/* ---- RGB-D: planes already in HBM, 16-bit depth, lock-step batches ------------------------------------------------------------------
 * The depth element format travels with the frame.  LVT_AMD_DEPTH_F32: metres, as lvt_amd_track_rgbd takes them.  LVT_AMD_DEPTH_U16: what depth cameras
 * deliver (TUM's PNGs: uint16 at 1/5000 m); the tracker samples the 16-bit plane where it has key points -- depth = (float)raw * depth_scale, one rounded
 * fp32 multiply, exactly what a caller converting the plane itself computes -- so a 16-bit frame tracks bit for bit like its fp32 conversion at half the
 * bytes moved, and nobody converts the ~306 000 pixels no key point sits on.  Raw 0 ("no depth") is 0 m: below every near plane, filtered like any other
 * out-of-range depth.  depth_scale is ignored for F32; for U16 it must be finite and > 0.
 * All of these return 0 when the frame was enqueued (or tracked) and -1 when it was refused -- then NOTHING was enqueued, frames in flight are unaffected and
 * lvt_amd_last_error says why (a batch: naming the sequence).  Refused: a stereo or pooled handle (pooled handles are stereo only), a NULL plane, a size that
 * is not the sequence's own, an unknown format, a bad depth_scale, a misaligned plane.  (The other way round, the stereo device calls -- lvt_amd_track_device[_async],
 * lvt_amd_batch_track_device_async[_mixed] -- refuse an RGB-D handle: they have no depth plane to hand over.)
 * Every call of this header and of lvt_c.h that takes a frame or waits for one refuses a handle that is neither a tracker, a pooled seat nor an lvt_create
 * handle -- NULL included -- before it touches the device: -1 where it returns an int, R and t untouched where it returns nothing. */
enum { LVT_AMD_DEPTH_F32 = 0, LVT_AMD_DEPTH_U16 = 1 };
/* one handle, planes resident in HBM.  Gray: 16-byte aligned pointer, pitch a multiple of 16.  Depth: pointer aligned to its element (4 / 2 bytes), pitch in
 * BYTES, a multiple of the element size and >= n_cols elements.  The planes must stay valid and unchanged until the frame has been collected. */
LVT_API int lvt_amd_track_rgbd_device_async(lvt_handle h, const void *d_gray, int gray_pitch_bytes, const void *d_depth, int depth_pitch_bytes,
                                            int depth_format, float depth_scale, int n_rows, int n_cols);
LVT_API int lvt_amd_track_rgbd_device(lvt_handle h, const void *d_gray, int gray_pitch_bytes, const void *d_depth, int depth_pitch_bytes, int depth_format,
                                      float depth_scale, int n_rows, int n_cols, double R[3][3], double t[3]);
/* one handle, HOST buffers (tightly packed, like lvt_amd_track_rgbd[_async]; page-locked ones are read in place), 16-bit depth */
LVT_API int lvt_amd_track_rgbd16(lvt_handle h, const unsigned char *gray, const uint16_t *depth16, float depth_scale, int n_rows, int n_cols,
                                 double R[3][3], double t[3]);
LVT_API int lvt_amd_track_rgbd16_async(lvt_handle h, const unsigned char *gray, const uint16_t *depth16, float depth_scale, int n_rows, int n_cols);
/* one step of a lock-step RGB-D batch -- lvt_amd_batch_create(p, 2, n) and lvt_amd_batch_create_mixed(p, 2, n) alike: arrays of B; d_gray[s] == NULL: sequence s
 * sits this step out (exactly as in lvt_amd_batch_track_device_async_mixed); a step with every pointer NULL is refused.  One format and scale per call (they
 * may change from step to step).  Results: lvt_amd_batch_wait / _get_counts, as for stereo batches. */
LVT_API int lvt_amd_batch_track_rgbd_device_async(lvt_handle h, const void *const *d_gray, const void *const *d_depth, const int *n_rows, const int *n_cols,
                                                  const int *gray_pitch_bytes, const int *depth_pitch_bytes, int depth_format, float depth_scale);
/* ---- lock-step batch of independent sequences on ONE GPU ----------------------------------------------
 * B sequences (e.g. several KITTI drives) advance frame by frame through a single launch chain (every kernel is
 * launched with gridDim.z = B); the latency-bound serial kernels of the path (pose refinement, greedy resolvers)
 * then occupy B compute units instead of one.  Sequences stay fully independent (no cross-sequence data). */
LVT_API lvt_handle lvt_amd_batch_create(const lvt_amd_params *p, int sensor_type, int n_sequences);
LVT_API int lvt_amd_batch_size(lvt_handle h);
/* d_left / d_right: host arrays of B device pointers (one stereo pair per sequence, same size & pitch) */
LVT_API void lvt_amd_batch_track_device_async(lvt_handle h, const void *const *d_left, const void *const *d_right,
                                              int n_rows, int n_cols, int pitch_bytes);
/* oldest un-collected frame: R = B x 9 doubles, t = B x 3 doubles, status = B ints (any may be NULL) */
LVT_API void lvt_amd_batch_wait(lvt_handle h, double *R, double *t, int *status);
LVT_API void lvt_amd_batch_get_counts(lvt_handle h, int seq, int out[32]);
/* ---- MIXED lock-step batch: every sequence with its own parameters ---------------------------------------
 * The reference gives every lvt_system its own lvt_parameters; KITTI 00 - 07 alone has three calibrations and three image sizes.
 * B sequences, sequence s with parameters p[s] (any mix of image size, intrinsics, detection grid, radii, thresholds, triangulation
 * policy).  Shared by the whole batch: the sensor type (stereo, or RGB-D: frames then go through lvt_amd_batch_track_rgbd_device_async) and the capacities (map / feature / cell limits).  NULL when any p[s] is one
 * lvt_amd_create would refuse.  The uniform calls above keep their behaviour and their launches; a mixed batch takes its frames through
 * the _mixed call below (which a uniform batch accepts too). */
LVT_API lvt_handle lvt_amd_batch_create_mixed(const lvt_amd_params *p /* [n_sequences] */, int sensor_type, int n_sequences);
/* per-sequence image geometry: arrays of B.  d_left[s] == NULL: sequence s has NO frame in this step -- it is left exactly as it is: no
 * frame is counted for it, lvt_amd_batch_wait returns its last pose and state, lvt_amd_batch_get_counts its last frame's counters (drives of
 * different lengths share a chain until the longest one ends).  Returns 0 when the step was enqueued; -1 when it was rejected -- a size that
 * is not that sequence's, a pitch that is not a multiple of 16, every pointer NULL -- and then NOTHING was enqueued and lvt_amd_last_error
 * names the sequence. */
LVT_API int lvt_amd_batch_track_device_async_mixed(lvt_handle h, const void *const *d_left, const void *const *d_right,
                                                   const int *n_rows, const int *n_cols, const int *pitch_bytes);
/* the parameters sequence `seq` was created with; 1 / 0 (not a batch handle, seq out of range) */
LVT_API int lvt_amd_batch_get_params(lvt_handle h, int seq, lvt_amd_params *out);
/* the work tables a mixed batch of these parameters launches its corner-score and corner-cell kernels from (host code, no GPU needed):
 * cells[i] = sequence << 16 | eye << 8 | cell, by non-increasing cell area; score[g] = (2 sequence + eye) << 22 | tile row << 8 | tile column for
 * workgroup g.  counts[0 / 1]: entries of the two tables, of which at most cells_cap / score_cap are written.  1 / 0 (refused parameters). */
LVT_API int lvt_amd_batch_mixed_tables(const lvt_amd_params *p, int sensor_type, int n_sequences, unsigned *cells, int cells_cap,
                                       unsigned *score, int score_cap, int counts[2]);

/* ---- a CALLER'S stream ------------------------------------------------------------------------------------------------------
 * Order this handle's frames behind the work of an existing HIP stream (e.g. torch.cuda.current_stream().cuda_stream): the tracking chain runs ON
 * that stream from the next frame on, and the feature stage -- which stays on a stream of the library's -- waits at the head of every frame for an
 * event recorded there.  A single handle or a batch (one stream for the whole batch).
 *  1. INPUTS.  Work enqueued on hip_stream BEFORE a frame call completes before any kernel of that frame reads the caller's planes (image, colour,
 *     raw or depth); no host synchronisation is needed between a producer kernel and lvt_amd_track_device[_async], lvt_amd_track_rgbd_device[_async],
 *     lvt_amd_batch_track_device_async[_mixed] or lvt_amd_batch_track_rgbd_device_async.  Without this call the library's streams are its own and are
 *     ordered behind NOTHING of the caller's: the planes must be complete (host-synchronised) when a frame call is made.
 *  2. RESULTS.  The records -- poses, states, counters, features, the map -- are bit for bit those of a handle on its private stream fed the same frames.
 *  3. RELEASE is unchanged: the planes belong to the tracker until the frame has been collected by the host.
 *  4. The call DRAINS first: the frames in flight are collected on the stream they were enqueued on (lvt_amd_get_host_stats out[1] == out[0] behind it; of
 *     their records the last one stays readable), then the old stream is synchronised.  The stream may be changed between frames any number of times.
 *     The stream stays the caller's: lvt_destroy synchronises it and never destroys it; it must outlive the handle or be replaced first.
 *  5. hip_stream == NULL is the legacy default stream (what the example above is on torch's default stream), for a single handle and for a batch.  (The
 *     CU-masked feature stream of a batch of 2 - 28 sequences synchronises with the NULL stream as every default-flag stream does; that adds waits for
 *     EARLIER work only, which is all a gate of this library ever waits for: DESIGN.md section 2, "A caller's stream".)  A producer that keeps the
 *     stream busy for longer than 20 ms in front of a frame call makes the early stream stand down for that frame, on any stream: reported through
 *     lvt_amd_last_error, results unaffected.
 *  6. A pooled handle runs on its pool's streams: it ignores the call and goes on tracking.  On an lvt_create handle the call is a use: the handle keeps
 *     its own chain when a second lvt_create with the same parameters follows.
 * COST.  The event lands behind the previous frame's tracking chain on the same stream, so a handle on a caller's stream gives up the overlap of a frame's
 * feature stage with the tracking of the frame before it (the asynchronous calls still overlap the host with the GPU).  A handle that never makes this
 * call launches and records exactly what it always did.  Returns nothing: when the event cannot be created the handle stays on the stream it had and
 * lvt_amd_last_error says so. */
LVT_API void lvt_amd_set_stream(lvt_handle h, void *hip_stream);
/* last HIP error string seen by this handle ("" if none); overflow / capacity diagnostics too.  A capacity report is its frame's own: once it has
 * been read here, the next frame collected that fits clears it (read after every frame, the string speaks for that frame; read every N frames, a
 * cut among them is still reported once); lvt_amd_reset clears it as well.  Every other report stays until the next one.
 * BLOCKING: when the last synchronous call returned on its early pose (the frame's tail -- staged update, triangulation -- was still running), this
 * call first collects that frame: its own reports (capacity overflow, a gate that timed out, a skipped frame) arrive with its full record.  A caller
 * that checks the string after EVERY lvt_track therefore gives up the overlap of that tail with its next upload (~30 us per frame); check it every N
 * frames, or use lvt_amd_get_last_pose for pose + state, which never waits.  Not thread-safe against a concurrent call on the same handle (like every
 * entry point); the returned pointer is valid until the next call on the handle (pooled handles: until the calling thread's next call). */
LVT_API const char *lvt_amd_last_error(lvt_handle h);

/* per-kernel timing with HIP events recorded on the handle's stream around every launch of the frame chain.
 * enable=1 resets the accumulators.  lvt_amd_profile_read returns 0 past the last slot. */
/* host-side counters of a handle: out[0] frames enqueued, out[1] frames collected, out[2] image / depth planes of host-buffer calls
   (lvt_track, lvt_amd_track_rgbd, ...) that were read IN PLACE because the caller's buffer is page-locked, out[3] planes copied through the
   library's staging buffer; out[4] frames that came through lvt_amd_track_async / _rgbd_async, out[5] of them: frames whose images were pulled by the launch of the frame before them,
   out[6] launches a lock-step batch's k_score is currently sent in (1 / 2: chosen from the batch's own gate stamps unless LVT_AMD_SCORE_PIECES fixes it),
   out[7] 1 when the handle orders its streams with events */
LVT_API void lvt_amd_get_host_stats(lvt_handle h, long long out[8]);

LVT_API void lvt_amd_profile_enable(lvt_handle h, int enable);
LVT_API int lvt_amd_profile_read(lvt_handle h, int slot, char *name, int name_cap, double *total_ms, long *calls);

/* ---- per-frame introspection (counter slots; the test oracle reports the same ones) ---- */
enum {
    LVT_AMD_C_N_LEFT = 0, LVT_AMD_C_N_RIGHT, LVT_AMD_C_MAP_SIZE, LVT_AMD_C_STAGED_SIZE, LVT_AMD_C_N_MATCHES,
    LVT_AMD_C_SECOND_PASS, LVT_AMD_C_N_ROW_MATCHES, LVT_AMD_C_N_TRIANGULATED, LVT_AMD_C_TRIANGULATED,
    LVT_AMD_C_RETRY_LEFT, LVT_AMD_C_RETRY_RIGHT, LVT_AMD_C_PNP_ITERS, LVT_AMD_C_PNP_INLIERS,
    LVT_AMD_C_MAP_SIZE_AT_MATCH, LVT_AMD_C_N_STAGED_ERASED, LVT_AMD_C_N_STAGED_PROMOTED, LVT_AMD_C_N_CULLED,
    LVT_AMD_C_FRAME, LVT_AMD_C_OVERFLOW /* bitmask of capacity overflows, 0 = none */,
    LVT_AMD_C_PNP_BORDERLINE /* chi2-gate decisions of this frame's pose refinement within 1e-8 of the 5.991 threshold */,
    LVT_AMD_C_ROW_FALLBACK /* 1: the tracking stream built this frame's row-match candidate lists itself (the early stream's were late) */,
    LVT_AMD_C_PNP_TRIALS /* LM trials of this frame's pose refinement */, LVT_AMD_C_PNP_REJECTIONS /* ... rejected ones */,
    LVT_AMD_C_PNP_TERMINATES /* passes ended by g2o's Terminate */,
    LVT_AMD_C__COUNT = 32
};
LVT_API void lvt_amd_get_counts(lvt_handle h, int out[LVT_AMD_C__COUNT]);
LVT_API int lvt_amd_get_features(lvt_handle h, int eye, float *xy, float *resp, uint8_t *desc, int cap);
LVT_API int lvt_amd_get_matches(lvt_handle h, int *feat_idx, double *xyz, int cap);
LVT_API int lvt_amd_get_row_matches(lvt_handle h, int *pairs, int cap);
LVT_API int lvt_amd_get_map(lvt_handle h, double *xyz, int *counter, int *age, uint8_t *desc, int cap);
LVT_API int lvt_amd_get_staged(lvt_handle h, double *xyz, int *counter, uint8_t *desc, int cap);
/* The candidate lists of the last frame, as the list builders left them (for tests that hold the builders to a reference list by list).  Every match starts from
 * such a list: per query the train features that pass the window predicate, as keys (distance << 16 | index), ascending.  which = LVT_AMD_LISTS_MAP: the map
 * points' lists against the left features (of the second pass, where one ran), _STAGED: the staged points' lists behind the pose, _ROW: the left features' lists
 * against the right features.  keys (n x kc words) and counts (n): valid are keys[q][0 .. min(counts[q], kc)); a count above kc says the list overflowed and only
 * the count holds.  proj (n x 2) / vis (n): the queries of the map / staged lists as the device used them (untouched for _ROW, whose queries are the left
 * features).  Lists the frame did not build (first frame, LOST at its start, RGB-D row lists, staged lists without a pose or without staging) come back with n = 0.
 * A single-sequence handle only; host side only (copies behind a drain: no launch, nothing a frame computes changes).  Any pointer may be NULL (not copied).
 * Returns n, or -1: bad handle, a batch, `which` out of range, cap < n (info, when given, is filled in nevertheless). */
enum { LVT_AMD_LISTS_MAP = 0, LVT_AMD_LISTS_STAGED = 1, LVT_AMD_LISTS_ROW = 2 };
typedef struct {
    int kc;                 /* list capacity */
    int stood_down_map;     /* the binned list kernel left this frame's early map lists / row lists to the wavefront-per-query builder behind it */
    int stood_down_row;     /* (0 on a handle that does not run the binned kernel) */
    int pass2;              /* find_matches' second pass ran: the map lists are those of the doubled radius */
    int n_early;            /* map points [0, n_early) were listed on the early stream, the rest by the frame's own prologue */
    int binned;             /* the handle runs the binned list kernel in front of the wavefront-per-query builders */
    int n;                  /* queries of the lists asked for (what the call returns when cap suffices) */
    int reserved;
} lvt_amd_list_info;
LVT_API int lvt_amd_get_candidate_lists(lvt_handle h, int which, unsigned *keys, int *counts, float *proj, signed char *vis, int cap, lvt_amd_list_info *info);
LVT_API void lvt_amd_get_pose(lvt_handle h, double q_wxyz[4], double p[3]);
/* pose (as the tracker holds it) and state (1 / 2 / 3, -1 on error) of the frame the last tracking call returned; unlike lvt_amd_get_pose and
   lvt_get_status it does not wait for that frame's tail (staged update, triangulation) when the call returned on the early pose */
LVT_API int lvt_amd_get_last_pose(lvt_handle h, double q_wxyz[4], double p[3]);
LVT_API void lvt_amd_get_predicted_pose(lvt_handle h, double q_wxyz[4], double p[3]);
/* bring-up profiling: cycle stamps written by detection cell 0 of the left image */
LVT_API void lvt_amd_get_debug(lvt_handle h, long long out[32]);
/* wall-clock (100 MHz) start / end stamps of the kernels on the inter-frame critical path, for the frame lvt_amd_wait returned
 * last (tools/timeline.py); does not drain the pipeline */
LVT_API void lvt_amd_get_timeline(lvt_handle h, long long out[16]);
/* how the handle's streams hand over: 0 = polling gates + early stream (the fast path of a single handle), 1 = event barriers
 * only.  LVT_AMD_ORDERING=polling / events fixes it at creation; unset, the first live handle of a process polls and
 * single-sequence handles created beside it use events (independent handles share the process's hardware queues, and a
 * polling gate holds up whatever another handle queued behind it) */
LVT_API int lvt_amd_get_ordering(lvt_handle h);
/* raw per-pixel intermediates of the last frame: what = 0 score map (u8, rows x pitch),
 * 1 box-sum map (u16, rows x pitch), 2 the rectified image of a handle with rectifiers (u8, rows x pitch; 0 bytes without them),
 * 3 the converted gray image of a handle with a colour pixel format (u8, rows x pitch, before rectification; 0 bytes on a gray handle, and when the
 *   last frame was handed in before the colour format was set: nothing was converted for it),
 * 4 the registered depth plane of a handle with a depth camera (fp32, rows x pitch; 0 bytes without one, and when the last frame was handed in before
 *   the camera was set),
 * 5 the equalised image of a handle with an equalisation record (u8, rows x pitch; 0 bytes without one, and when the last frame was handed in before the
 *   record was set), 6 the tables that image was made with (u8, tiles_x * tiles_y rows of 256),
 * 7 the eye's feature mask as the tracker holds it (u8, rows x pitch, the padding columns zero; 0 bytes for an eye without one; needs no frame).
 * returns bytes written, pitch via *pitch_out (in elements). */
LVT_API int lvt_amd_get_plane(lvt_handle h, int eye, int what, void *dst, int cap_bytes, int *pitch_out);

/* ---- stage entry points on caller-provided data (differential tests vs the oracle) ---- */
/* motion-only BA alone (reference lvt_pnp_solver.cpp:60-128): pts n x 3 f64, obs n x 2 f32 (host) */
LVT_API int lvt_amd_pnp(const lvt_amd_params *p, const double q_in[4], const double p_in[3], const double *pts,
                        const float *obs, int n, double q_out[4], double p_out[3], int *n_solve_calls);
/* the same with the chi2 gates laid open (each may be NULL): err_out = the 2n edge errors the second gate saw, level_out[i] = 1 for an
 * edge a gate demoted (lvt_pnp_solver.cpp:109-116), *borderline = decisions taken within 1e-8 of the 5.991 threshold (those are
 * re-evaluated in the reference's operation order before they are taken; LVT_AMD_C_PNP_BORDERLINE reports the same per frame) */
LVT_API int lvt_amd_pnp_detail(const lvt_amd_params *p, const double q_in[4], const double p_in[3], const double *pts,
                               const float *obs, int n, double q_out[4], double p_out[3], int *n_solve_calls,
                               double *err_out, int *level_out, int *borderline);
/* ... and the Levenberg-Marquardt bookkeeping laid open (g2o's OptimizationAlgorithmLevenberg as configured at lvt_pnp_solver.cpp:44-53, 105-117): trace =
 * trace_cap rows x 4 doubles, one row per LM trial {lambda, chi2 at the estimate, chi2 of the trial, rho} (may be NULL); stats = {trials, rejected
 * trials (rho <= 0 or a non-finite chi2: lambda *= ni, the estimate is popped, the edge errors stay the trial's), passes ended by Terminate (10 trials
 * in one iteration, or rho == 0)}.  LVT_AMD_C_PNP_TRIALS / _REJECTIONS / _TERMINATES report the same per frame. */
LVT_API int lvt_amd_pnp_trace(const lvt_amd_params *p, const double q_in[4], const double p_in[3], const double *pts,
                              const float *obs, int n, double q_out[4], double p_out[3], int *n_solve_calls,
                              double *err_out, int *level_out, int *borderline, double *trace, int trace_cap, int stats[3]);
/* the constant-velocity motion model alone (reference lvt_motion_model.cpp:42-65), run by one device thread through the frame path's own code: state =
 * {last_q[4] (w x y z), ang_vel[4], last_p[3], lin_vel[3]} on entry, the model's next state on return; q, p = the current pose; q_out, p_out = the
 * predicted one.  Host pointers; runs on the current device.  0 on success, -1 on a NULL argument or a HIP failure. */
LVT_API int lvt_amd_motion_predict(double state[14], const double q[4], const double p[3], double q_out[4], double p_out[3]);
/* batched masked 2-NN Hamming (reference lvt_image_features_struct.cpp:68-120 + cv::BFMatcher knnMatch k=2):
 * B independent problems; per problem M queries (desc 32 B, xy f32) against N train (desc, xy, flag u8);
 * candidate iff !flag && dx*dx+dy*dy < r2 (f32, strict) [mode 0] or |band| row test [mode 1].
 * All pointers are DEVICE pointers; out: B x M x 4 int32 (idx1,d1,idx2,d2; -1/INT_MAX when absent).
 * Returns the kernel's elapsed time in microseconds (HIP events on `stream`), <0 on error. */
LVT_API float lvt_amd_hamming_match_batched(const void *q_desc, const void *q_xy, const void *t_desc,
                                            const void *t_xy, const void *t_flag, int B, int M, int N,
                                            float r2, int mode, int img_rows, int img_cols, void *out,
                                            void *hip_stream);
/* same, `launches` identical launches back to back between the two events; returns the AVERAGE per launch (a single
 * launch's event pair also times ~5 us of launch latency -- this is the form bench.py's roofline uses) */
LVT_API float lvt_amd_hamming_match_batched_n(const void *q_desc, const void *q_xy, const void *t_desc,
                                              const void *t_xy, const void *t_flag, int B, int M, int N,
                                              float r2, int mode, int img_rows, int img_cols, void *out,
                                              void *hip_stream, int launches);

/* ---- EuRoC pre-step: stereo rectification (reference examples/euroc/euroc_example.cpp:95-107,142-143 = cv::initUndistortRectifyMap
 * with CV_32FC1 maps + cv::remap INTER_LINEAR, BORDER_CONSTANT 0).  K, R, Pnew row-major 3x3, D = k1 k2 p1 p2 k3.
 * The maps are built once on the device; lvt_amd_rectify_device rectifies one 8-bit image already in HBM: ONE launch on hip_stream, in that stream's
 * order, nothing is synchronised.  src_pitch >= width (the source's padding is never read); dst_pitch >= width and dst_pitch % 4 == 0: every byte of
 * height x dst_pitch is written, the columns from width on as zero, nothing behind them.  Returns 0; -1 (NULL, a pitch that breaks these rules) and then
 * nothing was launched.  lvt_amd_rectify does the same for tightly packed host buffers.
 *
 * RECTIFICATION, the arithmetic of one output pixel.  For a map entry m (either map) the 1/32-px fixed-point value is
 *   - cvRound(m * 32.f), round half to even, when the fp32 product is finite and inside (-2^31, 2^31);
 *   - INT_MIN otherwise (NaN, an infinity, |m * 32.f| >= 2^31).
 * The sample's corner is (sxf >> 5, syf >> 5) (an arithmetic shift: it floors), each clamped to -32768 ... 32767; the fractions are sxf & 31, syf & 31 (never
 * negative); the four weights are (32 - ax)(32 - ay) 32, ax (32 - ay) 32, (32 - ax) ay 32, ax ay 32, except 32767, 0, 0, 1 where both fractions are zero; a
 * source pixel outside sw x sh counts as 0; the pixel is (sum + 2^14) >> 15, clamped to 0 ... 255.  An INT_MIN entry is at -32768 behind the shift and the
 * clamp: outside every source, and the pixel is 0.  The map builder produces such entries where the homogeneous coordinate of a row passes through zero (the
 * rectifying rotation puts the new camera's horizon inside the image) and on a garbage calibration, which lvt_amd_rectifier_create accepts.  The INT_MIN
 * part of the rule is cv::remap on x86 as OpenCV's source reads (cvRound(float) is cvtss2si, whose answer outside int is 0x80000000), not as something run.
 *
 * lvt_amd_remap_device: that arithmetic alone on caller data.  d_src (sh rows of src_pitch >= sw bytes, any address) and d_dst (dh rows of dst_pitch bytes,
 * dst_pitch >= dw, dst_pitch % 4 == 0, 4-byte aligned) are DEVICE pointers, map1 / map2 HOST arrays of dw x dh floats; the map's size need not be the
 * source's.  route 0: k_rectify on the float maps (lvt_amd_rectify_device's launch); route 1: k_rectify_fix, then k_rectify_frames with a table of one image
 * (a tracker's feature stage).  Every byte of dh x dst_pitch is written, the columns from dw on as zero, nothing else.  Null stream; returns when the plane is
 * written.  *launches (may be NULL): kernels launched.  Refused (-1, *launches = 0, nothing launched, the sentence in lvt_amd_last_error(NULL)): a NULL
 * pointer, a size <= 0, src_pitch < sw, dst_pitch < dw or dst_pitch % 4 != 0 or a misaligned d_dst, src_pitch * sh or dst_pitch * dh beyond INT_MAX, an
 * unknown route. ---- */
typedef void *lvt_amd_rectifier;
LVT_API int lvt_amd_remap_device(const void *d_src, int sw, int sh, int src_pitch, const float *map1, const float *map2, int dw, int dh,
                                 void *d_dst, int dst_pitch, int route, int *launches);
LVT_API lvt_amd_rectifier lvt_amd_rectifier_create(const double K[9], const double D[5], const double R[9],
                                                   const double Pnew[9], int width, int height);
LVT_API void lvt_amd_rectifier_destroy(lvt_amd_rectifier r);
LVT_API int lvt_amd_rectify_device(lvt_amd_rectifier r, const void *d_src, int src_pitch, void *d_dst, int dst_pitch,
                                   void *hip_stream);
LVT_API int lvt_amd_rectify(lvt_amd_rectifier r, const unsigned char *src, unsigned char *dst);
LVT_API int lvt_amd_rectifier_get_maps(lvt_amd_rectifier r, float *map1, float *map2);

/* LENS MODELS: a rectifier from a lens record, for a raw image of any size.  lvt_amd_rectifier_create knows the five-coefficient plumb-bob lens and one size;
 * lvt_amd_rectifier_create_lens takes the three models a calibration arrives in (ROS CameraInfo, Kalibr, OpenCV) and a SOURCE (the raw image,
 * lens.width x lens.height) that need not be the DESTINATION (the rectified image and the maps, dst_width x dst_height):
 *   - LVT_AMD_LENS_RADTAN: plumb_bob (D[5 ...] zero) and rational_polynomial, OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, unused ones zero;
 *   - LVT_AMD_LENS_FISHEYE: equidistant (cv::fisheye, Kalibr pinhole-equi), D = k1 k2 k3 k4; D[4 ...] is not read.
 * The text below is the definition: the maps are equal to it, bit for bit (FISHEYE: up to the last bit of atan, see there).  It follows the published
 * arithmetic of cv::initUndistortRectifyMap and cv::fisheye::initUndistortRectifyMap with CV_32FC1 maps, with two known differences: the tilted-sensor terms
 * (tauX, tauY) are not taken, and cv::fisheye inverts Pnew R by SVD where both models here use the closed form below.
 *
 * Shared by both models.  All arithmetic is fp64, one IEEE operation per written operation (no fused multiply-add), operands left to right.
 *   - iR is the inverse of the product Pnew R (each entry summed over k ascending) by cofactors: d = S0 (S4 S8 - S5 S7) - S1 (S3 S8 - S5 S6) + S2 (S3 S7 - S4 S6);
 *     d == 0: iR = I; otherwise every cofactor times (1 / d) -- what lvt_amd_rectifier_create computes.
 *   - for destination row i: _x = i iR[1] + iR[2], _y = i iR[4] + iR[5], _w = i iR[7] + iR[8] at column 0; stepping one column adds iR[0], iR[3], iR[6].
 *     This is a left-to-right chain of rounded adds along the row, and the chain IS the definition (start + j step rounds differently).
 * RADTAN.  iw = 1 / _w, x = _x iw, y = _y iw, x2 = x x, y2 = y y, r2 = x2 + y2, _2xy = 2 x y,
 *     kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2),
 *     xd = x kr + p1 _2xy + p2 (r2 + 2 x2) + s1 r2 + (s2 r2) r2,    yd = y kr + p1 (r2 + 2 y2) + p2 _2xy + s3 r2 + (s4 r2) r2,
 *     u = fx xd + u0, v = fy yd + v0.  With k4 ... s4 zero and equal sizes these are lvt_amd_rectifier_create's maps, bit for bit.
 * FISHEYE.  If _w <= 0 (a ray from behind the new camera): u = (_x > 0) ? -inf : +inf, v = (_y > 0) ? -inf : +inf.  Otherwise
 *     x = _x / _w, y = _y / _w, r = sqrt(x x + y y), theta = atan(r), t2 = theta theta, t4 = t2 t2, t6 = t4 t2, t8 = t4 t4,
 *     theta_d = theta ((((1 + k1 t2) + k2 t4) + k3 t6) + k4 t8), scale = (r == 0) ? 1 : theta_d / r,
 *     u = (fx x) scale + u0, v = (fy y) scale + v0.
 *     sqrt and the divisions are correctly rounded; atan is the device library's, which may differ from another libm's in its last bit.
 * Both maps are (float)u, (float)v.  Everything behind them is RECTIFICATION above: the 1/32-px fixed point, INT_MIN for NaN, infinities and out-of-range
 * values (the pixel is 0), and the remap from a source of lens.width x lens.height.
 *  - the remap stays bilinear (no area filter): a source more than about twice the destination each way aliases.  Choose Pnew and the destination accordingly.
 *  - with such a rectifier lvt_amd_rectify takes a tightly packed lens.width x lens.height image and writes a dst_width x dst_height one; lvt_amd_rectify_device
 *    wants src_pitch >= lens.width, and the destination rules are unchanged; lvt_amd_rectifier_get_maps writes dst_width x dst_height floats per map.
 *  - lvt_amd_rectifier_create_lens returns NULL, with the sentence in lvt_amd_last_error(NULL) ending in "(nothing was created)", in this order, for: a NULL
 *    argument; an unknown model; a source side outside 1 ... 8192; a destination side outside 1 ... 8192; a non-finite field of K or D (FISHEYE: of D[0 ... 3]);
 *    a non-finite field of R or Pnew.  A singular Pnew R is accepted as by lvt_amd_rectifier_create (iR = I).
 *  - lvt_amd_rectifier_get_info: the record the rectifier was made from (FISHEYE: D[4 ...] read back as zero; a rectifier of lvt_amd_rectifier_create: RADTAN,
 *    its five coefficients, width x height both ways) and dst_size = {dst_width, dst_height}.  0; -1 for a NULL argument.
 *  - not here: the tilted-sensor and omnidirectional (Mei) models; computing R and Pnew from a stereo extrinsic (cv::stereoRectify). */
enum { LVT_AMD_LENS_RADTAN = 0, LVT_AMD_LENS_FISHEYE = 1 };
typedef struct lvt_amd_lens {
    int model;
    int width, height;     /* of the RAW image, 1 ... 8192 each way */
    double K[9];           /* row-major; fx, fy, u0, v0 are read */
    double D[12];          /* RADTAN: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 (OpenCV's order, unused ones zero); FISHEYE: k1 k2 k3 k4, the rest ignored */
} lvt_amd_lens;
LVT_API lvt_amd_rectifier lvt_amd_rectifier_create_lens(const lvt_amd_lens *lens, const double R[9], const double Pnew[9], int dst_width, int dst_height);
LVT_API int lvt_amd_rectifier_get_info(lvt_amd_rectifier r, lvt_amd_lens *lens_out, int dst_size[2]);   /* 0 / -1 */

/* RAW stereo frames: rectification inside the tracker's feature stage.  With a pair of rectifiers attached, every stereo frame handed to the handle --
 * lvt_track, lvt_amd_track_async, lvt_amd_track_device[_async]; a batch: the sequences with rectifiers in lvt_amd_batch_track_device_async[_mixed] -- is a RAW
 * frame: one launch at the head of the feature stage (k_rectify_frames: both eyes of every such sequence of the step) rectifies it into planes the tracker
 * owns, byte for byte what lvt_amd_rectify_device writes, and the frame is tracked from those.  No host round trip, no second upload, no launch or stream of the
 * caller's to order.  A handle or sequence without rectifiers launches exactly what it did before.
 *  - THE FRAME'S SIZE.  A pair's DESTINATION size is the sequence's img_width x img_height; its two SOURCE sizes (lvt_amd_rectifier_create: the same size;
 *    lvt_amd_rectifier_create_lens: the lens's width x height) are equal to each other and need not be the destination's.  From the attach on the sequence's
 *    frame size is the source size: every stereo entry point takes n_rows x n_cols = the source's and refuses anything else, the tracker's own size
 *    included; a batch sequence in lvt_amd_batch_track_device_async_mixed likewise (sit-outs as ever), and lvt_amd_batch_track_device_async wants its one size
 *    to be every sequence's.  Detaching returns the sequence to its own size.  What is sized by the frame's bytes follows the source (the staging buffers,
 *    the image ring and the fused pull of lvt_amd_track_async, with a colour format the colour and the converted planes: convert at the source's size, then
 *    remap); everything behind the rectified plane -- equalisation, masks, label masks, the detector -- stays at the sequence's size.  A pair whose source is
 *    the destination's size allocates and launches exactly what it always did.
 *  - host entry points pull the raw images where they pulled the rectified ones (the staged planes of the call, the fused pull of lvt_amd_track_async included);
 *    device entry points read the caller's raw planes in place: any pitch >= n_cols (the pitch % 16 rule applies to rectified planes only); the planes must
 *    stay valid until the frame has been collected, as always.
 *  - the rectifiers are BORROWED: they must outlive the handle or be detached first (NULL, NULL detaches; one NULL is refused); several sequences and handles may
 *    share a pair.
 *  - refused (-1, nothing changed, the reason in lvt_amd_last_error), in this order behind the handle's kind: one rectifier NULL; per rectifier, left first, a
 *    DESTINATION size that is not the sequence's img_width x img_height, then one created on another device; two source sizes that differ (the sentence names
 *    both); frames in flight.  Also an RGB-D handle, a pooled or automatic seat, seq out of range, a handle with frames in flight (attach before the first frame or after every
 *    frame has been collected).  A successful attach counts as use of an lvt_create handle: it stays on its own chain when a second lvt_create arrives.
 *  - lvt_track_with_external_corners on such a handle is refused (nothing is tracked, lvt_amd_last_error says so): the corners would be in rectified coordinates.
 *  - lvt_amd_get_plane(h, eye, 2, ...) reads the rectified image of the last frame back (u8, rows x pitch; 0 for a handle without rectifiers); what = 3 (the
 *    converted gray image of a colour handle, before the remap) has the SOURCE's rows and a pitch of its own when the source is not the sequence's size;
 *    lvt_amd_profile_read reports the launch as "k_rectify_frames". */
LVT_API int lvt_amd_set_rectifiers(lvt_handle h, lvt_amd_rectifier left, lvt_amd_rectifier right);
LVT_API int lvt_amd_batch_set_rectifiers(lvt_handle h, int seq, lvt_amd_rectifier left, lvt_amd_rectifier right);

/* COLOUR frames: gray conversion inside the tracker's feature stage.  The pixel format is a property of the handle, or of one sequence of a batch, like the
 * rectifiers.  Once a colour format is set, EVERY frame-taking call on that handle or sequence -- lvt_track, lvt_track_with_external_corners,
 * lvt_amd_track_async, lvt_amd_track_device[_async], lvt_amd_track_rgbd[_async], lvt_amd_track_rgbd16[_async], lvt_amd_track_rgbd_device[_async], the
 * batch calls (sit-outs included) -- takes its image(s) interleaved in that format.  One launch at the head of the feature stage (k_gray_frames: every
 * colour image of the step) converts them into planes the tracker owns,
 *     gray = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14        (cv::cvtColor's 8-bit BGR2GRAY; (255,0,0) -> 76, (0,255,0) -> 150, (0,0,255) -> 29)
 * and the frame is tracked from those; with rectifiers attached the order is the reference's: convert, then remap.  The alpha byte of the 4-byte formats
 * is ignored.  A handle or sequence that never sets a format launches exactly what it did before; LVT_AMD_PIX_GRAY8 returns a handle to that path.
 *  - n_rows / n_cols stay in PIXELS.  Host buffers are tightly packed, n_cols * bpp bytes per row; page-locked ones are read in place as before.
 *  - device planes: any base address and any pitch_bytes >= n_cols * bpp (a smaller pitch is refused); the pitch % 16 / 16-byte alignment rules belong to gray
 *    planes.  For RGB-D the `gray` argument is the colour image; the depth plane and its format are untouched.
 *  - external corners are in the same coordinates: lvt_track_with_external_corners stays allowed.
 *  - refused (-1, nothing changed, the reason in lvt_amd_last_error): an unknown format, a pooled or automatic seat, seq out of range, the batch call on a
 *    handle that is not a batch and the other way round, a handle with frames in flight (set the format before the first frame or after every frame has
 *    been collected).  A successful set counts as use of an lvt_create handle.
 *  - lvt_amd_get_plane(h, eye, 3, ...) reads the converted gray plane of the last frame back; lvt_amd_profile_read reports the launch as "k_gray_frames". */
enum { LVT_AMD_PIX_GRAY8 = 0, LVT_AMD_PIX_BGR8 = 1, LVT_AMD_PIX_RGB8 = 2, LVT_AMD_PIX_BGRA8 = 3, LVT_AMD_PIX_RGBA8 = 4 };
LVT_API int lvt_amd_set_pixel_format(lvt_handle h, int format);                 /* 0 / -1 */
LVT_API int lvt_amd_batch_set_pixel_format(lvt_handle h, int seq, int format);  /* 0 / -1 */
LVT_API int lvt_amd_get_pixel_format(lvt_handle h, int seq);                    /* format, -1: bad handle / seq */

/* SENSOR FORMATS: Bayer mosaics, YUV 4:2:2 and 16-bit gray, turned into 8-bit gray inside the tracker's feature stage.  A sensor format is a property of the
 * handle, or of one sequence of a batch, like the pixel format; the record is copied.  It is not state: lvt_amd_reset, lvt_amd_batch_reset and snapshots
 * neither hold nor change it.  Once it is set, EVERY frame-taking call on that handle or sequence, of either sensor (on an RGB-D sequence it describes the one
 * image), host or device, synchronous or asynchronous, the batch calls uniform and mixed, sit-outs included, takes the sensor's plane, and one launch at the
 * head of the feature stage (k_sensor_frames: every such image of the step, in k_gray_frames' place: convert, reduce, remap, equalise) writes the gray planes
 * the frame is tracked from.  A handle or sequence that never sets one allocates and launches exactly what it did; format = LVT_AMD_SENSOR_NONE unsets the
 * property, frees what only it allocated and returns the handle to that path.
 *  THE DEFINITION -- integer arithmetic throughout; tests/sensor_util.py restates it in numpy and the checks hold the kernels to it byte for byte (the claim
 *  is equality with this text, not with any library's demosaicing).
 *   - BAYER (8 bit).  The pattern names the colours of pixels (0,0), (1,0) / (0,1), (1,1).  A channel that is missing at a pixel is the mean of the nearest
 *     samples of that colour -- 4 diagonal, 4 axial or 2 axial -- kept unscaled as X4 = 4 x the value: the sum of four, twice the sum of two, or four times
 *     the pixel's own sample.  Neighbours outside the image are mirrored without repeating the edge (-1 -> 1, W -> W - 2; rows likewise): the colour phase is
 *     kept.       gray = (4899 R4 + 9617 G4 + 1868 B4 + 32768) >> 16            (one rounding; the largest sum is 16 744 448)
 *     A flat field R = G = B = v gives v.  A mosaic of an image that is constant per channel has X4 = 4 X everywhere, and (4 s + 32768) >> 16 ==
 *     (s + 8192) >> 14: it gives exactly the value of COLOUR frames above for that colour.
 *   - YUYV / UYVY (YUV 4:2:2).  gray[y][x] = row[2 x] / row[2 x + 1].  No range expansion (a limited-range 16 ... 235 luma stays 16 ... 235).
 *   - MONO16 (little-endian uint16_t), window [lo, hi]:   g = min(max(v, lo), hi);   out = ((g - lo) * 255 + ((hi - lo) >> 1)) / (hi - lo)   (truncating;
 *     below 2^24).  auto_window = 0: the record's lo, hi.  auto_window = 1: per image and per frame from the frame's own histogram -- 4096 bins of v >> 4
 *     over the W x H pixels, cum(b) = pixels in bins <= b, N = W H, 64-bit products:
 *         lo_bin = the smallest b with cum(b) * 1000 > lo_permille * N;     hi_bin = the smallest b with cum(b) * 1000 >= (1000 - hi_permille) * N;
 *         lo = 16 lo_bin, hi = 16 hi_bin + 15;   where hi - lo < min_span:  mid = (lo + hi) >> 1, lo = max(0, mid - (min_span >> 1)), hi = lo + min_span,
 *         and if hi > 65535 then hi = 65535, lo = hi - min_span.
 *     Two further launches in front of the conversion (k_sensor_hist, k_sensor_levels), only where a sequence asks for it.  Each frame stands alone: the
 *     window is NOT smoothed over frames.
 *  - a row is W bytes (Bayer) or 2 W bytes (YUYV, UYVY, MONO16); n_rows / n_cols stay in PIXELS.  Host buffers are tightly packed.  Device planes are read in
 *    place at any address and any pitch that holds a row; MONO16 needs an even address and an even pitch and is refused otherwise.
 *  - MUTUALLY EXCLUSIVE with a colour pixel format: either setter is refused on a sequence that has the other.
 *  - external corners are in the same coordinates: lvt_track_with_external_corners stays allowed.
 *  - refused (-1, nothing changed, the reason in lvt_amd_last_error, every sentence ending "(nothing was changed)"), in this order: a pooled or automatic
 *    seat; the batch call on a handle that is not a batch and the other way round; seq out of range; a bad record -- NULL; an unknown format; for MONO16
 *    auto_window outside 0 ... 1, then (fixed) lo, hi outside 0 <= lo < hi <= 65535 or (auto) lo_permille, hi_permille outside 0 ... 499, min_span outside
 *    1 ... 65535; for Bayer a frame narrower or lower than 2 pixels: the sentence names the field --; a sequence with a colour pixel format; a handle with
 *    frames in flight.  A successful set counts as use of an lvt_create handle.  The fields a format does not use are ignored.
 *  - lvt_amd_get_sensor_format: 1 = a format is set (copied to *out), 0 = none, -1 = bad handle / seq.
 *  - lvt_amd_get_sensor_window: the window image `eye` (0 / 1; RGB-D: 0) of sequence seq was mapped with in the last collected frame: 1 with lo, hi; 0 where
 *    there is none (no MONO16 format, no frame yet, or the sequence SAT OUT of the last collected step -- whatever it tracked before: the answer is about
 *    that step, and it is 1 again after the next step the sequence has a frame in); -1 = bad handle / seq / eye.  A fixed window reports
 *    the record's.
 *  - lvt_amd_get_plane(h, eye, 3, ...) reads the converted plane of the last frame back, as for colour.  lvt_amd_profile_read reports the launches as
 *    "k_sensor_frames", "k_sensor_hist" and "k_sensor_levels" (the first for a handle with a sensor format only, the other two for one with an auto window only).
 *  - lvt_amd_convert_sensor_device: the stage alone on caller planes (device pointers).  src: height rows of src_pitch_bytes >= a row, any address (MONO16:
 *    even); dst: height rows of dst_pitch bytes, dst_pitch >= width, dst_pitch % 4 == 0, 4-byte aligned; sides 1 ... 16384 (Bayer: 2 ...).  Every byte of the
 *    destination rows is written, the columns from width on as zero, nothing else.  window_out (may be NULL): the window a MONO16 image was mapped with
 *    ({0, 0} for the other formats).  Null stream; returns when the plane is written.  0, or -1 (nothing launched, the sentence in lvt_amd_last_error(NULL)).
 *  - not here: range expansion for YUV; smoothing of the auto window over frames; 10- and 12-bit PACKED formats; planar NV12, whose Y plane already is a gray
 *    plane with a pitch and enters as one. */
enum { LVT_AMD_SENSOR_NONE = 0,
       LVT_AMD_SENSOR_BAYER_RGGB8 = 16, LVT_AMD_SENSOR_BAYER_BGGR8 = 17, LVT_AMD_SENSOR_BAYER_GRBG8 = 18, LVT_AMD_SENSOR_BAYER_GBRG8 = 19,
       LVT_AMD_SENSOR_YUYV = 24, LVT_AMD_SENSOR_UYVY = 25,
       LVT_AMD_SENSOR_MONO16 = 32 };
typedef struct {
    int format;
    int auto_window;        /* MONO16: 0 = [lo, hi] below, 1 = from each frame's histogram */
    int lo, hi;             /* MONO16 fixed window, 0 <= lo < hi <= 65535 */
    int lo_permille, hi_permille;   /* MONO16 auto: share of pixels allowed below / above the window, each 0 ... 499 */
    int min_span;           /* MONO16 auto: smallest hi - lo, 1 ... 65535 */
    int reserved[1];
} lvt_amd_sensor_format;
LVT_API int lvt_amd_set_sensor_format(lvt_handle h, const lvt_amd_sensor_format *f);
LVT_API int lvt_amd_batch_set_sensor_format(lvt_handle h, int seq, const lvt_amd_sensor_format *f);
LVT_API int lvt_amd_get_sensor_format(lvt_handle h, int seq, lvt_amd_sensor_format *out);
LVT_API int lvt_amd_get_sensor_window(lvt_handle h, int seq, int eye, int *lo, int *hi);   /* the window the last collected frame was mapped with */
LVT_API int lvt_amd_convert_sensor_device(const lvt_amd_sensor_format *f, const void *src, int src_pitch_bytes, int width, int height,
                                          uint8_t *dst, int dst_pitch, int window_out[2]);   /* the stage alone, on caller planes in HBM */

/* FRAME REDUCTION: large frames, averaged down by an integer factor inside the tracker's feature stage.  The tracker's capacities are shaped for KITTI- and
 * VGA-sized images; cameras deliver 1080p to 4K.  A reduction is a property of the handle, or of one sequence of a batch, like the pixel format; the record is
 * copied.  It is not state: lvt_amd_reset, lvt_amd_batch_reset and snapshots neither hold nor change it.  Once it is set, EVERY frame-taking call on that
 * handle or sequence, of either sensor, takes frames of the record's width x height, and one launch at the head of the feature stage (k_reduce_frames: every
 * such image of the step) averages them into planes the tracker owns; the frame is tracked from those.  A handle or sequence that never sets a record
 * allocates and launches exactly what it did, and factor = 1 returns a handle to that path and releases what was sized by the large frame.
 *  THE DEFINITION (tests/reduce_util.py restates it in numpy; the checks hold the kernel to it byte for byte).
 *   - bW x bH is the BASE size: the rectifiers' source size where a pair is attached, else the sequence's img_width x img_height.
 *   - a record is valid when factor is 1 ... 8 and width, height are 1 ... 16384; for factor f >= 2 also width / f == bW and height / f == bH (integer
 *     division): the frame may carry up to f - 1 trailing columns and rows, which are never read.
 *   - for a gray frame g and 0 <= x < bW, 0 <= y < bH:
 *         S = sum over dy, dx in [0, f) of g[f y + dy][f x + dx];      out[y][x] = (S + (f f >> 1)) / (f f)        (integer division; S <= 255 f f)
 *   - a colour frame is converted first, per pixel, by the formula of COLOUR frames above; the gray image is then averaged.
 *   - ORDER in the feature stage: convert, REDUCE, remap, equalise.  Everything behind the reduced plane stays at the sizes it has without a reduction: the
 *     rectified planes, equalisation, masks, label masks, the detector and everything downstream.
 *   - GEOMETRY.  Reduced pixel x covers source columns [f x, f x + f), so with pixel centres at integers a pinhole of the frame becomes
 *         fx' = fx / f,   cx' = (cx + 0.5) / f - 0.5,   fy' = fy / f,   cy' = (cy + 0.5) / f - 0.5;
 *     distortion coefficients (functions of the normalised ray) and the baseline in metres are unchanged.  The sequence's lvt_amd_params are those of the
 *     REDUCED image: the caller computes them (lvt_amd_lens_reduced does, for a lens record).
 *   - the gain over picking pixels has been measured on synthetic texture only (profiles/frame_reduction.md); it has not been measured on real footage.
 *  - THE FRAME'S SIZE is the record's width x height at every entry point; anything else is refused like any other wrong size, the tracker's own included.
 *    What is sized by the frame's bytes follows it (the staging buffers, the planes the host entry points pull into, the colour and the converted planes).
 *  - host buffers are tightly packed at the frame's size.  Device planes are read in place: any base address, any pitch >= width * bpp (where base and pitch
 *    are multiples of 4 the kernel loads 8- and 16-byte vectors, otherwise bytes: the same result).
 *  - RECTIFIERS first, then the reduction: the reduced image is the rectifiers' source (make them from lvt_amd_lens_reduced's record).  With a reduction in
 *    force lvt_amd_set_rectifiers / lvt_amd_batch_set_rectifiers, attach or detach, are refused: clear the reduction first.
 *  - lvt_track_with_external_corners on such a handle is refused (nothing is tracked): the call cannot know which image the corners are in.
 *  - RGB-D: a frame on a sequence with a reduction and WITHOUT a depth camera is refused before anything is enqueued -- the depth plane has no size of its own.
 *    A depth plane registered to the large colour image enters through lvt_amd_set_depth_camera with identity extrinsics and the large image's pinhole.
 *  - refused (-1, nothing changed, the reason in lvt_amd_last_error, every sentence ending "(nothing was changed)"), in this order: a pooled or automatic seat;
 *    the batch call on a handle that is not a batch and the other way round; seq out of range; a bad record (NULL, then factor, width, height, then the
 *    size that does not reduce to the base -- the sentence names both); a handle with frames in flight.  A successful set counts as use of an lvt_create handle.
 *  - lvt_amd_get_reduction: 1 = a reduction is in force (copied to *out), 0 = none, -1 = bad handle / seq.
 *  - lvt_amd_get_plane(h, eye, 9, ...) reads the reduced plane of the last frame back (u8, bH rows, its pitch in *pitch_out, the padding columns zero; 0 bytes
 *    without a reduction); what = 3 (the converted gray of a colour handle) then has the frame's rows and a pitch of its own.  lvt_amd_profile_read reports the
 *    launch as "k_reduce_frames" (a handle with a reduction only).
 *  - lvt_amd_reduce_device: the stage alone on caller planes (device pointers, u8).  d_src: src_h rows of src_pitch >= src_w bytes, any address; d_dst:
 *    src_h / factor rows of dst_pitch bytes, dst_pitch >= src_w / factor, dst_pitch % 4 == 0, 4-byte aligned; factor 2 ... 8, sides factor ... 16384.  Every
 *    byte of the destination rows is written, the columns from src_w / factor on as zero, nothing else.  Null stream; returns when the plane is written.
 *    *launches (may be NULL): kernels launched.  0, or -1 (*launches = 0, nothing launched, the sentence in lvt_amd_last_error(NULL)).
 *  - lvt_amd_lens_reduced: host only, no device.  *out = the lens of the reduced image by the GEOMETRY rule, in double (K[0], K[4] divided; K[2], K[5]
 *    shifted; width, height by integer division; model and D copied).  factor 1 ... 8; -1 for a NULL argument, another factor, or a side that reduces to 0.
 *  - not here: fusing the colour conversion into the reduction; a non-integer factor. */
typedef struct lvt_amd_reduction {
    int factor;           /* 1 = off; 2 ... 8 */
    int width, height;    /* the FRAME's size in pixels, as every entry point will then take it */
} lvt_amd_reduction;
LVT_API int lvt_amd_set_reduction(lvt_handle h, const lvt_amd_reduction *r);                        /* 0 / -1 */
LVT_API int lvt_amd_batch_set_reduction(lvt_handle h, int seq, const lvt_amd_reduction *r);
LVT_API int lvt_amd_get_reduction(lvt_handle h, int seq, lvt_amd_reduction *out);                   /* 1 set, 0 none, -1 bad handle / seq */
LVT_API int lvt_amd_reduce_device(const void *d_src, int src_w, int src_h, int src_pitch, int factor,
                                  void *d_dst, int dst_pitch, int *launches);                       /* the stage alone, caller planes in HBM */
LVT_API int lvt_amd_lens_reduced(const lvt_amd_lens *in, int factor, lvt_amd_lens *out);            /* host only, no device */

/* UNREGISTERED DEPTH: depth registration inside the tracker's feature stage. Without a depth camera the depth plane of an RGB-D frame is taken as registered
 * to the gray image (TUM's files, sensors that register in hardware).  A depth camera says that the plane is delivered in ANOTHER camera -- its own size,
 * its own pinhole, a rigid offset from the colour camera (RealSense D4xx: the left infrared camera; Azure Kinect, Orbbec: a second camera a few centimetres
 * away).  It is a property of the handle, or of one sequence of a batch, like the pixel format; the record is copied.  It is not state: it is neither in
 * snapshots nor restored by them.  Once it is set, EVERY RGB-D frame-taking call on that handle or sequence -- lvt_amd_track_rgbd[_async],
 * lvt_amd_track_rgbd16[_async], lvt_amd_track_rgbd_device[_async], lvt_amd_batch_track_rgbd_device_async (uniform and mixed, sit-outs included) -- takes the depth
 * plane as the sensor delivers it, cam.width x cam.height, in either depth format.  Two launches of the feature stage (k_depth_clear at its head,
 * k_depth_register directly in front of the feature gather) build the registered fp32 plane the tracker samples; a handle or sequence that never sets a
 * camera launches exactly what it did before, and NULL returns a handle to that path.
 *  The definition -- fp32 throughout, one IEEE operation per written operation.  K_c, k1 k2 p1 p2 k3, W, H are the sequence's own lvt_amd_params; the
 *  registered plane lives on the raw, distorted colour pixel grid (where the feature gather samples it).  For depth pixel (i, j), column i, row j:
 *   1. z = the fp32 element, or (float)raw16 * depth_scale.  Skipped unless z is finite and > 0.
 *   2. proj(a, b):  X = ((a - cx_d) / fx_d) * z,  Y = ((b - cy_d) / fy_d) * z;  Xc = (R00 X + R01 Y) + R02 z + t0, likewise Yc, Zc, left to right;
 *      x = Xc / Zc, y = Yc / Zc;  r2 = x x + y y;  rad = 1 + r2 (k1 + r2 (k2 + r2 k3));  xd = x rad + (2 p1 x y + p2 (r2 + 2 x x));
 *      yd = y rad + (p1 (r2 + 2 y y) + 2 p2 x y);  u = xd fx + cx,  v = yd fy + cy.
 *   3. (u0, v0) = proj(i - 0.5, j - 0.5), (u1, v1) = proj(i + 0.5, j + 0.5), Zc of proj(i, j).  Skipped unless that Zc is finite and > 0 and u0, v0, u1, v1
 *      are finite with magnitude < 1e6.
 *   4. the footprint is the pixel centres of the half-open box (the top-left rule): x0 = ceil(u0), x1 = ceil(u1) - 1, y0 = ceil(v0), y1 = ceil(v1) - 1;
 *      skipped when x1 - x0 >= 16 or y1 - y0 >= 16 (a calibration error); then clipped to [0, W-1] x [0, H-1].
 *   5. every covered pixel takes min(current, Zc); the plane starts at +inf, and a pixel nothing lands on stays +inf: beyond every far plane, filtered like
 *      any other out-of-range depth.  No hole filling, no smoothing.
 *  - n_rows / n_cols stay the GRAY image's.  Host depth buffers are tightly packed at the camera's size; page-locked ones are read in place as before.
 *  - device depth planes: a pitch of at least cam.width elements; pointer and pitch aligned to the element, as before.
 *  - refused (-1, nothing changed, the reason in lvt_amd_last_error): a stereo handle, a pooled or automatic seat, seq out of range, the batch call on a handle
 *    that is not a batch and the other way round, a handle with frames in flight (set the camera before the first frame or after every frame has been
 *    collected), a bad record -- width or height outside 1 ... 8192, a non-finite field, fx or fy <= 0.  A successful set counts as use of an lvt_create handle.
 *  - lvt_amd_get_depth_camera: 1 = a camera is set (copied to *out), 0 = none, -1 = bad handle / seq.
 *  - lvt_amd_get_plane(h, 0, 4, ...) reads the registered plane of the last frame back (fp32, rows x pitch; 0 bytes on a handle without a camera);
 *    lvt_amd_profile_read reports the launches as "k_depth_clear" and "k_depth_register" (a handle with a camera only).
 *  - lvt_amd_register_depth_device: the stage alone on caller data (device pointers; `colour`: fx fy cx cy, k1 k2 p1 p2 k3, img_width, img_height are read),
 *    for differential tests: d_out, out_pitch_bytes / 4 >= img_width words per row, every word of img_height rows is written.  0 / -1. */
typedef struct lvt_amd_depth_camera {   /* the camera the depth plane is delivered in */
    int   width, height;                 /* of the depth plane, pixels */
    float fx, fy, cx, cy;                /* pinhole, no distortion */
    float R[9], t[3];                    /* row-major; p_colour = R p_depth + t, metres */
} lvt_amd_depth_camera;
LVT_API int lvt_amd_set_depth_camera(lvt_handle h, const lvt_amd_depth_camera *cam);                /* NULL: registered frames again; 0 / -1 */
LVT_API int lvt_amd_batch_set_depth_camera(lvt_handle h, int seq, const lvt_amd_depth_camera *cam);
LVT_API int lvt_amd_get_depth_camera(lvt_handle h, int seq, lvt_amd_depth_camera *out);             /* 1 set, 0 none, -1 bad handle / seq */
LVT_API int lvt_amd_register_depth_device(const lvt_amd_depth_camera *cam, const lvt_amd_params *colour,
                                          const void *d_depth, int depth_pitch_bytes, int depth_format, float depth_scale,
                                          void *d_out /* fp32 */, int out_pitch_bytes, void *hip_stream);

/* DIM frames: CLAHE contrast equalisation inside the tracker's feature stage.  The detector's threshold is fixed; on dim images (EuRoC's dark sequences, a
 * tunnel, lamp light) it finds nothing.  An equalisation record is a property of the handle, or of one sequence of a batch, like the pixel format; the record
 * is copied.  It is not state: lvt_amd_reset, lvt_amd_batch_reset and snapshots neither hold nor change it.  Once it is set, EVERY frame-taking call on that
 * handle or sequence, of either sensor, has the gray plane its detector would read equalised first: two launches at the head of the feature stage
 * (k_clahe_lut: one table per tile; k_clahe_apply: the interpolated gather) write planes the tracker owns, and the frame is tracked from those -- the
 * detector, the descriptor patches and the box sums all see the equalised plane.  Order: convert (pixel format), then remap (rectifiers), then equalise.
 * Opt-in: undimmed frames lose a few per cent of their matches when equalised.  A handle or sequence that never sets a record launches exactly what it did
 * before, and NULL returns a handle to that path.
 *  The definition.  It follows the published algorithm of cv::CLAHE for 8-bit images; the claim is equality with THIS text, not with OpenCV (known
 *  differences below).  Input: the W x H gray plane.  Integer arithmetic where written as integer; where written as fp32, one IEEE operation per written
 *  operation, (float) of an integer rounds to nearest even, rint rounds half to even.
 *   1. Geometry.  Wp = W + ((-W) mod tiles_x), Hp likewise (a dimension that already divides is not padded); tile_w = Wp / tiles_x, tile_h = Hp / tiles_y,
 *      area = tile_w * tile_h.  The padded columns and rows mirror the image without repeating the edge pixel: x >= W reads 2 (W - 1) - x, likewise y
 *      (BORDER_REFLECT_101).
 *   2. Clip level.  c = clip_limit * (float)area / 256.0f (two fp32 operations, left to right).  clip = area if c >= (float)area (compared in fp32, before any
 *      conversion); otherwise clip = max((int)c, 1), truncating.
 *   3. Per tile (tx, ty): hist = the 256-bin histogram of its area padded pixels.  excess = sum of max(hist[i] - clip, 0); every bin is cut to clip;
 *      batch = excess / 256, residual = excess - 256 * batch; every bin gains batch; if residual > 0: step = max(256 / residual, 1) and the bins
 *      0, step, 2 step, ... gain 1 each, stopping at residual of them or at bin 255.  One pass: the redistribution is not iterated.
 *   4. Table.  cum = the inclusive integer prefix sum of hist; lut_scale = 255.0f / (float)area; L[ty][tx][i] = clamp(rint((float)cum[i] * lut_scale), 0, 255).
 *   5. Pixel (x, y) of value v.  fx = (float)x * (1.0f / (float)tile_w) - 0.5f; x1 = floor(fx); xa = fx - (float)x1; xa1 = 1.0f - xa; x2 = x1 + 1; then -- AFTER
 *      xa is taken -- x1 and x2 are clamped to [0, tiles_x - 1].  The same for y.
 *      out = clamp(rint((L[y1][x1][v] * xa1 + L[y1][x2][v] * xa) * ya1 + (L[y2][x1][v] * xa1 + L[y2][x2][v] * xa) * ya), 0, 255), every operation rounded to fp32.
 *  Known differences from cv::CLAHE: OpenCV computes the clip level in double and converts it to int whatever its size; it pads BOTH dimensions by a whole
 *  tile count's remainder as soon as one of them does not divide (a dimension that divides then gains tiles pixels, here it gains none); and its builds may
 *  contract the interpolation's multiply-adds.  None of this has been compared against OpenCV.
 *  - the record: tiles_x, tiles_y each 1 ... 16, tiles_x <= img_width, tiles_y <= img_height; clip_limit finite and > 0.
 *  - external corners are in the same coordinates: lvt_track_with_external_corners stays allowed (a handle with rectifiers still refuses it).
 *  - refused (-1, nothing changed, the reason in lvt_amd_last_error): a pooled or automatic seat, the batch call on a handle that is not a batch and the other
 *    way round, seq out of range, a bad record (the sentence names the field and its limits), a handle with frames in flight (set the record before the
 *    first frame or after every frame has been collected) -- in this order.  A successful set counts as use of an lvt_create handle.
 *  - lvt_amd_get_equalisation: 1 = a record is set (copied to *out), 0 = none, -1 = bad handle / seq.
 *  - lvt_amd_get_plane(h, eye, 5, ...) reads the equalised plane of the last frame back (u8, rows x pitch; 0 bytes on a handle without a record, and when the
 *    last frame went in before the record was set); (h, eye, 6, ...) reads the tables it was made with, tiles_x * tiles_y x 256 bytes, tile (tx, ty) at row
 *    ty * tiles_x + tx.  lvt_amd_profile_read reports the launches as "k_clahe_lut" and "k_clahe_apply" (a handle with a record only).
 *  - lvt_amd_equalise_device: the stage alone on caller planes (device pointers, u8): d_src any address, src_pitch >= w; d_dst 4-byte aligned, dst_pitch a
 *    multiple of 4 and >= w -- every byte of h rows x dst_pitch is written, the columns from w on as zero; w, h 1 ... 8192.  Both launches go to hip_stream; the
 *    call allocates its table buffer and frees it after synchronising that stream.  0 / -1.
 *  - lvt_amd_equalisation_plan: host only, no device needed.  out = {Wp, Hp, tile_w, tile_h, area, clip}, *lut_scale (may be NULL) as in 4.; -1 for a record the
 *    setter would refuse on an image of w x h. */
typedef struct lvt_amd_equalisation {
    int   tiles_x, tiles_y;   /* 1 ... 16 each, and <= the image's width / height */
    float clip_limit;         /* finite, > 0 */
} lvt_amd_equalisation;
LVT_API int lvt_amd_set_equalisation(lvt_handle h, const lvt_amd_equalisation *cfg);                /* NULL: plain frames again; 0 / -1 */
LVT_API int lvt_amd_batch_set_equalisation(lvt_handle h, int seq, const lvt_amd_equalisation *cfg);
LVT_API int lvt_amd_get_equalisation(lvt_handle h, int seq, lvt_amd_equalisation *out);             /* 1 set, 0 none, -1 bad handle / seq */
LVT_API int lvt_amd_equalise_device(const lvt_amd_equalisation *cfg, const void *d_src, int src_pitch, int w, int h, void *d_dst, int dst_pitch,
                                    void *hip_stream);
LVT_API int lvt_amd_equalisation_plan(const lvt_amd_equalisation *cfg, int w, int h, int out[6], float *lut_scale);

/* FEATURE MASKS: key points on masked pixels are dropped inside the tracker's feature stage.  The ego vehicle's bonnet, a robot's own arm, timestamp and logo
 * overlays, the black surround of a rectified wide-angle lens, pixels a segmentation network has labelled movable: all of them give well-textured, strongly
 * matching features that are wrong.  A mask is a property of the handle, or of one sequence of a batch, like the pixel format; masks are NOT offered for pooled
 * and automatic seats.  A handle or sequence that never sets a mask launches exactly what it did.
 *
 * DEFINITION (tests/mask_util.py restates it in numpy; the checks hold the tracker to it bit for bit).  A mask is an 8-bit image of the sequence's
 * img_width x img_height, one per eye, on the pixel grid the detector reads: the rectified grid where rectifiers are attached, otherwise the frame's own grid.
 * A byte != 0 means "key points allowed" (OpenCV's convention).  For every feature the gather step kept, in its output order:
 *     ix = (int)(bx + 0.5f);  iy = (int)(by + 0.5f)          -- fp32 add, then truncation: cv::KeyPointsFilter::runByPixelsMask
 *     keep = 0 <= ix < W && 0 <= iy < H && mask[iy][ix] != 0
 * (bx, by) is the raw pixel BRIEF samples at -- for an RGB-D handle with lens distortion NOT the undistorted (x, y) the feature is reported with.  The kept
 * features stay in order (a stable compaction) and the feature count becomes their number: everything downstream -- BRIEF, the hash cells, row matching, map
 * matching, a LOST frame's kept count, relocalisation -- sees only them.  Consequences:
 *  - ORDERING.  The filter acts after detection, ANMS, the border filter and the RGB-D depth filter, and after the truncation to 4096 features.  The "fewer
 *    than 200 corners" retry is still decided on the unmasked count.  A masked corner may still have suppressed an unmasked neighbour in NMS / ANMS and used some
 *    of its cell's budget: what OpenCV's own mask does with a grid detector.
 *  - An ALL-ZERO mask leaves no features: the frame behaves like a frame without features.
 *  - A mask is a property, not state: lvt_amd_reset and snapshots neither hold nor change it; the snapshot bytes are what they were.
 *  - EXTERNAL corners (lvt_track_with_external_corners) are filtered the same way, in the same coordinates: that is where fractional coordinates meet the
 *    rounding rule (k + 0.5 belongs to pixel k + 1; -0.7 belongs to pixel 0).
 * One launch (k_mask_features, reported under that name by lvt_amd_profile_read for a handle with a mask) between the gather step and BRIEF.
 *
 * CALLS.  lvt_amd_set_mask / lvt_amd_batch_set_mask take tightly packed host buffers (img_width bytes per row); lvt_amd_set_mask_device /
 * lvt_amd_batch_set_mask_device take planes in HBM at any address and any pitch >= img_width.  One eye may be NULL (no mask for that eye); both NULL unsets the
 * property.  The tracker keeps its own copy: the data is copied in the order of the handle's tracking stream -- the caller's stream where lvt_amd_set_stream
 * gave one -- and the copy has completed before the call returns; the caller's buffer is free then.  The mask holds for every later frame until it is set again.
 * Refused under the "Frame properties" contract, in this order, each with -1, the handle as it was and the sentence in lvt_amd_last_error ending in
 * "(nothing was changed)": a bad handle (no report); a pooled or automatic seat; the batch call on a solo handle and the solo call on a batch; seq out of
 * range; a pitch smaller than the width; a right-eye mask on an RGB-D handle; frames in flight.  A successful set counts as a use of an lvt_create handle.
 *  - lvt_amd_get_mask_stats: out = {kept left, dropped left, kept right, dropped right} of the frame lvt_amd_get_counts answers for (an eye without a mask
 *    reports 0, 0).  1 = written; 0 = the sequence has no mask, its last frame went in before the masks it has now were set, or it sat the last collected
 *    step of its batch out; -1 = bad handle / seq.
 *  - lvt_amd_get_plane(h, eye, 7, ...) reads the mask back.
 *  - lvt_amd_mask_features: the stage alone on caller data (host pointers).  The n <= 4096 features' eight arrays are compacted in place against a
 *    width x height mask of `pitch` bytes per row and come back whole; returns the new count, -1 on a refusal (lvt_amd_last_error(NULL)). */
LVT_API int lvt_amd_set_mask(lvt_handle h, const void *left, const void *right);                    /* 0 / -1 */
LVT_API int lvt_amd_batch_set_mask(lvt_handle h, int seq, const void *left, const void *right);
LVT_API int lvt_amd_set_mask_device(lvt_handle h, const void *d_left, int pitch_left, const void *d_right, int pitch_right);
LVT_API int lvt_amd_batch_set_mask_device(lvt_handle h, int seq, const void *d_left, int pitch_left, const void *d_right, int pitch_right);
LVT_API int lvt_amd_get_mask_stats(lvt_handle h, int seq, int out[4]);
LVT_API int lvt_amd_mask_features(int n, float *x, float *y, float *resp, float *bx, float *by, float *depth, int16_t *hcx, int16_t *hcy, const uint8_t *mask,
                                  int width, int height, int pitch);

/* LABEL MASKS: a segmentation image travels with each frame.  A feature mask (above) is a property and needs a quiet handle; a segmentation network delivers
 * a new image every frame, usually at 1/4 or 1/8 of the image's size, as class ids, and is least reliable on object outlines -- where corners sit.  A LABEL MASK
 * record is the property (how a label image becomes a mask); the label images themselves are attached per frame, WITH FRAMES IN FLIGHT, and the tracker builds
 * that frame's mask plane itself: upsampling, the class table and the dilation in one launch.  Not offered for pooled and automatic seats.  A handle or
 * sequence that never sets a record launches exactly what it did.
 *
 * DEFINITION (tests/label_mask_util.py restates it in numpy; pure integer arithmetic, the checks hold the tracker to it bit for bit).  The record is
 *     label_width, label_height  1 ... 8192 each: the size of the label image, independent of the image size (smaller or larger)
 *     drop[256]                  a byte != 0: label l forbids key points
 *     dilate                     0 ... 15, in pixels of the detector's grid
 * For a frame that carries a label image `lab` of that size for an eye, with W, H the sequence's image size and `static` the eye's mask from lvt_amd_set_mask
 * where it has one:
 *     lx(x) = (x * label_width) / W        ly(y) = (y * label_height) / H      -- integer division; the products stay below 2^27
 *     f0(x, y) = drop[lab[ly(y)][lx(x)]] != 0
 *     f(x, y)  = OR of f0(x', y') over |x' - x| <= dilate, |y' - y| <= dilate, 0 <= x' < W, 0 <= y' < H      -- a square window, clipped, never wrapped
 *     m(x, y)  = (!f(x, y) && (no static mask || static[y][x] != 0)) ? 255 : 0
 * m is the plane k_mask_features filters that eye of that frame with, under its unchanged rule (ix = (int)(bx + 0.5f), ...).  Everything FEATURE MASKS states
 * about ordering holds as it stands: the filter acts after detection, ANMS, the border filter, the depth filter and the guard; the retry is decided on the
 * unmasked count; external corners are filtered the same way; labels live on the grid the detector reads, the rectified grid where rectifiers are attached.
 * An eye that got no label image, a frame that got none and a sequence without a record are filtered as before: by the static mask alone, or not at all.
 *
 * THE RECORD.  lvt_amd_set_label_mask / lvt_amd_batch_set_label_mask copy the record; NULL unsets it.  Refused under the "Frame properties" contract with the
 * checks of lvt_amd_set_mask in their order, each with -1, the handle as it was and the sentence in lvt_amd_last_error ending in "(nothing was changed)": a bad
 * handle (no report); a pooled or automatic seat; the batch call on a solo handle and the solo call on a batch; seq out of range; a record outside the ranges
 * above (the sentence names the field and its limits); frames in flight.  The record is not state: lvt_amd_reset and snapshots neither hold nor change it.
 *  - lvt_amd_get_label_mask: 1 = *out written; 0 = the sequence has no record; -1 = bad handle / seq.
 *
 * PER FRAME.  lvt_amd_frame_labels_device takes u8 planes in HBM at any address and any pitch >= label_width; lvt_amd_frame_labels takes tightly packed host
 * buffers (label_width bytes per row).  seq is 0 on a solo handle (the calls have ONE spelling).  Both are accepted with frames in flight.
 *  - BINDING.  The images belong to the NEXT frame submitted for that sequence after the call, whatever entry point submits it (lvt_track,
 *    lvt_track_with_external_corners, lvt_amd_track_async, the device and RGB-D entries, the batch calls), and that frame alone consumes them.  The frame is
 *    named by its number, lvt_amd_get_host_stats' out[0] + 1 at the time of the call: a frame lvt_amd_track_async still holds back has its number already and
 *    can never take the labels meant for the frame behind it.
 *  - A second call before the frame replaces the first; both pointers NULL clears a pending attachment; one eye NULL: that eye gets no labels.
 *    lvt_amd_reset / lvt_amd_batch_reset drop a pending attachment.
 *  - A batch step consumes every sequence's attachment, also that of a sequence that sits the step out (nothing is built for it).
 *  - Device planes are read in place on the feature stream: they must stay valid and unchanged until that frame has been collected (the rule of the device
 *    image entries).  Host buffers are free when the call returns; the call does not wait for the frames in flight -- it copies into a page-locked ring of
 *    8 slots and makes room first, so that the slot's last user (8 frames ago) has been collected.
 *  - Refused with -1, the sentence in lvt_amd_last_error ending in "(nothing was attached)", in this order: a bad handle (no report); a pooled or automatic
 *    seat; seq out of range; a sequence without a record; a pitch below label_width; right-eye labels on an RGB-D handle.
 *
 * READ-BACK.  lvt_amd_get_mask_stats also answers for a frame that was filtered through labels (an eye that was filtered neither way reports 0, 0);
 * lvt_amd_get_plane(h, eye, 8, ...) returns the plane built for the last collected frame (u8, rows x pitch, padding columns zero; 0 bytes where none was
 * built); lvt_amd_profile_read reports the launch as "k_label_mask", only for a handle with a record.
 *  - lvt_amd_build_label_mask: the stage alone on caller data (host pointers).  `labels` is label_height rows of label_pitch >= label_width bytes, the static
 *    mask (or NULL) H rows of static_pitch >= W bytes, `out` H rows of out_pitch bytes (a multiple of 4, >= W) which come back whole -- the padding columns
 *    zero.  0, or -1 on a refusal (lvt_amd_last_error(NULL)) or a HIP failure. */
typedef struct lvt_amd_label_mask {
    int label_width, label_height;
    uint8_t drop[256];
    int dilate;
} lvt_amd_label_mask;
LVT_API int lvt_amd_set_label_mask(lvt_handle h, const lvt_amd_label_mask *cfg);                    /* 0 / -1 */
LVT_API int lvt_amd_batch_set_label_mask(lvt_handle h, int seq, const lvt_amd_label_mask *cfg);
LVT_API int lvt_amd_get_label_mask(lvt_handle h, int seq, lvt_amd_label_mask *out);
LVT_API int lvt_amd_frame_labels(lvt_handle h, int seq, const void *left, const void *right);      /* 0 / -1 */
LVT_API int lvt_amd_frame_labels_device(lvt_handle h, int seq, const void *d_left, int pitch_left, const void *d_right, int pitch_right);
LVT_API int lvt_amd_build_label_mask(const lvt_amd_label_mask *cfg, const uint8_t *labels, int label_pitch, int W, int H, const uint8_t *static_or_NULL,
                                     int static_pitch, uint8_t *out, int out_pitch);

/* DEPTH GUARD: RGB-D key points whose depth has no support around it are dropped inside the tracker's feature stage.  A key point's depth is ONE pixel of the
 * depth plane, depth[(int)y][(int)x] (the reference does the same), and corners cluster where that sample is worst: on occlusion boundaries, where the corner a
 * foreground edge makes with background texture is no 3-D point; on the flying pixels a time-of-flight or structured-light sensor delivers between foreground and
 * background; on lone valid pixels inside holes.  A guard is a property of an RGB-D handle, or of one sequence of an RGB-D batch, like the depth camera; it is
 * NOT offered for pooled and automatic seats, and a stereo handle is refused.  A handle or sequence that never sets a guard launches exactly what it did.
 *
 * DEFINITION (tests/depth_guard_util.py restates it in numpy; the checks hold the tracker to it bit for bit).  The record is
 *     radius 1 ... 3;  min_support 1 ... (2 * radius + 1)^2 - 1;  tol_abs, tol_rel finite and >= 0 (metres, and a share of the depth)
 * and lvt_amd_depth_guard_default gives {1, 4, 0.01f, 0.02f}.  The plane is the one the gather step sampled, with its pitch, format and scale: the registered
 * fp32 plane where a depth camera is set, the 16-bit plane with its scale where the frame came in as LVT_AMD_DEPTH_U16.  A pixel's sample s is what the gather
 * step would have read there: the value itself (fp32), or (float)raw * scale in ONE rounded fp32 multiply (16-bit).  A sample is VALID when
 * near_plane <= s && s <= far_plane; a NaN is not valid.  For every feature the gather step kept, in its output order, with (bx, by) the raw position BRIEF
 * samples at:
 *     cx = (int)bx;  cy = (int)by                  -- truncation, the gather step's own pixel; inside the plane when bx > -1 && bx < W && by > -1 && by < H
 *     d_c = s(cx, cy);  the feature is dropped when the pixel is outside the plane or d_c is not valid
 *     t = tol_abs + tol_rel * d_c                  -- two rounded fp32 operations, the product first; no fused multiply-add
 *     support = the number of (dx, dy) != (0, 0) with |dx|, |dy| <= radius and (cx + dx, cy + dy) inside the plane whose sample s is valid and has
 *               fabsf(s - d_c) <= t                -- one rounded fp32 subtraction
 *     keep = support >= min_support
 * The kept features stay in order (a stable compaction) and the feature count becomes their number; the depth a kept feature reports stays the centre sample.
 * Consequences:
 *  - ORDERING.  The guard acts after detection, ANMS, the border filter and the depth-range filter, and after the truncation to 4096 features; it acts BEFORE the
 *    feature mask, whose statistics count what the guard left.  The "fewer than 200 corners" retry is decided as before, on the detector's count.
 *  - The window is clipped at the plane's border: a key point near it has fewer neighbours to draw support from, never an implied one.
 *  - In a registered plane a pixel nothing landed on (+inf) is simply not valid.
 *  - FRACTIONAL positions are guarded at their truncated pixel, the gather step's own.  The tracker never meets one: lvt_track_with_external_corners is a stereo
 *    entry (as in the reference) and a stereo handle has no guard; lvt_amd_depth_guard_features takes positions of any bit pattern.
 *  - A guard is a property, not state: lvt_amd_reset and snapshots neither hold nor change it; the snapshot bytes are what they were.
 *  - EQUIVALENCE.  Detected corners are integers, so a guarded frame equals the unguarded tracker fed the plane where(keep, depth, 0), keep being the rule above
 *    evaluated at every pixel: a zero fails the depth-range test of the gather step exactly where the guard would have dropped the key point, and the retry does
 *    not look at depth.  This ends at the truncation: in a frame with more than 4096 key points behind the depth-range test (reported as a capacity overflow) the
 *    guard thins the first 4096, while the zeroed plane lets later ones move up.  Lens distortion is covered: the gather step and the guard read the same
 *    raw pixel, whatever (x, y) the feature is reported with.
 * One launch (k_depth_guard, reported under that name by lvt_amd_profile_read for a handle with a guard) directly behind the gather step.
 *
 * CALLS.  lvt_amd_set_depth_guard / lvt_amd_batch_set_depth_guard copy the record; NULL unsets the property.  Refused under the "Frame properties" contract, in
 * this order, each with -1, the handle as it was and the sentence in lvt_amd_last_error ending in "(nothing was changed)": a bad handle (no report); a pooled or
 * automatic seat; a stereo handle; the batch call on a solo handle and the solo call on a batch; seq out of range; a record outside the ranges above (the
 * sentence names the field and its limits); frames in flight.
 *  - lvt_amd_get_depth_guard: 1 = *out written; 0 = the sequence has no guard; -1 = bad handle / seq.
 *  - lvt_amd_get_depth_guard_stats: out = {kept, dropped} of the frame lvt_amd_get_counts answers for.  1 = written; 0 = the sequence has no guard, its last
 *    frame went in before the record it has now was set, or it sat the last collected step of its batch out; -1 = bad handle / seq.
 *  - lvt_amd_depth_guard_features: the stage alone on caller data (host pointers).  The n <= 4096 features' eight arrays are compacted in place against a
 *    width x height depth plane of `pitch_elems` elements per row (depth_format LVT_AMD_DEPTH_F32 / _U16, depth_scale for the latter) and come back whole;
 *    returns the new count, -1 on a refusal (lvt_amd_last_error(NULL)). */
typedef struct { int radius; int min_support; float tol_abs; float tol_rel; } lvt_amd_depth_guard;
LVT_API void lvt_amd_depth_guard_default(lvt_amd_depth_guard *out);
LVT_API int lvt_amd_set_depth_guard(lvt_handle h, const lvt_amd_depth_guard *cfg);                  /* 0 / -1 */
LVT_API int lvt_amd_batch_set_depth_guard(lvt_handle h, int seq, const lvt_amd_depth_guard *cfg);
LVT_API int lvt_amd_get_depth_guard(lvt_handle h, int seq, lvt_amd_depth_guard *out);
LVT_API int lvt_amd_get_depth_guard_stats(lvt_handle h, int seq, int out[2]);
LVT_API int lvt_amd_depth_guard_features(int n, float *x, float *y, float *resp, float *bx, float *by, float *depth_of, int16_t *hcx, int16_t *hcy,
                                         const void *depth, int depth_format, float depth_scale, int width, int height, int pitch_elems, float near_plane,
                                         float far_plane, const lvt_amd_depth_guard *cfg);

/* ---- SNAPSHOTS: one sequence's state saved, restored, moved between handles and seats -------------------------------------------------
 * A tracker's state lives in HBM: its control record, the local map, the staged points and the motion model.  A snapshot is a copy of it, device-resident and
 * owned by the library: ONE contiguous allocation (header | control record | the live map and staged arrays, the first map_n / staged_n points in storage
 * order), gathered by one kernel launch (k_state_pack) and scattered back by one (k_state_unpack).  Its exported form is the same bytes, headed by magic,
 * version, the sizes and capacities of the build, sensor type, the sequence's lvt_amd_params, point counts, section offsets, total size and a 64-bit checksum
 * of everything behind the header.  The words of the control record that belong to a launch chain, not to the tracker (stream hand-over sequence numbers, gate
 * counters, debug stamps), are zero in a snapshot: two snapshots of one state export identical bytes whatever route the frames took, and a snapshot taken
 * right after an apply exports the bytes that were applied.  `seq` is 0 for a solo handle.
 *  - take: drains the handle as the introspection calls do; the snapshot is the state after the last frame enqueued; the source is untouched and goes on
 *    tracking.  Allowed in every state: NOT_INITIALIZED (an empty map), TRACKING, LOST.  The batch call takes every sequence with ONE drain and ONE launch
 *    (16 sequences per launch), out[s] = sequence s.
 *  - apply: replaces the WHOLE state of the target sequence; the next frame handed in continues the snapshot's trajectory as if the source had tracked it, bit
 *    for bit.  lvt_amd_get_pose, lvt_amd_get_counts, lvt_get_status, lvt_amd_get_map, lvt_amd_get_staged and lvt_amd_batch_get_counts answer from the snapshot
 *    as soon as apply returns.  The other per-frame read-backs (features, matches, row matches, planes) stay those of the TARGET's own last frame -- their
 *    buffers are per-frame scratch, not state -- and speak of the snapshot's trajectory from the next frame on.  A snapshot may be applied any number of times
 *    (a clone) and stays valid until it is destroyed.  The batch call applies s[i] to sequence i, NULL = leave alone.  A successful apply counts as use of an
 *    lvt_create handle.
 *  - export / import: the route to a file, another process or another device.  export copies the blob to host memory and writes the checksum (the bytes
 *    written, -1: cap is too small; lvt_amd_snapshot_get_info says how many are needed); import checks the bytes and uploads them to `device`
 *    (-1: the current one).  lvt_amd_snapshot_describe does the checks alone: host code, no GPU needed.
 *  - lvt_amd_batch_reset: lvt_system::reset for ONE sequence of a lock-step batch (lvt_amd_reset on a batch handle resets them all); drains first.
 *  - refused (-1 or NULL, nothing changed, the reason in lvt_amd_last_error; a batch names the sequence): seq out of range (a solo handle: seq != 0); a batch
 *    call on a solo handle; apply of a snapshot whose lvt_amd_params differ from the target sequence's (compared byte for byte, as the pool compares them), of
 *    another sensor type, or living on another device (between devices: export, then import); apply with frames in flight (apply after every frame has been
 *    collected); pooled and automatic seats, both ways; import or describe of bytes that are too short or have a wrong magic, version, recorded record size,
 *    capacities, section offsets or checksum -- those two have no handle: lvt_amd_last_error(NULL) gives the reason of the calling thread's last refusal.
 *  - out of scope: pooled and automatic seats (moving a tracked handle into the pool needs the pool's quiesce and its per-seat host records); a reset or
 *    restore without draining the pipeline; applying across different parameters or capacities.
 *  - lvt_amd_profile_read reports the launches as "k_state_pack" / "k_state_unpack" (time between HIP events on the handle's stream). */
typedef void *lvt_amd_snapshot;            /* one sequence's state, device-resident, owned by the library */
typedef struct lvt_amd_snapshot_info {     /* all int / long long, no padding surprises */
    int version, sensor_type, state, frame_number, map_n, staged_n, src_map_cur, src_staged_cur, device;   /* device: -1 from lvt_amd_snapshot_describe */
    long long bytes;                       /* size of the exported form */
} lvt_amd_snapshot_info;
LVT_API lvt_amd_snapshot lvt_amd_snapshot_take(lvt_handle h, int seq);                         /* NULL on refusal */
LVT_API int lvt_amd_snapshot_apply(lvt_handle h, int seq, lvt_amd_snapshot s);                 /* 0 / -1 */
LVT_API int lvt_amd_batch_snapshot_take(lvt_handle h, lvt_amd_snapshot *out /* [B] */);        /* 0 / -1 */
LVT_API int lvt_amd_batch_snapshot_apply(lvt_handle h, const lvt_amd_snapshot *s /* [B], NULL = leave alone */);
LVT_API int lvt_amd_snapshot_get_info(lvt_amd_snapshot s, lvt_amd_snapshot_info *out);         /* 0 / -1 */
LVT_API int lvt_amd_snapshot_get_params(lvt_amd_snapshot s, lvt_amd_params *out);              /* 0 / -1 */
LVT_API long long lvt_amd_snapshot_export(lvt_amd_snapshot s, void *host_buf, long long cap);  /* bytes written, -1 */
LVT_API lvt_amd_snapshot lvt_amd_snapshot_import(const void *bytes, long long n, int device /* -1: current */);
LVT_API int lvt_amd_snapshot_describe(const void *bytes, long long n, lvt_amd_snapshot_info *out, lvt_amd_params *p);  /* 0 / -1 */
LVT_API void lvt_amd_snapshot_destroy(lvt_amd_snapshot s);
LVT_API int lvt_amd_batch_reset(lvt_handle h, int seq);                                        /* 0 / -1 */

/* ---- POSE UNCERTAINTY: a per-frame 6x6 covariance from the solver's edges -----------------------------------------------------------------
 * The reference publishes its odometry with both covariance blocks at zero (lvt_ros.cpp:268-299).  A handle that asks for it gets, per frame and per
 * sequence, the information matrix of the frame's 2D-3D edges at the PUBLISHED pose and its inverse.  Opt-in: one launch of its own (k_pose_info, one
 * workgroup per sequence, on the tracking stream directly behind k_pnp); a handle that never asks launches exactly what it did.
 *  Pose convention.  Pose (R, p) is camera-to-world, as lvt_track returns it.  The perturbation is xi = (dp, dtheta): p <- p + dp in metres on world axes,
 *    R <- R Exp([dtheta]x) in radians on camera axes -- the pose solver's own parametrisation (t += dx[0..2], q <- q (sqrt(1 - |v|^2), v)) with dtheta = 2 v.
 *  Edge quantities.  For edge i with its map point X and its observation (u, v) -- what lvt_amd_get_matches / lvt_amd_get_features(0) return for the frame:
 *    pc = R^T (X - p);  e = (fx pcx / pcz + cx - u, fy pcy / pcz + cy - v);
 *    the edge is an INLIER iff pcz > 0 and e.e <= 5.991, with comparisons false for NaN;
 *    weight w = 1 / (1 + e.e / 5.991): the Cauchy kernel of the solver, rho' only, no second-order term;  J = de/dxi, 2 x 6.
 *  Outputs.  info = sum over inliers of w J^T J;  cov = info^-1.  Both 6 x 6, row-major, in the order (px, py, pz, thetax, thetay, thetaz) and exactly symmetric.
 *    Unit pixel noise: cov is NOT scaled by the residual -- chi2, sq_err and n_inliers are what a caller needs to scale it.
 *  status: 0 = none (not enabled, first frame, LOST at or before this frame, skipped or absent frame, or just reset / restored); 1 = valid;
 *    2 = degenerate: n_inliers < 3, or an LDL^T pivot d_k <= 1e-12 info[k][k] (a sum of <= 4096 fp64 terms carries that much relative noise: a pivot below it
 *    is not information) -- info is still delivered, cov is all zero.
 *  - lvt_amd_enable_pose_info: a property of the handle, all sequences of a batch together; 0 / -1.  Refused (-1, nothing changed, the reason in
 *    lvt_amd_last_error): frames in flight (enable before the first frame or after every frame has been collected), a pooled or automatic seat, a bad handle.
 *    A successful call counts as use of an lvt_create handle.  Enabling is not state: it is neither in snapshots nor restored by them.
 *  - lvt_amd_get_pose_info: the record of the frame lvt_amd_get_pose / lvt_amd_get_counts answer for, waiting where they wait (`seq` is 0 for a solo handle).
 *    1 = record copied, 0 = not enabled (the record is zero-filled), -1 = bad handle or seq.  lvt_amd_reset, lvt_amd_batch_reset and lvt_amd_snapshot_apply
 *    leave status 0 until the next tracked frame.
 *  - lvt_amd_pose_info_eval: the same evaluation on caller data (host pointers: pts n x 3 f64, obs n x 2 f32, 0 <= n <= 4096; q unit, either sign),
 *    for differential tests; 0 / -1.
 *  - lvt_amd_pose_info_to_ros: host only.  cov with its rotation part on FIXED WORLD axes (dphi = R dtheta), i.e. M cov M^T with M = blockdiag(I, R): the
 *    convention of geometry_msgs/PoseWithCovariance for the camera pose itself.  (The odometry accumulator below has its own, for base_link in odom.)
 *  - lvt_amd_profile_read reports the launch as "k_pose_info" (an enabled handle only). */
typedef struct lvt_amd_pose_info {
    double cov[36], info[36];
    double chi2;        /* sum of 5.991 log(1 + e.e / 5.991) over inliers */
    double sq_err;      /* sum of e.e over inliers */
    int n_edges, n_inliers;
    int n_borderline;   /* edges with |e.e - 5.991| < 1e-6 */
    int status;
    int frame;          /* LVT_AMD_C_FRAME of the frame the record belongs to */
    int reserved;
} lvt_amd_pose_info;
#define LVT_AMD_POSE_INFO_SIZE 616
#ifdef __cplusplus
static_assert(sizeof(lvt_amd_pose_info) == LVT_AMD_POSE_INFO_SIZE, "lvt_amd_pose_info is part of the ABI");
#else
_Static_assert(sizeof(lvt_amd_pose_info) == LVT_AMD_POSE_INFO_SIZE, "lvt_amd_pose_info is part of the ABI");
#endif
LVT_API int lvt_amd_enable_pose_info(lvt_handle h, int enable);                               /* 0 / -1 */
LVT_API int lvt_amd_get_pose_info(lvt_handle h, int seq, lvt_amd_pose_info *out);             /* 1 / 0 / -1 */
LVT_API int lvt_amd_pose_info_eval(const lvt_amd_params *p, const double q_wxyz[4], const double pos[3], const double *pts, const float *obs, int n,
                                   lvt_amd_pose_info *out);
LVT_API void lvt_amd_pose_info_to_ros(const double cov[36], const double R[3][3], double cov_ros[36]);

/* ---- RELOCALISATION: recover a LOST tracker against its kept map ------------------------------------------------------------------------------
 * The tracker latches LOST at its first frame with fewer than min_num_matches_for_tracking matches and returns the last pose from then on; the reference's
 * only way out is a reset, which throws the map away.  But a LOST tracker keeps its map, and the feature stage goes on running.  lvt_amd_relocalise is an
 * explicit call BETWEEN frames on a quiet handle, modelled on lvt_amd_snapshot_apply: it searches the kept map for the last frame handed in -- the frame
 * lvt_amd_get_features answers for -- with no pose prior, decides whether the result is good enough, and commits the new state; the next frame tracks on
 * from it in the old map's coordinates.  Any state is accepted (TRACKING, or LOST after any number of frames) as long as the map holds a point; a snapshot
 * applied in a later session followed by a relocalisation on the first frame continues in the snapshot's coordinates.  Nothing in the per-frame launch
 * chain changes: a handle that never calls it allocates and launches exactly what it did, and snapshots keep their bytes.
 * The stages are entry points of their own as well, in the style of lvt_amd_hamming_match_batched and lvt_amd_pnp: the global descriptor match (stage 1),
 * the correspondences (stage 2) on features and a map the caller hands in, and hypotheses, scoring and refinement (stages 3 - 5) on correspondences the
 * caller has formed.  The claim is equality with THIS text; tests/reloc_util.py restates it in numpy.
 *  Arithmetic.  The 32-bit floats of the observations and the parameters are widened to fp64, everything after that is fp64: one IEEE operation per written
 *  operation, correctly rounded division and square root, only + - * / sqrt, sums of three in the order ((a b + c d) + e f).  A comparison that involves a NaN
 *  is false.
 *   1. Global match.  For every query descriptor i < n_query the two nearest of ALL n_map map descriptors by Hamming distance, ties to the lowest map index
 *      (cv::BFMatcher::knnMatch with k = 2 and no mask).  No position predicate.  The record is (idx1, d1, idx2, d2), -1 / INT_MAX where there is none.
 *      On a handle: the queries are the N left features of the last frame, the map the M = map_n points of the live copy (both read on the device, M clamped
 *      to the capacity).  A feature is ACCEPTED by the tracker's own rule with cnt = min(M, 2): d1 / d2 < tracking_ratio_test_threshold in fp32 (so 0 / 0
 *      fails) for cnt = 2, d1 <= descriptor_matching_threshold for cnt = 1.  n_matched counts the accepted features.
 *   2. Correspondences.  A map point claimed by several accepted features keeps the one with the smallest (d1, i).  The survivors, ordered by feature index,
 *      are the correspondences c = 0 ... n_corr - 1: the map point's position X, the feature's (u, v) = its stored coordinates (undistorted for RGB-D) and a
 *      camera-frame point Pc, or none.
 *        RGB-D: Z = the depth the feature stage kept for the feature (inside the near and far planes).
 *        Stereo: the partner among the right features j with (float)max((int)y_l - 2, 0) <= y_r <= (float)min((int)y_l + 2, img_height) and
 *          x_l - x_r >= min_disparity in fp32: the top two by Hamming distance (ties to the lowest j), accepted by the tracker's rule with
 *          triangulation_ratio_test_threshold and cnt = min(candidates, 2).  No exclusivity between left features: this is a hypothesis generator, not the
 *          row matcher.  Z = (fx baseline) / (x_l - x_r).
 *        Pc = (((x - cx) Z) / fx, ((y - cy) Z) / fy, Z).
 *      The correspondences with a point, in order, are numbered 0 ... n3 - 1 (n_with_point).  n3 < 3: status 1.
 *      (The stage entry lvt_amd_reloc_solve takes the caller's correspondences: X, (u, v), Pc and has_pc.)
 *   3. Hypotheses.  For h = 0 ... n_hypotheses - 1 and j = 0, 1, 2:  x = seed + (3 h + j + 1) 0x9E3779B97F4A7C15 mod 2^64, then the splitmix64 finaliser
 *      x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27, x *= 0x94D049BB133111EB, x ^= x >> 31; sample j is number (x mod n3) of the correspondences with a
 *      point.  With a_k = Pc and b_k = X of the three samples, the triad of either set is
 *          d = p1 - p0, n1 = (dx dx + dy dy) + dz dz, e1 = d / sqrt(n1);   c = e1 x (p2 - p0), n3 = (cx cx + cy cy) + cz cz, e3 = c / sqrt(n3);   e2 = e3 x e1
 *      with (a x b) = (ay bz - az by, az bx - ax bz, ax by - ay bx), and
 *          R[i][j] = (e1b[i] e1a[j] + e2b[i] e2a[j]) + e3b[i] e3a[j]      (camera to world)
 *          mean(p) = ((p0 + p1) + p2) / 3,     t[i] = mean(b)[i] - ((R[i][0] ma[0] + R[i][1] ma[1]) + R[i][2] ma[2])
 *      A hypothesis scores 0 when two of its samples coincide, or when n1 <= 1e-12 or n3 <= 1e-12 in either set.
 *   4. Score.  For EVERY correspondence, with or without a Pc:  dx = X - t;  pc[j] = (R[0][j] dx[0] + R[1][j] dx[1]) + R[2][j] dx[2];
 *          e = ((fx pcx) / pcz + cx - u, (fy pcy) / pcz + cy - v);   an inlier iff pcz > 0 and ex ex + ey ey <= gate_px2.
 *      The best hypothesis has the largest count, ties to the lowest h.  A count below the success count max(min_inliers, min_num_matches_for_tracking):
 *      status 2.
 *   5. Refine.  The inliers of the best hypothesis, in correspondence order, are the edges; the start pose is (quaternion of R, t), the quaternion by the
 *      branch on the trace / largest diagonal element the odometry accumulator uses.  The solver is the pose refinement of the frame path, the code behind
 *      lvt_amd_pnp.  n_refined_inliers is what LVT_AMD_C_PNP_INLIERS counts for a frame; below the success count, or a pose that is not finite: status 3.
 *   6. Commit (status 0, and not dry_run).  The sequence's control record becomes its own with: state TRACKING; the last and the optimised pose = the refined
 *      pose, the returned R, t and status to match; the motion model at rest at that pose (last pose = it, angular velocity the identity quaternion, linear
 *      velocity 0, nothing pending); last_matches = {n, n, n} with n = n_refined_inliers; no early-stream work carried (the first frame afterwards is matched
 *      entirely on the tracking stream); the stream hand-over words of a just-reset record, as a snapshot apply writes them.  The frame number, the map with its
 *      counters and ages and the staged set stay as they were.  lvt_get_status, lvt_amd_get_pose, lvt_amd_get_last_pose and lvt_amd_get_counts answer from the
 *      new state at once; the pose-uncertainty record has status 0 until the next tracked frame.  On status 1 ... 3 and on every dry_run not one byte of the
 *      sequence's state changes; lvt_amd_get_matches still answers for the last frame either way (the solver runs on buffers of the call's own).
 *  - lvt_amd_relocalise / lvt_amd_batch_relocalise (one sequence of a uniform or mixed batch; its neighbours are untouched): 0 for status 0, 1 for status
 *    1 ... 3 (nothing was changed), -1 for a refusal: the complete sentence is in lvt_amd_last_error and ends in "(nothing was changed)".  Refused, in this
 *    order: a bad handle; a pooled or automatic seat; the batch call on a solo handle and the reverse; seq out of range; a bad config field; frames in flight
 *    (collect every frame first); a handle that has not seen a frame; an empty map; a last frame that was skipped, absent or poisoned (it has no features).
 *    A HIP failure inside the call is outside that contract: -1, the HIP error's text in lvt_amd_last_error, `out` unwritten.
 *    Seven launches and the commit on the handle's tracking stream, ONE stream synchronisation, one read-back of the result record; the buffers are allocated
 *    by the first call.
 *  - lvt_amd_reloc_config: n_hypotheses 1 ... 1024; gate_px2 and min_disparity finite and > 0; min_inliers >= 3; dry_run 0 or 1.  A field out of range is
 *    refused (-1, the sentence names the field and ends in "(nothing was changed)"; these calls have no handle: lvt_amd_last_error(NULL) has it).
 *    lvt_amd_reloc_solve checks min_disparity and dry_run and does not use them.
 *  - lvt_amd_reloc_result: status 0 = a pose, 1 = fewer than 3 correspondences with a camera-frame point, 2 = the best hypothesis is below the success count,
 *    3 = the refined pose is not finite or its inliers fall below the success count.  The pose (camera-to-world, as lvt_track returns it) is filled for status
 *    0 and 3 and zero otherwise.  n_features, n_map and n_matched belong to a handle's call; the stage entry leaves them zero.
 *  - lvt_amd_reloc_match_device: stage 1 on DEVICE pointers aligned to 16 bytes: d_query n_query x 32 bytes, d_map n_map x 32 bytes, d_out n_query x 4 int32;
 *    n_query 0 ... 4096, n_map 0 ... 32768.  The map is cut into slices of lvt_amd_reloc_slice_length(n_map) points (32 ... 1024, about 32 slices), a
 *    workgroup holds one slice in LDS.  Two launches on hip_stream; the call allocates its key buffer and frees it once that stream has run them.  Returns
 *    the time between HIP events around the launches in microseconds, < 0 on a refusal or failure.  Environment, read by this entry alone: LVT_AMD_RELOC_MATCH=uniform
 *    runs the variant that loads the slice's descriptors straight from memory at a wave-uniform address instead of staging them in LDS (same records; for
 *    measurements, profiles/relocalisation.md).
 *  - lvt_amd_reloc_solve: stages 3 - 5 on HOST pointers: pts n x 3 f64, obs n x 2 f32, pc n x 3 f64, has_pc n bytes, 0 <= n <= 4096; of `p` the intrinsics
 *    and min_num_matches_for_tracking are read.  counts_out (n_hypotheses ints), inliers_out (n ints; the first n_hyp_inliers are written), hyp_R (9,
 *    row-major) and hyp_t (3) -- the best hypothesis, status 0 and 3 only -- may each be NULL.  Returns 0 for status 0, 1 for status 1 ... 3, -1 on a refusal.
 *  - lvt_amd_reloc_correspond: stage 2, behind stage 1, on HOST pointers, through the very launches a handle's call makes for them (the capacity grid, every
 *    size read on the device).  The call lays the data out as a handle holds it, in device buffers of its own, and synchronises once.
 *      sensor 1 (stereo) or 2 (RGB-D).  Of `p`: img_height, fx, fy, cx, cy, baseline, tracking_ratio_test_threshold, triangulation_ratio_test_threshold and
 *      descriptor_matching_threshold; of the config: min_disparity (the other fields are checked and not used).
 *      Left features: x, y (f32), desc (32 bytes each), depth (f32, RGB-D only), 0 <= n_left <= 4096.  Right features: the same without depth,
 *      0 <= n_right <= 4096; RGB-D ignores them.  The map: map_pos n_map x 3 f64, map_desc n_map x 32 bytes, 0 <= n_map <= 32768.
 *      map_copy 0 or 1: the copy of the two the map is placed in and the live-copy word names; the OTHER copy gets other_pos / other_desc (n_map rows each;
 *      NULL: zeros), which a correct call never reads.
 *      lost_frame 0 or 1.  1: the counts arrive as a LOST frame leaves them -- the feature counts themselves are zero, the counts are the ones the frame's
 *      epilogue kept beside them, marked as belonging to the frame the buffer holds.
 *      Out: n_features, n_map, n_matched, n_corr, n_with_point and status of `out` (1 for n_with_point < 3, otherwise -1: stages 3 - 5 have not run; the
 *      other fields zero).  Per correspondence c < n_corr: corr_feat[c] the feature index, X[3 c ..] , uv[2 c ..], has_pc[c], and -- where has_pc[c] -- Pc[3 c ..];
 *      with_pc[k], k < n_with_point.  Each array has room for 4096 elements (rows).  They are uploaded as the caller filled them and read back whole: an
 *      element beyond the counts, and a Pc row without a point, comes back with the caller's bytes.  claims_left (may be NULL): how many entries of the
 *      mutual filter's claim table are not empty behind the call (a call leaves the table as it found it: 0).
 *      Returns 0, or -1 on a refusal: a NULL argument, a count or a flag out of range, a bad config field, parameters lvt_amd_create would refuse. */
typedef struct lvt_amd_reloc_config {
    int      n_hypotheses;    /* 256 */
    float    gate_px2;        /* 16.0: the scoring gate in px^2 */
    float    min_disparity;   /* 1.0 */
    int      min_inliers;     /* 30 */
    uint64_t seed;            /* 0 */
    int      dry_run;         /* 0 */
    int      reserved;
} lvt_amd_reloc_config;
typedef struct lvt_amd_reloc_result {
    int status;
    int n_features, n_map, n_matched, n_corr, n_with_point;
    int best_hypothesis, n_hyp_inliers, n_refined_inliers;
    int reserved;
    double q_wxyz[4], p[3];
    double R[3][3], t[3];
} lvt_amd_reloc_result;
#define LVT_AMD_RELOC_CONFIG_SIZE 32
#define LVT_AMD_RELOC_RESULT_SIZE 192
#ifdef __cplusplus
static_assert(sizeof(lvt_amd_reloc_config) == LVT_AMD_RELOC_CONFIG_SIZE && sizeof(lvt_amd_reloc_result) == LVT_AMD_RELOC_RESULT_SIZE,
              "the relocalisation records are part of the ABI");
#else
_Static_assert(sizeof(lvt_amd_reloc_config) == LVT_AMD_RELOC_CONFIG_SIZE && sizeof(lvt_amd_reloc_result) == LVT_AMD_RELOC_RESULT_SIZE,
               "the relocalisation records are part of the ABI");
#endif
LVT_API int lvt_amd_relocalise(lvt_handle h, const lvt_amd_reloc_config *cfg /* NULL = defaults */, lvt_amd_reloc_result *out);
LVT_API int lvt_amd_batch_relocalise(lvt_handle h, int seq, const lvt_amd_reloc_config *cfg, lvt_amd_reloc_result *out);
LVT_API void lvt_amd_reloc_default_config(lvt_amd_reloc_config *cfg);
LVT_API int lvt_amd_reloc_slice_length(int n_map);
LVT_API float lvt_amd_reloc_match_device(const void *d_query, int n_query, const void *d_map, int n_map, void *d_out, void *hip_stream);
LVT_API int lvt_amd_reloc_solve(const lvt_amd_params *p, const lvt_amd_reloc_config *cfg /* NULL = defaults */, const double *pts, const float *obs,
                                const double *pc, const uint8_t *has_pc, int n, int *counts_out, int *inliers_out, double *hyp_R, double *hyp_t,
                                lvt_amd_reloc_result *out);
LVT_API int lvt_amd_reloc_correspond(const lvt_amd_params *p, const lvt_amd_reloc_config *cfg /* NULL = defaults */, int sensor, const float *xl, const float *yl,
                                     const uint8_t *desc_l, const float *depth_l, int n_left, const float *xr, const float *yr, const uint8_t *desc_r, int n_right,
                                     const double *map_pos, const uint8_t *map_desc, const double *other_pos, const uint8_t *other_desc, int n_map, int map_copy,
                                     int lost_frame, lvt_amd_reloc_result *out, int *corr_feat, double *X, float *uv, uint8_t *has_pc, double *Pc, int *with_pc,
                                     int *claims_left);

/* ---- odometry accumulator: the consumer right behind the path -----------------------------------------------
 * What the reference's ROS node does with every pose (lvt/src/lvt_ros.cpp:86-92 constructor, :215-311 on_stereo_image), without
 * ROS: poses are re-expressed in an x-forward / z-up frame (rot_fix = Rz(-pi/2) Rx(-pi/2)), the frame-to-frame delta is moved
 * into the base frame (base_to_sensor, identity by default) and accumulated into base_to_odom; a frame with an older time stamp
 * is ignored; when tracking is LOST the odometry resets the tracker (lvt_system::reset) and -- if reset_pose_on_lost -- its own
 * accumulated pose, and publishes nothing for that frame.
 *   pose_out  : position x y z + orientation qx qy qz qw of the base in the odom frame
 *   twist_out : linear xyz, angular xyz (delta / time since the previous published frame; zeros for the first frame or dt = 0)
 * lvt_amd_odometry_push_pose is the pure host-side step (a pose that was tracked elsewhere; `h` may be NULL at creation);
 * lvt_amd_odometry_update = lvt_track + lvt_get_status + that step (+ the reset on LOST).
 * Return value of both: 1 = published, 0 = nothing published (LOST and reset, or stale time stamp), -1 = bad arguments. */
typedef void *lvt_amd_odometry;
LVT_API lvt_amd_odometry lvt_amd_odometry_create(lvt_handle h, const double base_to_sensor[12] /* 3x4 row-major or NULL */, int reset_pose_on_lost);
LVT_API void lvt_amd_odometry_destroy(lvt_amd_odometry o);
LVT_API void lvt_amd_odometry_reset(lvt_amd_odometry o); /* the node's reset_vo service (lvt_ros.cpp:184-198): tracker reset, deltas restart, accumulated pose back to identity */
/* RELOCALISATION POLICY.  Once set (max_lost_frames > 0), a frame that comes back LOST makes the accumulator call lvt_amd_relocalise on its tracker instead of
 * resetting it.  On success the relocalised pose is pushed and 1 is returned: last_R / last_p are still those of the last tracked frame, so the published delta
 * spans the gap and the trajectory stays continuous.  On failure (also: an accumulator without a tracker) nothing is published and nothing is reset -- the map
 * stays --; the max_lost_frames-th consecutive failure falls back to the reference's reset, exactly as without the policy.  cfg NULL: the default config;
 * max_lost_frames <= 0: the policy is off and the accumulator behaves as it always did.  0; -1: a bad config field, dry_run = 1 included -- the accumulator's
 * relocalisation commits -- (the sentence in lvt_amd_last_error(NULL)).  lvt_amd_odometry_push_pose_cov / _update_cov: cov_out is all zero for a frame the
 * policy relocalised (cov_in and the perturbation map belong to the LOST frame handed in, not to the pose that was published). */
LVT_API int lvt_amd_odometry_set_relocalisation(lvt_amd_odometry o, const lvt_amd_reloc_config *cfg, int max_lost_frames);
LVT_API int lvt_amd_odometry_push_pose(lvt_amd_odometry o, const double R[3][3], const double t[3], int status, double stamp_sec,
                                       double pose_out[7], double twist_out[6]);
LVT_API int lvt_amd_odometry_update(lvt_amd_odometry o, unsigned char *left, unsigned char *right, int n_rows, int n_cols, double stamp_sec,
                                    double pose_out[7], double twist_out[6]);
/* ... with the covariance of the published pose.  cov_in: the frame's lvt_amd_pose_info::cov in the convention above; NULL when there is none (hand in
 * NULL unless the record's status is 1: a degenerate record's cov is all zero and says nothing).
 * cov_out: the 6 x 6 row-major covariance of the published base_link-in-odom pose in ROS's order and axes -- position, then rotation about the FIXED axes of
 * odom (geometry_msgs/PoseWithCovariance) --, obtained by pushing xi through the accumulator's own arithmetic.  With (R_po, .) the accumulated pose BEFORE this
 * frame, R_B the rotation of base_to_sensor, (., p_C) = base_to_sensor^-1, F = rot_fix, L the previous frame's fixed rotation (F R_prev; F before the first
 * frame and after a restart) and Q = R_po R_B F R:
 *     dp_ob = Q R^T dp - Q [L^T p_C]x dtheta,      dphi_ob = Q dtheta
 * so cov_out = M cov_in M^T with M = [Q R^T, -Q [L^T p_C]x; 0, Q].  It is the uncertainty of THIS frame's localisation against the local map, not
 * accumulated drift: the poses before it are taken as exact.  cov_out is all zero when cov_in is NULL or nothing was published (LOST, stale stamp).
 * pose_out, twist_out and the return value are exactly those of the functions above.  lvt_amd_odometry_update_cov tracks, fetches the record
 * (lvt_amd_get_pose_info; a record whose status is not 1 -- a handle that never enabled it included -- gives zeros) and pushes. */
LVT_API int lvt_amd_odometry_push_pose_cov(lvt_amd_odometry o, const double R[3][3], const double t[3], int status, double stamp_sec,
                                           const double cov_in[36], double pose_out[7], double twist_out[6], double cov_out[36]);
LVT_API int lvt_amd_odometry_update_cov(lvt_amd_odometry o, unsigned char *left, unsigned char *right, int n_rows, int n_cols, double stamp_sec,
                                        double pose_out[7], double twist_out[6], double cov_out[36]);

#ifdef __cplusplus
}
#endif
#endif
