// lvt_stage_entries.h -- the calls that run ONE stage alone on caller data (included by lvt_host.hip): the pose solver, the motion model, the rectifier's remap, the batched Hamming
// matcher, the pose-uncertainty record and the stages of the relocalisation.  Every differential test goes through them.  (lvt_amd_equalise_device, the
// CLAHE stage alone, stays beside clahe_img in lvt_frame_props.h and uses the same helpers; so do lvt_amd_mask_features and lvt_amd_depth_guard_features, the
// two filters behind k_gather, beside their setters there: what the two share -- the features into a host-built Seq, the upload, the fetch -- is StageFeatures.)
//
// WHAT they share: a call has no handle, so a refusal goes to the calling thread (refuse_call, lvt_amd_last_error(NULL)); its parameters come through
// stage_params; all of its device memory comes from one StageScratch, which frees it when the call returns, whichever way it returns; a call that reports a time
// takes it from a StageTimer.  No entry calls hipMalloc, hipFree or hipEventCreate itself.
#pragma once

namespace lvt {

// ---- the device memory of one call ---------------------------------------------------------------------------------------------------------------------
// The first HIP failure latches: every later buf is nullptr without a HIP call, every later fetch false, so a call takes all its buffers, asks ok() once and
// launches only then.  Copies run on the null stream and block the host.
class StageScratch {
    std::vector<void *> owned;
    bool good = true;

  public:
    StageScratch() = default;
    StageScratch(const StageScratch &) = delete;
    StageScratch &operator=(const StageScratch &) = delete;
    ~StageScratch() {
        for (void *p : owned) (void)hipFree(p);
    }
    bool ok() const { return good; }
    // n elements (at least 16 bytes), every byte `fill`, then the n elements of src where there are any.  The bytes are in place when it returns: the caller
    // may launch on any stream.
    template <typename T>
    T *buf(size_t n, const T *src = nullptr, int fill = 0) {
        void *p = nullptr;
        const size_t bytes = n * sizeof(T), cap = std::max(bytes, (size_t)16);
        if (!good || hipMalloc(&p, cap) != hipSuccess) return good = false, nullptr;
        owned.push_back(p);
        hipError_t e = hipMemset(p, fill, cap);
        if (e == hipSuccess) e = (src && bytes) ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) : hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return good = false, nullptr;
        return static_cast<T *>(p);
    }
    // n elements back to the host; nothing to do for n == 0 or a NULL dst (an output the caller did not ask for)
    template <typename T>
    bool fetch(T *dst, const T *src, size_t n) {
        if (good && dst && src && n && hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) good = false;
        return good;
    }
};

// ---- the parameters of one call ------------------------------------------------------------------------------------------------------------------------
// *pin as lvt_amd_create derives them for `sensor`; false: pin is NULL, or parameters lvt_amd_create would refuse.  A stage that reads no image size takes a
// 64 x 64 one where the caller gave none.  height_is_read: the stage reads img_height (the row band of stage 2's stereo partner search), so the caller must
// give it: a non-positive one is refused like any other bad parameter.
static bool stage_params(const lvt_amd_params *pin, int sensor, Params &prm, bool height_is_read = false) {
    if (!pin) return false;
    lvt_amd_params tmp = *pin;
    if (tmp.img_width <= 0) tmp.img_width = 64;
    if (tmp.img_height <= 0 && !height_is_read) tmp.img_height = 64;
    return derive_params(tmp, sensor, prm);
}

// ---- the time of one call's launches -------------------------------------------------------------------------------------------------------------------
// two HIP events around what the caller enqueues between begin and end; the first failure latches
class StageTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t err;
    void note(hipError_t e) {
        if (err == hipSuccess) err = e;
    }

  public:
    StageTimer() {
        err = hipEventCreate(&e0);
        note(hipEventCreate(&e1));
    }
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    ~StageTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    hipError_t error() const { return err; }
    void begin(hipStream_t st) { note(err == hipSuccess ? hipEventRecord(e0, st) : err); }
    void end(hipStream_t st) { note(err == hipSuccess ? hipEventRecord(e1, st) : err); }
    // waits for the end event: everything enqueued before it has run.  Microseconds between the two events, < 0 on any failure
    float us() {
        float ms = -1.0f;
        if (err == hipSuccess) note(hipEventSynchronize(e1));
        if (err == hipSuccess) note(hipEventElapsedTime(&ms, e0, e1));
        return (err == hipSuccess && ms >= 0) ? ms * 1000.0f : -1.0f;
    }
};

static Pose pose_of(const double q[4], const double p[3]) {
    Pose r;
    for (int k = 0; k < 4; k++) r.q[k] = q[k];
    for (int k = 0; k < 3; k++) r.p[k] = p[k];
    return r;
}
static void pose_out(const Pose &r, double q[4], double p[3]) {
    for (int k = 0; k < 4; k++) q[k] = r.q[k];
    for (int k = 0; k < 3; k++) p[k] = r.p[k];
}

// a matcher refusal: the sentence to the calling thread and, as ever, to stderr
static float hamming_refuse(const char *why) {
    refuse_call("lvt_amd_hamming_match_batched", why);
    std::fprintf(stderr, "%s\n", g_call_refusal.c_str());
    return -1.0f;
}
}  // namespace lvt

extern "C" {

// ---- motion-only BA on caller data ---------------------------------------------------------------------------------------------------------------------
// err_out (2n doubles, may be NULL): the edge errors the second chi2 gate saw; level_out (n ints, may be NULL): 1 = demoted by a gate;
// *borderline (may be NULL): gate decisions taken within PNP_GATE_MARGIN of the threshold
// trace (trace_cap rows x 4 doubles, may be NULL): one row per LM trial {lambda, chi2 at the estimate, chi2 of the trial, rho}; stats (may be NULL):
// {trials, rejected trials, passes ended by Terminate}.  What the kernel does not write comes back zero.  Inliers, or -1 (bad parameters, a HIP failure)
LVT_API int lvt_amd_pnp_trace(const lvt_amd_params *pin, const double q_in[4], const double p_in[3], const double *pts, const float *obs, int n,
                              double q_out[4], double p_out[3], int *n_solve_calls, double *err_out, int *level_out, int *borderline,
                              double *trace, int trace_cap, int stats[3]) {
    Params prm;
    if (!stage_params(pin, 1, prm)) return -1;
    if (!trace || trace_cap < 0) trace_cap = 0;
    const size_t nn = (size_t)std::max(n, 0);
    StageScratch S;
    const double *dX = S.buf<double>(nn * 3, pts);
    const float *dObs = S.buf<float>(nn * 2, obs);
    double *dErr = S.buf<double>(nn * 2 + 2);
    int8_t *dLevel = S.buf<int8_t>(nn);
    Pose *dOut = S.buf<Pose>(1);
    int *dInfo = S.buf<int>(8);
    double *dTrace = S.buf<double>((size_t)trace_cap * 4);
    if (!S.ok()) return -1;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pnp_standalone), hipFuncAttributeMaxDynamicSharedMemorySize, PNP_DYN_BYTES);
    hipLaunchKernelGGL(k_pnp_standalone, dim3(1), dim3(PNP_THREADS), PNP_DYN_BYTES, 0, prm, pose_of(q_in, p_in), dX, dObs, dErr, dLevel, n, dOut, dInfo,
                       trace_cap ? dTrace : (double *)nullptr, trace_cap);
    Pose out;
    int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int8_t> lv(level_out ? nn : 0);
    if (hipGetLastError() != hipSuccess || !S.fetch(&out, dOut, 1) || !S.fetch(info, dInfo, 8)) return -1;
    if (stats) stats[0] = info[3], stats[1] = info[4], stats[2] = info[5];
    pose_out(out, q_out, p_out);
    if (n_solve_calls) *n_solve_calls = info[0];
    if (borderline) *borderline = info[2];
    S.fetch(trace, dTrace, (size_t)std::min(trace_cap, std::max(info[3], 0)) * 4);
    S.fetch(err_out, dErr, nn * 2);
    S.fetch(lv.data(), dLevel, lv.size());
    for (size_t i = 0; i < lv.size(); i++) level_out[i] = lv[i];
    return S.ok() ? info[1] : -1;
}
LVT_API int lvt_amd_pnp_detail(const lvt_amd_params *pin, const double q_in[4], const double p_in[3], const double *pts, const float *obs, int n,
                               double q_out[4], double p_out[3], int *n_solve_calls, double *err_out, int *level_out, int *borderline) {
    return lvt_amd_pnp_trace(pin, q_in, p_in, pts, obs, n, q_out, p_out, n_solve_calls, err_out, level_out, borderline, nullptr, 0, nullptr);
}
LVT_API int lvt_amd_pnp(const lvt_amd_params *pin, const double q_in[4], const double p_in[3], const double *pts, const float *obs, int n,
                        double q_out[4], double p_out[3], int *n_solve_calls) {
    return lvt_amd_pnp_detail(pin, q_in, p_in, pts, obs, n, q_out, p_out, n_solve_calls, nullptr, nullptr, nullptr);
}

// ---- the constant-velocity motion model on caller data (the contract of the oracle's lvto_motion_predict) ---------------------------------------------------------
// state = {last_q[4], ang_vel[4], last_p[3], lin_vel[3]} in, the model's next state out; (q, p) the current pose; runs on the current device.  0 / -1
LVT_API int lvt_amd_motion_predict(double state[14], const double q[4], const double p[3], double q_out[4], double p_out[3]) {
    if (!state || !q || !p || !q_out || !p_out) return -1;
    double io[21];
    std::copy_n(state, 14, io);
    std::copy_n(q, 4, io + 14), std::copy_n(p, 3, io + 18);
    StageScratch S;
    Ctl *dCtl = S.buf<Ctl>(1);
    double *dIo = S.buf<double>(21, io);
    if (!S.ok()) return -1;
    hipLaunchKernelGGL(k_motion_predict_standalone, dim3(1), dim3(64), 0, 0, dCtl, dIo);
    if (hipGetLastError() != hipSuccess || !S.fetch(io, dIo, 21)) return -1;
    std::copy_n(io, 14, state);
    std::copy_n(io + 14, 4, q_out), std::copy_n(io + 18, 3, p_out);
    return 0;
}

// ---- the remap alone, on caller maps (k_rectify.hip; the definition is in include/lvt_amd_ext.h, "RECTIFICATION") ---------------------------------------------------
// d_src (sh rows of src_pitch bytes, any address) and d_dst (dh rows of dst_pitch bytes, 4-byte aligned) are DEVICE pointers; map1, map2 are HOST arrays of
// dw x dh floats.  route 0: k_rectify on the float maps (what lvt_amd_rectify_device launches); route 1: k_rectify_fix, then k_rectify_frames with a one-image
// RectTable (what a tracker's feature stage launches).  Runs on the null stream and returns when the plane is written.  *launches (may be NULL): the kernels
// the call launched, 0 on a refusal.  0, or -1 on a refusal (lvt_amd_last_error(NULL)) or a HIP failure.
LVT_API int lvt_amd_remap_device(const void *d_src, int sw, int sh, int src_pitch, const float *map1, const float *map2, int dw, int dh, void *d_dst,
                                 int dst_pitch, int route, int *launches) {
    const char *who = "lvt_amd_remap_device";
    if (launches) *launches = 0;
    if (!d_src || !map1 || !map2 || !d_dst) return refuse_call(who, "a NULL argument (nothing was launched)");
    if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0) return refuse_call(who, "a size that is not positive (nothing was launched)");
    if (src_pitch < sw) return refuse_call(who, "a source pitch smaller than the source width (nothing was launched)");
    if (dst_pitch < dw || (dst_pitch & 3) || ((uintptr_t)d_dst & 3))
        return refuse_call(who, "a destination pitch smaller than the map width or no multiple of 4, or a destination that is not 4-byte aligned (nothing was launched)");
    if ((long long)src_pitch * sh > INT_MAX || (long long)dst_pitch * dh > INT_MAX)
        return refuse_call(who, "a plane of more than INT_MAX bytes (nothing was launched)");
    if (route != 0 && route != 1) return refuse_call(who, "unknown route " + std::to_string(route) + " (nothing was launched)");
    const size_t n = (size_t)dw * dh;
    StageScratch S;
    const float *d_map1 = S.buf<float>(n, map1), *d_map2 = S.buf<float>(n, map2);
    int2 *d_fix = route == 1 ? S.buf<int2>(n) : nullptr;
    if (!S.ok()) return refuse_call(who, hipGetErrorString(hipGetLastError()));
    int launched = 0;
    if (route == 0) {
        hipLaunchKernelGGL(k_rectify, dim3((dst_pitch / 4 + 255) / 256, dh), dim3(256), 0, 0, static_cast<const uint8_t *>(d_src), sw, sh, src_pitch, d_map1, d_map2,
                           dw, dh, static_cast<uint8_t *>(d_dst), dst_pitch);
        launched = 1;
    } else {
        RectTable tab;
        std::memset(&tab, 0, sizeof(tab));
        tab.im[0] = RectImg{static_cast<const uint8_t *>(d_src), d_fix, static_cast<uint8_t *>(d_dst), src_pitch, dst_pitch, sw, sh, dw, dh};
        hipLaunchKernelGGL(k_rectify_fix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_map1, d_map2, d_fix, n);
        hipLaunchKernelGGL(k_rectify_frames, dim3((dst_pitch / 4 * dh + 255) / 256, 1), dim3(256), 0, 0, tab);
        launched = 2;
    }
    if (launches) *launches = launched;
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return refuse_call(who, hipGetErrorString(hipGetLastError()));
    return 0;
}

// ---- batched masked 2-NN Hamming matcher on device-resident problems -----------------------------------------------------------------------------------
LVT_API float lvt_amd_hamming_match_batched_n(const void *q_desc, const void *q_xy, const void *t_desc, const void *t_xy, const void *t_flag,
                                              int B, int M, int N, float r2, int mode, int img_rows, int img_cols, void *out,
                                              void *hip_stream, int launches) {
    if (launches < 1) launches = 1;
    if (B > 0 && M > 0 && M <= HB_MMAX && N == 0) {  // an empty train set: knnMatch returns nothing for every query
        hipLaunchKernelGGL(k_hamming_none, dim3((unsigned)(((size_t)B * M + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
                           static_cast<int4 *>(out), (size_t)B * M);
        return hipStreamSynchronize(static_cast<hipStream_t>(hip_stream)) == hipSuccess ? 0.0f : -1.0f;
    }
    char why[200];
    if (B <= 0 || M <= 0 || N <= 0 || N > HB_NMAX || M > HB_MMAX) {
        snprintf(why, sizeof why, "bad sizes B=%d M=%d N=%d (N <= %d, M <= %d)", B, M, N, HB_NMAX, HB_MMAX);
        return hamming_refuse(why);
    }
    HammingArgs a;
    a.q_desc = static_cast<const uint64_t *>(q_desc);
    a.q_xy = static_cast<const float2 *>(q_xy);
    a.t_desc = static_cast<const uint64_t *>(t_desc);
    a.t_xy = static_cast<const float2 *>(t_xy);
    a.t_flag = static_cast<const uint8_t *>(t_flag);
    a.out = static_cast<int4 *>(out);
    a.M = M, a.N = N, a.r2 = r2, a.img_rows = img_rows, a.img_cols = img_cols;
    StageScratch S;
    a.dbg = std::getenv("LVT_AMD_HAMMING_DEBUG") ? S.buf<long long>(8) : nullptr;  // (a buffer that cannot be had: the call runs without the phase stamps)
    if (mode == 1) {
        a.nbx = 1, a.nby = img_rows + 1, a.csr = 0;
    } else {
        a.nbx = (int)std::ceil(img_cols / (float)HASH_CELL), a.nby = (int)std::ceil(img_rows / (float)HASH_CELL);
        a.csr = std::max(1, (int)std::ceil(std::sqrt(r2) / (float)HASH_CELL));
    }
    // the variant fixes how many candidate ranges a query keeps in registers (k_hamming.hip)
    void (*kern)(HammingArgs) = nullptr;
    {
        const int qpt = (M + HB_THREADS - 1) / HB_THREADS;
        const int tpt = (N + HB_THREADS - 1) / HB_THREADS;
#define LVT_PICK_T(MODE_, NSP_, Q_)                                                                                               \
    ((tpt == 1) ? k_hamming_batched<MODE_, NSP_, Q_, 1> : (tpt == 2) ? k_hamming_batched<MODE_, NSP_, Q_, 2> :                   \
     (tpt == 3) ? k_hamming_batched<MODE_, NSP_, Q_, 3> : k_hamming_batched<MODE_, NSP_, Q_, 4>)
#define LVT_PICK(MODE_, NSP_)                                                                                                     \
    kern = (qpt == 1) ? LVT_PICK_T(MODE_, NSP_, 1) : (qpt == 2) ? LVT_PICK_T(MODE_, NSP_, 2) : (qpt == 3) ? LVT_PICK_T(MODE_, NSP_, 3) \
                                                                                                          : LVT_PICK_T(MODE_, NSP_, 4)
        if (mode == 1) LVT_PICK(1, 1);
        else if (a.csr == 1) LVT_PICK(0, 3);
        else if (a.csr == 2) LVT_PICK(0, 5);
        else LVT_PICK(0, 0);
#undef LVT_PICK_T
#undef LVT_PICK
    }
    // a workgroup's 160 KiB hold the carve-up AND the kernel's static arrays (s_scan, s_hist, s_recheck): a size that leaves them no room is refused
    // here, not at the launch
    const size_t lds = hamming_lds_bytes(N, M, a.nbx * a.nby);
    hipFuncAttributes fattr;
    if (hipFuncGetAttributes(&fattr, reinterpret_cast<const void *>(kern)) != hipSuccess) return hamming_refuse("hipFuncGetAttributes failed");
    if (lds + fattr.sharedSizeBytes > 160 * 1024) {
        snprintf(why, sizeof why, "%zu + %zu bytes of LDS needed", lds, (size_t)fattr.sharedSizeBytes);
        return hamming_refuse(why);
    }
    // the timed region, which bench.py's matcher figures come from: the attribute is set before the first record, the launches run back to back between the
    // two records and nothing else goes to the stream between them
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    StageTimer T;
    if (T.error() != hipSuccess) {
        snprintf(why, sizeof why, "hipEventCreate failed: %s", hipGetErrorString(T.error()));
        return hamming_refuse(why);
    }
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    T.begin(st);
    for (int l = 0; l < launches; l++) hipLaunchKernelGGL(kern, dim3(B), dim3(HB_THREADS), lds, st, a);
    const hipError_t elaunch = hipGetLastError();
    T.end(st);
    float us = T.us();
    if (elaunch != hipSuccess) us = -1.0f;
    if (us < 0)
        std::fprintf(stderr, "lvt_amd_hamming_match_batched: attr=%s launch=%s timer=%s (B=%d M=%d N=%d lds=%zu)\n", hipGetErrorString(ea),
                     hipGetErrorString(elaunch), hipGetErrorString(T.error()), B, M, N, lds);
    long long hd[8] = {};
    if (a.dbg && S.fetch(hd, a.dbg, 8)) {
        if (hd[7] == 0) hd[7] = hd[5];
        std::fprintf(stderr, "hamming phases (cycles): load+zero %lld count %lld scan %lld scatter+qcount %lld qsort %lld radius+qsort2 %lld descriptors %lld total %lld\n",
                     hd[1] - hd[0], hd[2] - hd[1], hd[3] - hd[2], hd[4] - hd[3], hd[5] - hd[4], hd[7] - hd[5], hd[6] - hd[7], hd[6] - hd[0]);
    }
    return us < 0 ? -1.0f : us / (float)launches;
}

LVT_API float lvt_amd_hamming_match_batched(const void *q_desc, const void *q_xy, const void *t_desc, const void *t_xy, const void *t_flag,
                                            int B, int M, int N, float r2, int mode, int img_rows, int img_cols, void *out,
                                            void *hip_stream) {
    return lvt_amd_hamming_match_batched_n(q_desc, q_xy, t_desc, t_xy, t_flag, B, M, N, r2, mode, img_rows, img_cols, out, hip_stream, 1);
}

// ---- the pose-uncertainty record on caller data (k_poseinfo.hip) -----------------------------------------------------------------------------------------
LVT_API int lvt_amd_pose_info_eval(const lvt_amd_params *pin, const double q_wxyz[4], const double pos[3], const double *pts, const float *obs, int n,
                                   lvt_amd_pose_info *out) {
    if (!pin || !q_wxyz || !pos || !out || n < 0 || n > NF_MAX || (n > 0 && (!pts || !obs))) return -1;
    Params prm;
    if (!stage_params(pin, 1, prm)) return -1;
    StageScratch S;
    const double *dX = S.buf<double>((size_t)n * 3, pts);
    const float *dObs = S.buf<float>((size_t)n * 2, obs);
    lvt_amd_pose_info *dOut = S.buf<lvt_amd_pose_info>(1);
    if (!S.ok()) return -1;
    hipLaunchKernelGGL(k_pose_info_standalone, dim3(1), dim3(PI_THREADS), 0, 0, prm, pose_of(q_wxyz, pos), dX, dObs, n, dOut);
    return hipGetLastError() == hipSuccess && S.fetch(out, dOut, 1) ? 0 : -1;
}

// ---- relocalisation: the stages alone on caller data (k_reloc.hip; the definition is in include/lvt_amd_ext.h, "RELOCALISATION") -----------------------------------
// What the entries share with a handle's call (relocalise, lvt_host.hip): the config check and the launches of stages 1 and 2.
// "" when every field is in range, else the complete sentence of the refusal (it names the field)
static std::string reloc_config_fault(const lvt_amd_reloc_config &c) {
    char b[200] = "";
    if (c.n_hypotheses < 1 || c.n_hypotheses > RELOC_HYP_MAX)
        snprintf(b, sizeof b, "n_hypotheses is %d: it must be 1 ... %d (nothing was changed)", c.n_hypotheses, RELOC_HYP_MAX);
    else if (!(std::isfinite(c.gate_px2) && c.gate_px2 > 0))
        snprintf(b, sizeof b, "gate_px2 is %g: it must be finite and > 0 (nothing was changed)", (double)c.gate_px2);
    else if (!(std::isfinite(c.min_disparity) && c.min_disparity > 0))
        snprintf(b, sizeof b, "min_disparity is %g: it must be finite and > 0 (nothing was changed)", (double)c.min_disparity);
    else if (c.min_inliers < 3)
        snprintf(b, sizeof b, "min_inliers is %d: it must be >= 3 (nothing was changed)", c.min_inliers);
    else if (c.dry_run != 0 && c.dry_run != 1)
        snprintf(b, sizeof b, "dry_run is %d: it must be 0 or 1 (nothing was changed)", c.dry_run);
    return b;
}
// stages 1 and 2 of one call: four launches on `st`, the capacity grid, every size read on the device (RelocSeq's scalars and its FeatCtl).  A handle's call
// (relocalise) and the stage entry lvt_amd_reloc_correspond both come through here: what the entry is held to is what the handle runs.
static void reloc_launch_correspond(hipStream_t st, const RelocSeq &rs, const uint64_t *mdesc0, const uint64_t *mdesc1, const RelocBufs &b, const Params &prm,
                                    float min_disparity) {
    const RelocDims dims{rs.n_feat[0], rs.map_n, rs.map_cur, rs.fc};
    hipLaunchKernelGGL(k_reloc_match<true>, dim3(NF_MAX / RELOC_THREADS, MAP_MAX / RELOC_SLICE_MAX), dim3(RELOC_THREADS), 0, st, (const uint4 *)rs.desc[0],
                       (const uint4 *)mdesc0, (const uint4 *)mdesc1, dims, b.keys);
    hipLaunchKernelGGL(k_reloc_corr, dim3(1), dim3(1024), 0, st, rs, b, prm.track_ratio, prm.desc_th);
    hipLaunchKernelGGL(k_reloc_points, dim3(NF_MAX / (RELOC_THREADS / 64)), dim3(RELOC_THREADS), 0, st, rs, b, prm, min_disparity);
    hipLaunchKernelGGL(k_reloc_list, dim3(1), dim3(1024), 0, st, b);
}
// stage 1 alone.  d_query n_query x 32 B, d_map n_map x 32 B, d_out n_query x 4 int32 (idx1, d1, idx2, d2; -1 / INT_MAX when absent): DEVICE pointers, 16-byte
// aligned.  Both launches go to hip_stream; the call allocates its key buffer and frees it once the stream has run them (the timer's end event).  Returns the
// elapsed time of the two launches in microseconds (HIP events), < 0 on a refusal or a HIP failure (lvt_amd_last_error(NULL) has the sentence of a refusal).
LVT_API float lvt_amd_reloc_match_device(const void *d_query, int n_query, const void *d_map, int n_map, void *d_out, void *hip_stream) {
    if (n_query < 0 || n_query > NF_MAX || n_map < 0 || n_map > MAP_MAX || (n_query > 0 && (!d_query || !d_out)) || (n_map > 0 && n_query > 0 && !d_map) ||
        ((uintptr_t)d_query | (uintptr_t)d_map | (uintptr_t)d_out) % 16)
        return (float)refuse_call("lvt_amd_reloc_match_device",
                                  "n_query must be 0 ... 4096, n_map 0 ... 32768, the pointers device pointers aligned to 16 bytes (nothing was changed)");
    if (n_query == 0) return 0.0f;
    hipStream_t st = (hipStream_t)hip_stream;
    const int slice = reloc_slice_length(n_map), slices = (n_map + slice - 1) / slice, gx = (n_query + RELOC_THREADS - 1) / RELOC_THREADS;
    const int h_dims[3] = {n_query, n_map, 0};
    StageScratch S;
    uint2 *keys = S.buf<uint2>((size_t)std::max(slices, 1) * n_query);
    const int *d_dims = S.buf<int>(3, h_dims);
    StageTimer T;
    if (!S.ok() || T.error() != hipSuccess) return -1.0f;
    const RelocDims dims{d_dims, d_dims + 1, d_dims + 2, nullptr};
    T.begin(st);
    const char *lab = getenv("LVT_AMD_RELOC_MATCH");  // "uniform": the lab variant without LDS (this stage entry only; a handle's call always stages in LDS)
    if (slices > 0 && lab && !strcmp(lab, "uniform"))
        hipLaunchKernelGGL(k_reloc_match<false>, dim3(gx, slices), dim3(RELOC_THREADS), 0, st, (const uint4 *)d_query, (const uint4 *)d_map, (const uint4 *)d_map, dims,
                           keys);
    else if (slices > 0)
        hipLaunchKernelGGL(k_reloc_match<true>, dim3(gx, slices), dim3(RELOC_THREADS), 0, st, (const uint4 *)d_query, (const uint4 *)d_map, (const uint4 *)d_map, dims,
                           keys);
    hipLaunchKernelGGL(k_reloc_merge_records, dim3(gx), dim3(RELOC_THREADS), 0, st, (const uint2 *)keys, dims, (int4 *)d_out);
    T.end(st);
    const bool launched = hipGetLastError() == hipSuccess;
    const float us = T.us();
    return launched ? us : -1.0f;
}
// stages 3 - 5 alone.  Host pointers: pts n x 3 f64 (world), obs n x 2 f32, pc n x 3 f64 (camera frame), has_pc n bytes (0: the correspondence has no point, its
// pc row is not read), 0 <= n <= 4096.  counts_out (n_hypotheses ints), inliers_out (n ints: the best hypothesis' inliers, the first n_hyp_inliers of them),
// hyp_R (9) and hyp_t (3) may each be NULL; the last three are written for status 0 and 3 only.  Returns 0 / 1 as lvt_amd_relocalise does, -1 on a refusal.
LVT_API int lvt_amd_reloc_solve(const lvt_amd_params *pin, const lvt_amd_reloc_config *cfg_in, const double *pts, const float *obs, const double *pc,
                                const uint8_t *has_pc, int n, int *counts_out, int *inliers_out, double *hyp_R, double *hyp_t, lvt_amd_reloc_result *out) {
    const char *who = "lvt_amd_reloc_solve";
    if (!pin || !out || n < 0 || n > NF_MAX || (n > 0 && (!pts || !obs || !pc || !has_pc)))
        return refuse_call(who, "a NULL argument, or n outside 0 ... 4096 (nothing was changed)");
    lvt_amd_reloc_config cfg;
    lvt_amd_reloc_default_config(&cfg);
    if (cfg_in) cfg = *cfg_in;
    const std::string fault = reloc_config_fault(cfg);
    if (!fault.empty()) return refuse_call(who, fault);
    Params prm;
    if (!stage_params(pin, 1, prm)) return refuse_call(who, "parameters lvt_amd_create would refuse (nothing was changed)");
    std::vector<int> with_pc;
    for (int i = 0; i < n; i++)
        if (has_pc[i]) with_pc.push_back(i);
    RelocWork w{};
    w.res.n_corr = n, w.res.n_with_point = (int)with_pc.size();
    with_pc.resize((size_t)n);  // (uploaded whole)
    w.res.status = w.res.n_with_point < 3 ? 1 : -1;
    w.success = std::max(cfg.min_inliers, prm.min_matches);
    const size_t nn = (size_t)n;
    std::vector<int> counts((size_t)cfg.n_hypotheses, 0);
    StageScratch S;
    // (X, uv, Pc, with_pc; the sizes travel in the work record)
    const RelocCorr c{S.buf<double>(nn * 3, pts), S.buf<float>(nn * 2, obs), S.buf<double>(nn * 3, pc), S.buf<int>(nn, with_pc.data()), 0, 0};
    double *dEX = S.buf<double>(nn * 3), *dErr = S.buf<double>(nn * 2 + 2);
    float *dEObs = S.buf<float>(nn * 2);
    int *dCounts = S.buf<int>(counts.size()), *dInl = S.buf<int>(nn);
    int8_t *dLevel = S.buf<int8_t>(nn);
    RelocWork *dW = S.buf<RelocWork>(1, &w);
    if (S.ok()) {
        const RelocCam cam{(double)prm.fx, (double)prm.fy, (double)prm.cx, (double)prm.cy};
        const double gate = (double)cfg.gate_px2;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_reloc_refine), hipFuncAttributeMaxDynamicSharedMemorySize, PNP_DYN_BYTES);
        hipLaunchKernelGGL(k_reloc_score, dim3((cfg.n_hypotheses + 3) / 4), dim3(RELOC_THREADS), 0, 0, c, (const RelocWork *)dW, cam, (uint64_t)cfg.seed, gate, cfg.n_hypotheses,
                           dCounts);
        hipLaunchKernelGGL(k_reloc_select, dim3(1), dim3(RELOC_THREADS), 0, 0, c, cam, (uint64_t)cfg.seed, gate, cfg.n_hypotheses, (const int *)dCounts, dW, dInl, dEX,
                           dEObs);
        hipLaunchKernelGGL(k_reloc_refine, dim3(1), dim3(PNP_THREADS), PNP_DYN_BYTES, 0, prm, dW, (const double *)dEX, (const float *)dEObs, dErr, dLevel);
        if (hipGetLastError() == hipSuccess && S.fetch(&w, dW, 1) && S.fetch(counts.data(), dCounts, counts.size()) &&
            S.fetch(inliers_out, dInl, (size_t)std::max(w.n_edges, 0))) {
            if (w.res.status != 0 && w.res.status != 3) {  // the pose is zero unless the refinement ran
                for (int k = 0; k < 4; k++) w.res.q_wxyz[k] = 0;
                for (int k = 0; k < 3; k++) w.res.p[k] = w.res.t[k] = 0;
                for (int k = 0; k < 9; k++) w.res.R[k / 3][k % 3] = 0;
            } else {
                if (hyp_R) std::memcpy(hyp_R, w.hyp_R, sizeof w.hyp_R);
                if (hyp_t) std::memcpy(hyp_t, w.hyp_t, sizeof w.hyp_t);
            }
            if (counts_out) std::memcpy(counts_out, counts.data(), counts.size() * 4);
            *out = w.res;
            return w.res.status == 0 ? 0 : 1;
        }
    }
    return refuse_call(who, hipGetErrorString(hipGetLastError()));
}
// stage 2 (behind stage 1) alone, through the launches of a handle's call (reloc_launch_correspond).  Host pointers.  The data is laid out as a handle holds
// it: feature arrays of both eyes with their device counts, a FeatCtl, two map copies of which map_copy is the live one (the other copy is filled from
// other_pos / other_desc, zeros when NULL).  lost_frame: the counts are delivered as a LOST frame leaves them (Feat::n zero, FeatCtl::lost_n, lost_seq ==
// feat_seq).  The six output arrays hold NF_MAX elements each (X, Pc: x 3; uv: x 2): they are uploaded as the caller filled them and read back whole, so an
// element the kernels do not write comes back with the caller's bytes.  claims_left (may be NULL): entries of the claim table that are not empty behind the
// call.  Returns 0 (out->status: 1 or -1, as stage 2 leaves it), -1 on a refusal or a HIP failure.
LVT_API int lvt_amd_reloc_correspond(const lvt_amd_params *pin, const lvt_amd_reloc_config *cfg_in, int sensor, const float *xl, const float *yl,
                                     const uint8_t *desc_l, const float *depth_l, int n_left, const float *xr, const float *yr, const uint8_t *desc_r, int n_right,
                                     const double *map_pos, const uint8_t *map_desc, const double *other_pos, const uint8_t *other_desc, int n_map, int map_copy,
                                     int lost_frame, lvt_amd_reloc_result *out, int *corr_feat, double *X, float *uv, uint8_t *has_pc, double *Pc, int *with_pc,
                                     int *claims_left) {
    const char *who = "lvt_amd_reloc_correspond";
    const bool stereo = sensor == 1;
    if (!stereo) n_right = 0;
    if (!pin || !out || !corr_feat || !X || !uv || !has_pc || !Pc || !with_pc || (sensor != 1 && sensor != 2) || n_left < 0 || n_left > NF_MAX || n_right < 0 ||
        n_right > NF_MAX || n_map < 0 || n_map > MAP_MAX || (map_copy != 0 && map_copy != 1) || (lost_frame != 0 && lost_frame != 1) ||
        (n_left > 0 && (!xl || !yl || !desc_l || (!stereo && !depth_l))) || (n_right > 0 && (!xr || !yr || !desc_r)) || (n_map > 0 && (!map_pos || !map_desc)))
        return refuse_call(who, "a NULL argument, sensor not 1 or 2, a feature count outside 0 ... 4096, n_map outside 0 ... 32768, or map_copy or "
                                "lost_frame not 0 or 1 (nothing was changed)");
    lvt_amd_reloc_config cfg;
    lvt_amd_reloc_default_config(&cfg);
    if (cfg_in) cfg = *cfg_in;
    const std::string fault = reloc_config_fault(cfg);
    if (!fault.empty()) return refuse_call(who, fault);
    Params prm;
    if (!stage_params(pin, sensor, prm, true)) return refuse_call(who, "parameters lvt_amd_create would refuse (nothing was changed)");
    // (Feat::n of both eyes, map_n, map_cur)
    const int h_scalars[4] = {lost_frame ? 0 : n_left, lost_frame ? 0 : n_right, n_map, map_copy};
    FeatCtl fc{};
    fc.feat_seq = 1, fc.skip_seq = 0;  // a zeroed record would read as "this frame has no features"
    if (lost_frame) fc.lost_n[0] = n_left, fc.lost_n[1] = n_right, fc.lost_seq = fc.feat_seq;
    RelocWork w{};
    w.res.status = -1;
    const size_t nl = (size_t)n_left, nr = (size_t)n_right, nm = (size_t)n_map, cap = (size_t)NF_MAX;
    StageScratch S;
    const int *d_scalars = S.buf<int>(4, h_scalars);
    RelocSeq rs{};
    rs.x[0] = S.buf<float>(nl, xl), rs.y[0] = S.buf<float>(nl, yl);
    rs.desc[0] = (const uint64_t *)S.buf<uint8_t>(nl * 32, desc_l);
    rs.depth = stereo ? nullptr : S.buf<float>(nl, depth_l);
    if (stereo) {
        rs.x[1] = S.buf<float>(nr, xr), rs.y[1] = S.buf<float>(nr, yr);
        rs.desc[1] = (const uint64_t *)S.buf<uint8_t>(nr * 32, desc_r);
    }
    const uint64_t *mdesc[2];
    mdesc[map_copy] = (const uint64_t *)S.buf<uint8_t>(nm * 32, map_desc), mdesc[map_copy ^ 1] = (const uint64_t *)S.buf<uint8_t>(nm * 32, other_desc);
    rs.map_pos[map_copy] = S.buf<double>(nm * 3, map_pos), rs.map_pos[map_copy ^ 1] = S.buf<double>(nm * 3, other_pos);
    rs.n_feat[0] = d_scalars, rs.n_feat[1] = d_scalars + 1, rs.map_n = d_scalars + 2, rs.map_cur = d_scalars + 3;
    rs.fc = S.buf<FeatCtl>(1, &fc);
    const int slice = reloc_slice_length(n_map), slices = (n_map + slice - 1) / slice;
    RelocBufs b{};
    b.keys = S.buf<uint2>((size_t)std::max(slices, 1) * std::max(n_left, 1));
    b.claim = S.buf<uint32_t>(nm, nullptr, 0xFF);  // RELOC_NO_KEY
    b.corr_feat = S.buf<int>(cap, corr_feat), b.with_pc = S.buf<int>(cap, with_pc);
    b.X = S.buf<double>(cap * 3, X), b.Pc = S.buf<double>(cap * 3, Pc);
    b.uv = S.buf<float>(cap * 2, uv), b.has_pc = S.buf<uint8_t>(cap, has_pc);
    b.work = S.buf<RelocWork>(1, &w);
    if (S.ok()) {
        reloc_launch_correspond(nullptr, rs, mdesc[0], mdesc[1], b, prm, cfg.min_disparity);
        std::vector<uint32_t> claim(nm);
        if (hipGetLastError() == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess && S.fetch(&w, b.work, 1) &&
            S.fetch(corr_feat, b.corr_feat, cap) && S.fetch(with_pc, b.with_pc, cap) && S.fetch(X, b.X, cap * 3) &&
            S.fetch(Pc, b.Pc, cap * 3) && S.fetch(uv, b.uv, cap * 2) && S.fetch(has_pc, b.has_pc, cap) &&
            S.fetch(claim.data(), b.claim, nm)) {
            int left = 0;
            for (uint32_t k : claim) left += k != RELOC_NO_KEY;
            if (claims_left) *claims_left = left;
            *out = w.res;
            return 0;
        }
    }
    return refuse_call(who, hipGetErrorString(hipGetLastError()));
}
}  // extern "C"
