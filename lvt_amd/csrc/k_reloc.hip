// k_reloc.hip -- relocalisation: a search with no pose prior (include/lvt_amd_ext.h, "RELOCALISATION", has the definition; tests/reloc_util.py restates it).
//   k_reloc_match   stage 1: the two nearest map descriptors of every query over ALL map points.  A thread owns a query (its 256 bits in eight registers),
//                   a workgroup a slice of the map staged in LDS; every lane of a wave reads the same point (a broadcast read), so a pair costs 8 xor + 8 bcnt
//                   + the key update.  A slice writes its two packed keys distance << 16 | index per query: the tie rule is the integer minimum.
//   reloc_merge     the slices' keys of one query folded into its two best (keys of different points differ, so the fold is order-free)
//   k_reloc_corr    stage 2 on a handle's data: merge, the tracker's accept rule, the mutual filter (an integer minimum per claimed map point), ordered compaction
//   k_reloc_points  ... and each correspondence's camera-frame point: the depth, or the stereo partner found by one wavefront over the right features
//   k_reloc_list    ... and the correspondences that have one, in order
//   k_reloc_score   stages 3 and 4: one wavefront per hypothesis; every lane builds the pose (no broadcast, no LDS), the lanes stride over the correspondences,
//                   the count is a ballot popcount
//   k_reloc_select  arg-max with ties to the lowest hypothesis, the winning pose once more, its inliers in correspondence order as the solver's edges
//   k_reloc_refine  stage 5: pnp_solve (k_track.hip), the code behind k_pnp and lvt_amd_pnp, on the edges k_reloc_select wrote
//   k_reloc_commit  stage 6: one thread writes the sequence's Ctl (reloc_commit_ctl, which the host patches its ring with)
// fp64 after widening, one IEEE operation per written operation (the file is compiled with -ffp-contract=off like the rest of the library), + - * / sqrt only,
// sums of three written ((a b + c d) + e f).
// Included by lvt_host.hip behind k_track.hip, whose pnp_solve it uses.
#pragma once
#include "lvt_dev.h"
#include "lvt_math.h"
#include "../../include/lvt_amd_ext.h"

namespace lvt {

constexpr int RELOC_THREADS = 256;
constexpr int RELOC_SLICE_MAX = 1024;  // points of one slice: 32 KB of LDS
constexpr int RELOC_SLICE_MIN = 32;
constexpr int RELOC_HYP_MAX = 1024;
constexpr uint32_t RELOC_NO_KEY = 0xFFFFFFFFu;  // above every key: a key is distance << 16 | index < 257 << 16
constexpr double RELOC_DEGENERATE = 1e-12;

// the slice length follows M: about 32 slices whatever the map's size, so a map of a few hundred points still spreads over the chip
__host__ __device__ inline int reloc_slice_length(int M) {
    int s = (M + 31) / 32;
    s = (s + RELOC_SLICE_MIN - 1) / RELOC_SLICE_MIN * RELOC_SLICE_MIN;
    return s < RELOC_SLICE_MIN ? RELOC_SLICE_MIN : (s > RELOC_SLICE_MAX ? RELOC_SLICE_MAX : s);
}

// b1 <= b2 are the two smallest keys so far
__device__ __forceinline__ void reloc_top2(uint32_t &b1, uint32_t &b2, uint32_t k) {
    b2 = min(b2, max(b1, k));
    b1 = min(b1, k);
}

// where a call's sizes live: the stage entry uploads them, a handle's call reads the sequence's own device scalars (the feature count of the last frame,
// map_n and map_cur of the live map)
struct RelocDims {
    const int *n_query, *n_map, *map_cur;
    const FeatCtl *fc;  // a handle's call: of the last frame's buffer; the stage entry: nullptr
};
// the feature count of eye e of a handle's last frame: Feat::n, or -- a LOST frame, whose epilogue zeroed it -- the count that epilogue kept
__device__ __forceinline__ int reloc_n_feat(const int *n, const FeatCtl *fc, int e) {
    int v = *n;
    // (plain loads, not load_seq: the call runs on a drained handle, behind every writer of these words on its own stream, and every thread of the call's
    //  first four launches comes through here -- as acquire loads the two reads cost the call 38 us, measured: profiles/relocalisation.md)
    if (v == 0 && fc && fc->lost_seq == fc->feat_seq) v = fc->lost_n[e];
    return min(max(v, 0), NF_MAX);
}
__device__ __forceinline__ int reloc_n_query(const RelocDims &d) { return reloc_n_feat(d.n_query, d.fc, 0); }
__device__ __forceinline__ int reloc_n_map(const RelocDims &d) { return min(max(*d.n_map, 0), MAP_MAX); }

// grid (up to ceil(NF_MAX / 256), up to MAP_MAX / RELOC_SLICE_MAX): a workgroup outside the call's sizes leaves at the top.  keys: [slices][N] pairs.
// LDS: the slice is staged in LDS and read back at a wave-uniform address (the variant the library ships: profiles/relocalisation.md); !LDS: the same
// walk with the slice's descriptors loaded straight from memory at a wave-uniform address -- plain uniform loads, no LDS (the stage entry's lab variant)
template <bool LDS>
__global__ __launch_bounds__(RELOC_THREADS) void k_reloc_match(const uint4 *__restrict__ qdesc, const uint4 *__restrict__ mdesc0, const uint4 *__restrict__ mdesc1,
                                                               RelocDims dims, uint2 *__restrict__ keys) {
    __shared__ uint4 s_desc[LDS ? 2 * RELOC_SLICE_MAX : 1];
    const int N = reloc_n_query(dims), M = reloc_n_map(dims);
    const int slice = reloc_slice_length(M), base = blockIdx.y * slice;
    if (base >= M || blockIdx.x * RELOC_THREADS >= N) return;
    const uint4 *mdesc = ((*dims.map_cur & 1) ? mdesc1 : mdesc0) + 2 * (size_t)base;
    const int cnt = min(slice, M - base);
    if (LDS) {
        for (int i = threadIdx.x; i < 2 * cnt; i += RELOC_THREADS) s_desc[i] = mdesc[i];
        __syncthreads();
    }
    const int q = blockIdx.x * RELOC_THREADS + threadIdx.x;
    if (q >= N) return;
    const uint4 d0 = qdesc[2 * (size_t)q], d1 = qdesc[2 * (size_t)q + 1];
    uint32_t b1 = RELOC_NO_KEY, b2 = RELOC_NO_KEY;
    for (int p = 0; p < cnt; p++) {
        const uint4 a0 = LDS ? s_desc[2 * p] : mdesc[2 * p], a1 = LDS ? s_desc[2 * p + 1] : mdesc[2 * p + 1];
        uint32_t d = bcnt_acc(d0.x ^ a0.x, 0u);
        d = bcnt_acc(d0.y ^ a0.y, d), d = bcnt_acc(d0.z ^ a0.z, d), d = bcnt_acc(d0.w ^ a0.w, d);
        d = bcnt_acc(d1.x ^ a1.x, d), d = bcnt_acc(d1.y ^ a1.y, d), d = bcnt_acc(d1.z ^ a1.z, d), d = bcnt_acc(d1.w ^ a1.w, d);
        reloc_top2(b1, b2, d << 16 | (uint32_t)(base + p));
    }
    keys[(size_t)blockIdx.y * N + q] = make_uint2(b1, b2);
}

// the slices' keys of query q folded into its two best
__device__ __forceinline__ void reloc_merge(const uint2 *keys, int N, int M, int q, uint32_t &k1, uint32_t &k2) {
    const int slice = reloc_slice_length(M), slices = (M + slice - 1) / slice;
    uint32_t b1 = RELOC_NO_KEY, b2 = RELOC_NO_KEY;
    for (int s = 0; s < slices; s++) {
        const uint2 k = keys[(size_t)s * N + q];
        reloc_top2(b1, b2, k.x);
        reloc_top2(b1, b2, k.y);
    }
    k1 = b1, k2 = b2;
}

// the stage entry's records: (idx1, d1, idx2, d2), -1 / INT_MAX where there is none -- the format of lvt_amd_hamming_match_batched
__global__ __launch_bounds__(RELOC_THREADS) void k_reloc_merge_records(const uint2 *__restrict__ keys, RelocDims dims, int4 *__restrict__ out) {
    const int N = reloc_n_query(dims), M = reloc_n_map(dims);
    const int q = blockIdx.x * RELOC_THREADS + threadIdx.x;
    if (q >= N) return;
    uint32_t k1, k2;
    reloc_merge(keys, N, M, q, k1, k2);
    int4 r;
    r.x = k1 == RELOC_NO_KEY ? -1 : (int)(k1 & 0xFFFFu), r.y = k1 == RELOC_NO_KEY ? 0x7FFFFFFF : (int)(k1 >> 16);
    r.z = k2 == RELOC_NO_KEY ? -1 : (int)(k2 & 0xFFFFu), r.w = k2 == RELOC_NO_KEY ? 0x7FFFFFFF : (int)(k2 >> 16);
    out[q] = r;
}

// the correspondences of one call, as k_reloc_score and k_reloc_select read them
struct RelocCorr {
    const double *X;     // [n][3] world points
    const float *uv;     // [n][2] observations
    const double *Pc;    // [n][3] camera-frame points (read where has_pc says so)
    const int *with_pc;  // [n3] the correspondences that have a point, ascending
    int n, n3;           // (filled by reloc_sizes from the call's work record)
};
struct RelocCam {
    double fx, fy, cx, cy;
};
// what the call's kernels hand on and the host reads back once
struct RelocWork {
    lvt_amd_reloc_result res;
    double hyp_R[9], hyp_t[3];  // the best hypothesis
    Pose prior;                 // ... as the solver's start pose
    int n_edges;                // its inliers: the solver's edges (0: the call ended before the refinement)
    int success;                // max(min_inliers, min_num_matches_for_tracking)
};

// ---- stage 2 on a handle's own data ---------------------------------------------------------------------------------------------------------------
// the sequence's arrays the call reads, and the call's own buffers
struct RelocSeq {
    const float *x[2], *y[2], *depth;   // Feat::x, y of both eyes, Feat::depth of the left one (RGB-D)
    const uint64_t *desc[2];            // Feat::desc
    const int *n_feat[2];               // Feat::n
    const double *map_pos[2];           // MapSoA::pos of both copies
    const int *map_n, *map_cur;
    const FeatCtl *fc;                  // of the last frame's buffer
};
struct RelocBufs {
    uint2 *keys;        // [32 slices][NF_MAX]
    uint32_t *claim;    // [MAP_MAX] packed (d1, i) of the feature that holds a map point; RELOC_NO_KEY between calls
    int *corr_feat;     // [NF_MAX] feature index of correspondence c
    double *X, *Pc;     // [NF_MAX][3]
    float *uv;          // [NF_MAX][2]
    uint8_t *has_pc;    // [NF_MAX]
    int *with_pc;       // [NF_MAX]
    int *counts;        // [RELOC_HYP_MAX]
    int *inl;           // [NF_MAX]
    double *eX;         // [NF_MAX][3] the solver's own buffers: the frame's pnp_X, pnp_obs, pnp_feat are not touched
    float *eObs;
    double *eErr;       // [2 NF_MAX + 2]
    int8_t *eLevel;
    RelocWork *work;
};
constexpr int RELOC_NO_FEATURES = 9;  // RelocWork::res.status of a call whose last frame was skipped, absent or poisoned: the host refuses

// one workgroup of 1024 threads: the slice merge, the accept rule, the mutual filter (one integer minimum per claimed map point), the ordered compaction
__global__ __launch_bounds__(1024) void k_reloc_corr(RelocSeq S, RelocBufs B, float track_ratio, float desc_th) {
    __shared__ int s_scan[16];
    __shared__ int s_matched;
    RelocWork &w = *B.work;
    const RelocDims dims{S.n_feat[0], S.map_n, S.map_cur, S.fc};
    const int N = reloc_n_query(dims), M = reloc_n_map(dims);
    const bool no_features = load_seq(S.fc->skip_seq) == load_seq(S.fc->feat_seq);  // (frame_without_features for the frame the buffer holds)
    if (threadIdx.x == 0) s_matched = 0;
    __syncthreads();
    const double *pos = S.map_pos[*S.map_cur & 1];
    const int cnt = min(M, 2);
    uint32_t mine[NF_MAX / 1024];
    int idx[NF_MAX / 1024];
#pragma unroll
    for (int k = 0; k < NF_MAX / 1024; k++) {
        const int q = k * 1024 + threadIdx.x;
        mine[k] = RELOC_NO_KEY, idx[k] = -1;
        if (q < N && !no_features) {
            uint32_t k1, k2;
            reloc_merge(B.keys, N, M, q, k1, k2);
            if (accept_match(cnt, k1, k2, track_ratio, desc_th)) {
                idx[k] = (int)(k1 & 0xFFFFu);
                mine[k] = (k1 >> 16) << 16 | (uint32_t)q;
                atomicMin(&B.claim[idx[k]], mine[k]);
                atomicAdd(&s_matched, 1);
            }
        }
    }
    __threadfence();
    __syncthreads();
    bool keep[NF_MAX / 1024];
#pragma unroll
    for (int k = 0; k < NF_MAX / 1024; k++) keep[k] = idx[k] >= 0 && __hip_atomic_load(&B.claim[idx[k]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mine[k];
    __syncthreads();  // every claim has been read: the table goes back to empty where it was touched
    int total = 0;
#pragma unroll
    for (int k = 0; k < NF_MAX / 1024; k++) {
        if (idx[k] >= 0) B.claim[idx[k]] = RELOC_NO_KEY;
        int sum;
        const int c = total + block_excl_scan(keep[k] ? 1 : 0, s_scan, &sum);
        if (keep[k]) {
            const int q = k * 1024 + threadIdx.x, m = idx[k];
            B.corr_feat[c] = q;
            B.X[3 * c] = pos[3 * (size_t)m], B.X[3 * c + 1] = pos[3 * (size_t)m + 1], B.X[3 * c + 2] = pos[3 * (size_t)m + 2];
            B.uv[2 * c] = S.x[0][q], B.uv[2 * c + 1] = S.y[0][q];
        }
        total += sum;
    }
    if (threadIdx.x == 0) {
        w.res.n_features = N, w.res.n_map = M, w.res.n_matched = s_matched, w.res.n_corr = total;
        w.res.status = no_features ? RELOC_NO_FEATURES : -1;
    }
}

// the two smallest keys of a wavefront's lanes, each holding its own two (b1 <= b2); every lane ends with the wave's
__device__ __forceinline__ void reloc_wave_top2(uint32_t &b1, uint32_t &b2) {
    for (int off = 32; off; off >>= 1) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)b1, off), o2 = (uint32_t)__shfl_xor((int)b2, off);
        const uint32_t n1 = min(b1, o1), n2 = min(max(b1, o1), min(b2, o2));
        b1 = n1, b2 = n2;
    }
}

// one wavefront per correspondence, four per workgroup: its camera-frame point from the depth (RGB-D) or from its stereo partner among the right features
__global__ __launch_bounds__(RELOC_THREADS) void k_reloc_points(RelocSeq S, RelocBufs B, Params prm, float min_disparity) {
    const int c = blockIdx.x * (RELOC_THREADS / 64) + __builtin_amdgcn_readfirstlane(wave_id());
    if (c >= B.work->res.n_corr) return;
    const int i = B.corr_feat[c];
    const float xl = S.x[0][i], yl = S.y[0][i];
    double Z = 0.0;
    bool has = false;
    if (prm.sensor == 2) {
        Z = (double)S.depth[i];
        has = true;
    } else {
        const int NR = reloc_n_feat(S.n_feat[1], S.fc, 1);
        const float lo = (float)max((int)yl - ROW_RADIUS, 0), hi = (float)min((int)yl + ROW_RADIUS, prm.H);
        const uint64_t *dl = S.desc[0] + 4 * (size_t)i;
        const uint64_t a0 = dl[0], a1 = dl[1], a2 = dl[2], a3 = dl[3];
        uint32_t b1 = RELOC_NO_KEY, b2 = RELOC_NO_KEY;
        int n_cand = 0;
        for (int j = lane_id(); j < NR; j += 64) {
            const float xr = S.x[1][j], yr = S.y[1][j];
            if (yr >= lo && yr <= hi && (xl - xr) >= min_disparity) {
                const uint64_t *dr = S.desc[1] + 4 * (size_t)j;
                const uint32_t d = (uint32_t)(__popcll(a0 ^ dr[0]) + __popcll(a1 ^ dr[1]) + __popcll(a2 ^ dr[2]) + __popcll(a3 ^ dr[3]));
                reloc_top2(b1, b2, d << 16 | (uint32_t)j);
                n_cand++;
            }
        }
        reloc_wave_top2(b1, b2);
        for (int off = 32; off; off >>= 1) n_cand += __shfl_xor(n_cand, off);
        if (accept_match(min(n_cand, 2), b1, b2, prm.tri_ratio, prm.desc_th)) {
            const float xr = S.x[1][b1 & 0xFFFFu];
            Z = ((double)prm.fx * (double)prm.baseline) / ((double)xl - (double)xr);
            has = true;
        }
    }
    if (lane_id() == 0) {
        B.has_pc[c] = has ? 1 : 0;
        if (has) {
            B.Pc[3 * c] = (((double)xl - (double)prm.cx) * Z) / (double)prm.fx;
            B.Pc[3 * c + 1] = (((double)yl - (double)prm.cy) * Z) / (double)prm.fy;
            B.Pc[3 * c + 2] = Z;
        }
    }
}

// one workgroup of 1024 threads: the correspondences that have a point, in order
__global__ __launch_bounds__(1024) void k_reloc_list(RelocBufs B) {
    __shared__ int s_scan[16];
    RelocWork &w = *B.work;
    const int n = w.res.n_corr;
    int total = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int c = c0 + threadIdx.x;
        const int has = (c < n && B.has_pc[c]) ? 1 : 0;
        int sum;
        const int pos = total + block_excl_scan(has, s_scan, &sum);
        if (has) B.with_pc[pos] = c;
        total += sum;
    }
    if (threadIdx.x == 0) {
        w.res.n_with_point = total;
        if (w.res.status != RELOC_NO_FEATURES) w.res.status = total < 3 ? 1 : -1;
    }
}

// stage 6: what a successful call leaves in the sequence's record.  The device writes it (k_reloc_commit), the host writes the same into its ring.
__host__ __device__ inline void reloc_commit_ctl(Ctl &k, const lvt_amd_reloc_result &r, const ChainWords &cw) {
    const int n = r.n_refined_inliers;
    k.state = 2;
    for (int i = 0; i < 4; i++) k.last_pose.q[i] = k.optimized.q[i] = k.mm_last_q[i] = r.q_wxyz[i], k.mm_ang_vel[i] = i ? 0.0 : 1.0;
    for (int i = 0; i < 3; i++) k.last_pose.p[i] = k.optimized.p[i] = k.mm_last_p[i] = r.p[i], k.mm_lin_vel[i] = 0.0, k.out_t[i] = r.t[i];
    for (int i = 0; i < 9; i++) k.out_R[i] = r.R[i / 3][i % 3];
    k.out_status = 2;
    k.mm_pending = 0;
    k.last_matches[0] = k.last_matches[1] = k.last_matches[2] = n;
    k.early_done = 0, k.early_accepted = 0;
    set_chain(k, cw);  // (k_state.hip: the chain words of a just-reset record, the stamps zero -- what k_state_unpack writes)
}
__global__ __launch_bounds__(64) void k_reloc_commit(Ctl *ctl, const RelocWork *work, ChainWords cw, int dry_run) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || dry_run || work->res.status != 0) return;
    reloc_commit_ctl(*ctl, work->res, cw);
}

// ---- stages 3 - 5 ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t reloc_sample(uint64_t seed, int h, int j, int n3) {
    uint64_t x = seed + (uint64_t)(3 * h + j + 1) * 0x9E3779B97F4A7C15ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x % (uint64_t)n3;
}

// e1, e2, e3 as the rows of E; false: degenerate
__device__ __forceinline__ bool reloc_triad(const double p0[3], const double p1[3], const double p2[3], double E[9]) {
    const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const double n1 = (ax * ax + ay * ay) + az * az;
    if (n1 <= RELOC_DEGENERATE) return false;
    const double l1 = sqrt(n1);
    const double e1x = ax / l1, e1y = ay / l1, e1z = az / l1;
    const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    const double cx = e1y * bz - e1z * by, cy = e1z * bx - e1x * bz, cz = e1x * by - e1y * bx;
    const double n3 = (cx * cx + cy * cy) + cz * cz;
    if (n3 <= RELOC_DEGENERATE) return false;
    const double l3 = sqrt(n3);
    const double e3x = cx / l3, e3y = cy / l3, e3z = cz / l3;
    E[0] = e1x, E[1] = e1y, E[2] = e1z;
    E[3] = e3y * e1z - e3z * e1y, E[4] = e3z * e1x - e3x * e1z, E[5] = e3x * e1y - e3y * e1x;
    E[6] = e3x, E[7] = e3y, E[8] = e3z;
    return true;
}

// hypothesis h: false scores 0 (coincident samples, a degenerate triad)
__device__ __forceinline__ bool reloc_hypothesis(const RelocCorr &c, uint64_t seed, int h, double R[9], double t[3]) {
    const int s0 = (int)reloc_sample(seed, h, 0, c.n3), s1 = (int)reloc_sample(seed, h, 1, c.n3), s2 = (int)reloc_sample(seed, h, 2, c.n3);
    if (s0 == s1 || s0 == s2 || s1 == s2) return false;
    const int i0 = c.with_pc[s0], i1 = c.with_pc[s1], i2 = c.with_pc[s2];
    double a[3][3], b[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a[0][k] = c.Pc[3 * i0 + k], a[1][k] = c.Pc[3 * i1 + k], a[2][k] = c.Pc[3 * i2 + k];
        b[0][k] = c.X[3 * i0 + k], b[1][k] = c.X[3 * i1 + k], b[2][k] = c.X[3 * i2 + k];
    }
    double Ea[9], Eb[9];
    if (!reloc_triad(a[0], a[1], a[2], Ea) || !reloc_triad(b[0], b[1], b[2], Eb)) return false;
    double ma[3], mb[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ma[k] = ((a[0][k] + a[1][k]) + a[2][k]) / 3.0;
        mb[k] = ((b[0][k] + b[1][k]) + b[2][k]) / 3.0;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = (Eb[i] * Ea[j] + Eb[3 + i] * Ea[3 + j]) + Eb[6 + i] * Ea[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = mb[i] - ((R[3 * i] * ma[0] + R[3 * i + 1] * ma[1]) + R[3 * i + 2] * ma[2]);
    return true;
}

__device__ __forceinline__ bool reloc_inlier(const RelocCorr &c, const RelocCam &cam, const double R[9], const double t[3], double gate, int i) {
    const double dx = c.X[3 * i] - t[0], dy = c.X[3 * i + 1] - t[1], dz = c.X[3 * i + 2] - t[2];
    const double px = (R[0] * dx + R[3] * dy) + R[6] * dz;
    const double py = (R[1] * dx + R[4] * dy) + R[7] * dz;
    const double pz = (R[2] * dx + R[5] * dy) + R[8] * dz;
    const double ex = ((cam.fx * px) / pz + cam.cx) - (double)c.uv[2 * i];
    const double ey = ((cam.fy * py) / pz + cam.cy) - (double)c.uv[2 * i + 1];
    return pz > 0.0 && (ex * ex + ey * ey) <= gate;  // (false for NaN)
}

// one wavefront per hypothesis, four per workgroup
__global__ __launch_bounds__(RELOC_THREADS) void k_reloc_score(RelocCorr c, const RelocWork *__restrict__ work, RelocCam cam, uint64_t seed, double gate,
                                                               int n_hyp, int *__restrict__ counts) {
    c.n = work->res.n_corr, c.n3 = work->res.n_with_point;
    const int h = blockIdx.x * (RELOC_THREADS / 64) + __builtin_amdgcn_readfirstlane(wave_id());
    if (h >= n_hyp) return;
    double R[9], t[3];
    int cnt = 0;
    if (c.n3 >= 3 && reloc_hypothesis(c, seed, h, R, t)) {
        for (int i0 = 0; i0 < c.n; i0 += 64) {
            const int i = i0 + lane_id();
            cnt += __popcll(__ballot(i < c.n && reloc_inlier(c, cam, R, t, gate, i)));
        }
    }
    if (lane_id() == 0) counts[h] = cnt;
}

// rotation matrix -> quaternion (w, x, y, z): lvt_odometry.h's mat3_to_quat, the branch on the trace / largest diagonal element
__device__ __forceinline__ void reloc_mat3_to_quat(const double R[9], double q[4]) {
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0) {
        const double s = sqrt(tr + 1.0), r = 0.5 / s;
        q[0] = 0.5 * s;
        q[1] = (R[7] - R[5]) * r, q[2] = (R[2] - R[6]) * r, q[3] = (R[3] - R[1]) * r;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        const double s = sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0), r = 0.5 / s;
        q[1 + i] = 0.5 * s;
        q[0] = (R[3 * k + j] - R[3 * j + k]) * r;
        q[1 + j] = (R[3 * j + i] + R[3 * i + j]) * r;
        q[1 + k] = (R[3 * k + i] + R[3 * i + k]) * r;
    }
}

// one workgroup.  inl: [n] the inlier list (correspondence indices, ascending); eX / eObs: the solver's edges
__global__ __launch_bounds__(RELOC_THREADS) void k_reloc_select(RelocCorr c, RelocCam cam, uint64_t seed, double gate, int n_hyp, const int *__restrict__ counts,
                                                                RelocWork *__restrict__ work, int *__restrict__ inl, double *__restrict__ eX,
                                                                float *__restrict__ eObs) {
    __shared__ int s_wave[RELOC_THREADS / 64];
    __shared__ int s_scan[16];
    RelocWork &w = *work;
    c.n = w.res.n_corr, c.n3 = w.res.n_with_point;
    if (c.n3 < 3) {  // status 1 (or a frame without features) stands in the record already; nothing to select
        if (threadIdx.x == 0) w.n_edges = 0;
        return;
    }
    // arg-max: count << 10 | (1023 - h), so the larger key is the larger count, then the lower h
    int key = -1;
    for (int h = threadIdx.x; h < n_hyp; h += RELOC_THREADS) key = max(key, counts[h] << 10 | (RELOC_HYP_MAX - 1 - h));
    for (int off = 32; off; off >>= 1) key = max(key, __shfl_xor(key, off));
    if (lane_id() == 0) s_wave[wave_id()] = key;
    __syncthreads();
    key = max(max(s_wave[0], s_wave[1]), max(s_wave[2], s_wave[3]));
    const int best = RELOC_HYP_MAX - 1 - (key & (RELOC_HYP_MAX - 1)), best_cnt = key >> 10;
    const bool enough = best_cnt >= w.success;
    double R[9], t[3];
    const bool ok = reloc_hypothesis(c, seed, best, R, t);
    int total = 0;
    if (enough && ok) {  // (enough implies ok: a hypothesis that scores 0 is never enough, success >= 3)
        for (int i0 = 0; i0 < c.n; i0 += RELOC_THREADS) {
            const int i = i0 + threadIdx.x;
            const int in = (i < c.n && reloc_inlier(c, cam, R, t, gate, i)) ? 1 : 0;
            int sum;
            const int pos = total + block_excl_scan(in, s_scan, &sum);
            if (in) {
                inl[pos] = i;
                eX[3 * pos] = c.X[3 * i], eX[3 * pos + 1] = c.X[3 * i + 1], eX[3 * pos + 2] = c.X[3 * i + 2];
                eObs[2 * pos] = c.uv[2 * i], eObs[2 * pos + 1] = c.uv[2 * i + 1];
            }
            total += sum;
        }
    }
    if (threadIdx.x == 0) {
        w.res.best_hypothesis = best;
        w.res.n_hyp_inliers = best_cnt;
        w.n_edges = total;
        if (!enough || !ok) {
            w.res.status = 2;
        } else {
            for (int k = 0; k < 9; k++) w.hyp_R[k] = R[k];
            for (int k = 0; k < 3; k++) w.hyp_t[k] = t[k], w.prior.p[k] = t[k];
            reloc_mat3_to_quat(R, w.prior.q);
        }
    }
}

// the refinement: k_pnp's own solver on the edges above; the call's result record is complete behind it
__global__ __launch_bounds__(PNP_THREADS) void k_reloc_refine(Params prm, RelocWork *work, const double *X, const float *obs, double *err, int8_t *level) {
    __shared__ PnpShared sh;
    __shared__ double red[PNP_RED];
    extern __shared__ __attribute__((aligned(16))) uint8_t pnp_dyn[];
    RelocWork &w = *work;
    const int n = w.n_edges;
    if (n <= 0) return;  // status 1 or 2
    const Pose prior = w.prior;
    for (int i = threadIdx.x; i < n; i += PNP_THREADS) level[i] = 0;
    if (threadIdx.x == 0) sh.trace = nullptr, sh.trace_cap = 0;
    __syncthreads();
    Pose res;
    int inliers, calls, borderline;
    pnp_solve(prm, prior, X, obs, err, level, n, sh, red, pnp_dyn, res, inliers, calls, borderline, nullptr, false);
    if (threadIdx.x == 0) {
        bool finite = true;
        for (int k = 0; k < 4; k++) finite = finite && isfinite(res.q[k]);
        for (int k = 0; k < 3; k++) finite = finite && isfinite(res.p[k]);
        w.res.n_refined_inliers = inliers;
        w.res.status = (finite && inliers >= w.success) ? 0 : 3;
        for (int k = 0; k < 4; k++) w.res.q_wxyz[k] = res.q[k];
        for (int k = 0; k < 3; k++) w.res.p[k] = res.p[k];
        double R[9], t[3];
        pose_to_Rt(res, R, t);
        for (int k = 0; k < 9; k++) w.res.R[k / 3][k % 3] = R[k];
        for (int k = 0; k < 3; k++) w.res.t[k] = t[k];
    }
}

}  // namespace lvt
