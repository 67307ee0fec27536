// k_poseinfo.hip -- pose uncertainty: the information matrix of a frame's 2D-3D edges at the PUBLISHED pose and its inverse
// (include/lvt_amd_ext.h, "POSE UNCERTAINTY").  k_pnp keeps neither its last system (it may belong to a rejected
// trial) nor its errors and levels, so the matrix is evaluated once more, in one pass over the edges, by a kernel of its own behind it.
//   perturbation  xi = (dp, dtheta): p <- p + dp (world axes, metres), R <- R Exp([dtheta]x) (camera axes, radians)
//   edge          pc = R^T (X - p), e = (fx pcx / pcz + cx - u, fy pcy / pcz + cy - v)
//   inlier        pcz > 0 and e.e <= 5.991 (false for NaN);  weight w = 1 / (1 + e.e / 5.991): the solver's Cauchy kernel, rho' only
//   J = de/dxi    de/dpc = [fx / pcz, 0, -fx pcx / pcz^2; 0, fy / pcz, -fy pcy / pcz^2],  dpc/dp = -R^T,  dpc/dtheta = [pc]x
//   info = sum over inliers of w J^T J,  cov = info^-1 (LDL^T, six back-substitutions)
// fp64, IEEE divisions, no contraction (the file is compiled with -ffp-contract=off like the rest of the library).  One pass: nothing is staged in LDS
// beyond the reduction, no scratch.  The sums are those of block_sum<28> (k_track.hip): a fixed tree, so a sequence's record does not depend on the
// batch it rides in.
// Included by lvt_host.hip behind k_track.hip, whose block_sum / PNP_RED it uses.
#pragma once
#include "lvt_dev.h"
#include "lvt_math.h"
#include "../../include/lvt_amd_ext.h"

namespace lvt {

constexpr int PI_THREADS = PNP_THREADS;  // block_sum's tree is written for four wavefronts
constexpr int PI_WORDS = (int)(sizeof(lvt_amd_pose_info) / 8);
static_assert(sizeof(lvt_amd_pose_info) % 8 == 0, "the record travels as 8-byte words");
constexpr double PI_PIVOT_REL = 1e-12;   // a pivot below this share of its diagonal element is the noise of a sum of <= 4096 fp64 terms, not information
constexpr double PI_BORDER = 1e-6;

// thread 0: info (symmetric, from the packed upper triangle), then cov by LDL^T with the pivot test; false: degenerate (cov stays zero)
__device__ __forceinline__ bool pose_info_invert(const double *tri, double *info, double *cov) {
    double A[6][6], d[6];
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int c = a; c < 6; c++, k++) {
                A[c][a] = tri[k];
                info[6 * a + c] = info[6 * c + a] = tri[k];
            }
        }
    }
    double diag[6];
#pragma unroll
    for (int a = 0; a < 6; a++) diag[a] = A[a][a];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {  // right-looking: A's strict lower triangle becomes L, d the pivots
        d[j] = A[j][j];
        ok = ok && (d[j] > PI_PIVOT_REL * diag[j]) && isfinite(d[j]);  // (false for NaN)
        double cj[6];
#pragma unroll
        for (int i = j + 1; i < 6; i++) cj[i] = A[i][j], A[i][j] = cj[i] / d[j];
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
#pragma unroll
            for (int k2 = j + 1; k2 <= i; k2++) A[i][k2] = A[i][k2] - A[i][j] * cj[k2];
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int c = 0; c < 6; c++) {  // column c of the inverse: L y = e_c, z = y / d, L^T x = z
        double y[6], x[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double v = (i == c) ? 1.0 : 0.0;
#pragma unroll
            for (int k2 = 0; k2 < i; k2++) v = v - A[i][k2] * y[k2];
            y[i] = v;
        }
#pragma unroll
        for (int i = 5; i >= 0; i--) {
            double v = y[i] / d[i];
#pragma unroll
            for (int k2 = 5; k2 > i; k2--) v = v - A[k2][i] * x[k2];
            x[i] = v;
        }
#pragma unroll
        for (int r = 0; r <= c; r++) cov[6 * r + c] = cov[6 * c + r] = x[r];  // one triangle fills the other: exactly symmetric
    }
    return true;
}

// the whole evaluation, called by every thread of a PI_THREADS workgroup; rec: the record in LDS, complete for every thread on return
__device__ __forceinline__ void pose_info_body(const Params &prm, const Pose &pose, const double *__restrict__ X, const float *__restrict__ obs, int n, int frame,
                                               double *red, double *tri, lvt_amd_pose_info &rec) {
    const int tid = threadIdx.x;
    const double fx = prm.fx, fy = prm.fy, cx = prm.cx, cy = prm.cy;
    double R[9];
    q_to_R(pose.q, R);
    const double px = pose.p[0], py = pose.p[1], pz = pose.p[2];
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += PI_THREADS) {
        const double dx = X[3 * i] - px, dy = X[3 * i + 1] - py, dz = X[3 * i + 2] - pz;
        const double pcx = (R[0] * dx + R[3] * dy) + R[6] * dz;
        const double pcy = (R[1] * dx + R[4] * dy) + R[7] * dz;
        const double pcz = (R[2] * dx + R[5] * dy) + R[8] * dz;
        const double e0 = (fx * pcx / pcz + cx) - (double)obs[2 * i], e1 = (fy * pcy / pcz + cy) - (double)obs[2 * i + 1];
        const double e2 = e0 * e0 + e1 * e1;
        if (fabs(e2 - REPROJ_TH2) < PI_BORDER) acc[24] += 1.0;
        if (pcz > 0 && e2 <= REPROJ_TH2) {  // (both false for NaN)
            const double aux = 1.0 + e2 / REPROJ_TH2;
            const double w = 1.0 / aux;
            const double g0x = fx / pcz, g0z = -(fx * pcx) / (pcz * pcz);
            const double g1y = fy / pcz, g1z = -(fy * pcy) / (pcz * pcz);
            double J0[6], J1[6];
#pragma unroll
            for (int c = 0; c < 3; c++) {  // de/dpc (-R^T): column c of R^T is row c of R
                J0[c] = -(g0x * R[3 * c] + g0z * R[3 * c + 2]);
                J1[c] = -(g1y * R[3 * c + 1] + g1z * R[3 * c + 2]);
            }
            // de/dpc [pc]x,  [pc]x = [0 -z y; z 0 -x; -y x 0]
            J0[3] = -(g0z * pcy), J0[4] = g0z * pcx - g0x * pcz, J0[5] = g0x * pcy;
            J1[3] = g1y * pcz - g1z * pcy, J1[4] = g1z * pcx, J1[5] = -(g1y * pcx);
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int c = a; c < 6; c++, k++) acc[k] += w * (J0[a] * J0[c] + J1[a] * J1[c]);
            }
            acc[21] += REPROJ_TH2 * log(aux);
            acc[22] += e2;
            acc[23] += 1.0;
        }
    }
    const bool wave_active = (int)(tid & ~63u) < n;
    block_sum<28>(acc, red, tri, wave_active);  // (two barriers: tri is complete behind it)
    double *words = reinterpret_cast<double *>(&rec);
    for (int i = tid; i < PI_WORDS; i += PI_THREADS) words[i] = 0.0;
    __syncthreads();
    if (tid == 0) {
        rec.chi2 = tri[21], rec.sq_err = tri[22];
        rec.n_edges = n, rec.n_inliers = (int)tri[23], rec.n_borderline = (int)tri[24];
        rec.frame = frame;
        const bool ok = pose_info_invert(tri, rec.info, rec.cov) && rec.n_inliers >= 3;
        if (!ok)
            for (int k = 0; k < 36; k++) rec.cov[k] = 0.0;
        rec.status = ok ? 1 : 2;
    }
    __syncthreads();
}

// the record leaves for the caller's memory as 8-byte words, one per thread
__device__ __forceinline__ void pose_info_store(const lvt_amd_pose_info &rec, lvt_amd_pose_info *out) {
    const double *src = reinterpret_cast<const double *>(&rec);
    double *dst = reinterpret_cast<double *>(out);
    for (int i = threadIdx.x; i < PI_WORDS; i += PI_THREADS) dst[i] = src[i];
    __threadfence_system();
}

// One workgroup per sequence, on the tracking stream directly behind k_pnp: every input (pnp_X / pnp_obs / n_matches by k_track_mid, optimized by k_pnp) was
// written on that stream and its next writer is the next frame's chain behind this launch.  Writes its record (a slot of the pinned ring) and nothing else: the
// frame's completion flag is released by a later kernel of the same stream, so the record is visible to whoever has seen the flag.
template <bool BV>
__global__ __launch_bounds__(PI_THREADS) void k_pose_info(SeqArg<BV> sa, lvt_amd_pose_info *out) {
    const Seq &S = sa.get();
    const Ctl &ctl = *S.ctl;
    __shared__ lvt_amd_pose_info rec;
    __shared__ double red[PNP_RED];
    __shared__ double tri[28];
    if (!ctl.active || ctl.first_frame || ctl.lost_now) {  // block-uniform: no pose of this frame's own -> status 0
        double *words = reinterpret_cast<double *>(&rec);
        for (int i = threadIdx.x; i < PI_WORDS; i += PI_THREADS) words[i] = 0.0;
        __syncthreads();
        if (threadIdx.x == 0) rec.frame = ctl.counts[C_FRAME];
        __syncthreads();
    } else
        pose_info_body(S.prm, ctl.optimized, S.pnp_X, S.pnp_obs, min(ctl.n_matches, NF_MAX), ctl.counts[C_FRAME], red, tri, rec);
    pose_info_store(rec, out + blockIdx.z);
}

// stand-alone entry for differential tests (lvt_amd_pose_info_eval): the same device function on caller data; out is device memory
__global__ __launch_bounds__(PI_THREADS) void k_pose_info_standalone(Params prm, Pose pose, const double *X, const float *obs, int n, lvt_amd_pose_info *out) {
    __shared__ lvt_amd_pose_info rec;
    __shared__ double red[PNP_RED];
    __shared__ double tri[28];
    pose_info_body(prm, pose, X, obs, n, 0, red, tri, rec);
    pose_info_store(rec, out);
}

}  // namespace lvt
