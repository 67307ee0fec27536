// k_depthguard.hip -- depth guard: RGB-D key points whose depth sample has too little support in its neighbourhood are dropped inside the feature stage
// (lvt_amd_set_depth_guard; include/lvt_amd_ext.h has the definition under DEPTH GUARD, tests/depth_guard_util.py restates it in numpy).  ONE launch directly
// behind k_gather, which writes the Feat arrays and *F.n from ONE pixel of the depth plane per key point, and ahead of k_mask_features, k_brief and k_brief_img,
// which read them: no existing kernel body changes, and a handle that never set a guard launches exactly what it did.
//   k_depth_guard : one workgroup of 1024 threads per sequence, in the shape of k_mask_features.  The walk and its in-place compaction are compact_features
//                   (lvt_dev.h, which says why it is safe).  The rule reads the sample under k_gather's own pixel again (depth_sample, the function k_gather
//                   calls) and the (2r+1)^2 - 1 samples around it and counts those that are valid and within the tolerance of the centre; F.depth keeps the
//                   centre sample k_gather stored.  Thread 0 stores FeatCtl::guard_kept / guard_dropped.
// A THREAD PER FEATURE, not a few lanes per feature with a cross-lane sum.  The window's loads do not depend on one another and the radius is a template
// argument, so a thread's 8 / 24 / 48 loads unroll, and a frame's <= 4096 features are <= 4 chunks of 16 waves.  What the launch costs is the fetch of the
// window's cache lines through ONE compute unit -- a feature's window spans 3 / 5 / 7 rows of the plane, each another line, and k_gather has pulled only the
// centre's --, so radius 3 takes about three times radius 1 (profiles/depth_guard.md has the figures).  A row per
// lane would fetch the same lines through the same compute unit with MORE wave-level loads (3 rows on 4 lanes leave a quarter of every wave idle, 7 rows on 8
// lanes an eighth; 4096 features become 16 / 32 passes of the workgroup instead of 4, each with its scan and its two barriers) and add the reduction's DPP
// steps.  A form of this kernel whose loads were all unconditional (positions clamped into the plane, the format a second template argument: 86 VGPRs) measured
// the same (the profile's last section), so the plainer form stands.  Only the thread-per-feature shape was built.
// The per-sequence records travel BY VALUE like MaskTable: blockIdx.z is the slot, slot k belongs to sequence z0 + k, and a sequence without a guard (or
// without a frame in this step) has radius 0 -- the host writes every slot of every table -- and leaves at the top.  No scratch.
#include "lvt_dev.h"

namespace lvt {

struct GuardSeq {
    int radius, min_support;  // radius 0: the sequence has no guard
    float tol_abs, tol_rel;
};
constexpr int GUARD_PACK = 32;  // sequences per launch (512 bytes of arguments); a batch with more takes further launches
struct GuardTable {
    GuardSeq s[GUARD_PACK];
};
static_assert(sizeof(GuardTable) + 64 < 4096, "k_depth_guard's arguments must stay under 4096 bytes");

// the depth plane k_gather sampled, with its format, and the sequence's depth range
struct GuardPlane {
    const float *img;  // float or uint16_t elements (fmt)
    int pitch, fmt;    // elements / DEPTH_F32, DEPTH_U16
    float scale, near_plane, far_plane;
    int W, H;
};
// the sample k_gather reads at element i
__device__ __forceinline__ float guard_sample(const GuardPlane &P, size_t i) { return depth_sample(P.img, P.fmt, P.scale, i); }
__device__ __forceinline__ bool guard_valid(const GuardPlane &P, float s) { return P.near_plane <= s && s <= P.far_plane; }  // (a NaN fails both)

// the support of the sample d_c at pixel (cx, cy), inside the plane: the window's samples other than the centre that lie inside the plane, are valid and within
// t of d_c.  R is a template argument so that the loop unrolls and every load is issued before the first is waited for
template <int R>
__device__ __forceinline__ int guard_support(const GuardPlane &P, int cx, int cy, float d_c, float t) {
    int support = 0;
#pragma unroll
    for (int dy = -R; dy <= R; dy++)
#pragma unroll
        for (int dx = -R; dx <= R; dx++) {
            if (dx == 0 && dy == 0) continue;
            const int px = cx + dx, py = cy + dy;
            if (px < 0 || px >= P.W || py < 0 || py >= P.H) continue;  // (the window is clipped at the plane's border: no load outside it)
            const float s = guard_sample(P, (size_t)py * P.pitch + px);
            support += (guard_valid(P, s) && fabsf(__fsub_rn(s, d_c)) <= t) ? 1 : 0;
        }
    return support;
}
// the rule.  The pixel is k_gather's own, (int)bx, decided on the float so that no conversion leaves the range of an int: truncation sends exactly the values
// in (-1, W) to 0 ... W - 1 (a NaN fails both tests)
__device__ __forceinline__ bool guard_keep(const GuardPlane &P, const GuardSeq &G, float bx, float by) {
    if (!(bx > -1.0f && bx < (float)P.W && by > -1.0f && by < (float)P.H)) return false;
    const int cx = (int)bx, cy = (int)by;
    const float d_c = guard_sample(P, (size_t)cy * P.pitch + cx);
    if (!guard_valid(P, d_c)) return false;
    const float t = __fadd_rn(G.tol_abs, __fmul_rn(G.tol_rel, d_c));
    const int support = G.radius == 1 ? guard_support<1>(P, cx, cy, d_c, t) : G.radius == 2 ? guard_support<2>(P, cx, cy, d_c, t) : guard_support<3>(P, cx, cy, d_c, t);
    return support >= G.min_support;
}

__global__ __launch_bounds__(1024) void k_depth_guard(const Seq *seqs, GuardTable tab, int par, int z0) {
    const GuardSeq &G = tab.s[blockIdx.z];   // (uniform index: the record stays in scalar registers)
    if (G.radius < 1 || G.radius > 3) return;
    const Seq &S = seq_const(seqs, z0 + blockIdx.z);
    if (S.prm.sensor != 2) return;
    const FrameBuf &FB = S.fb[par];
    FeatCtl &ctl = *FB.fc;
    if (ctl.poison) return;
    __shared__ int scan[16];
    const Feat &F = FB.feat[0];
    GuardPlane P;
    P.img = ctl.in.depth_img, P.pitch = ctl.in.depth_pitch, P.fmt = ctl.in.depth_format, P.scale = ctl.in.depth_scale;
    P.near_plane = S.prm.near_plane, P.far_plane = S.prm.far_plane;
    P.W = S.prm.W, P.H = S.prm.H;
    int n_in;
    const int n_out = compact_features(F, scan, &n_in, [&](float bx, float by) { return guard_keep(P, G, bx, by); });
    if (threadIdx.x == 0) ctl.guard_kept = n_out, ctl.guard_dropped = n_in - n_out;
}

}  // namespace lvt
