// k_mask.hip -- feature masks: key points on masked pixels are dropped inside the feature stage (lvt_amd_set_mask; include/lvt_amd_ext.h has the definition,
// tests/mask_util.py restates it in numpy).  ONE launch at the seam between k_gather, which writes the Feat arrays and *F.n, and k_brief / k_brief_img, which
// read them: no existing kernel body changes, and a handle that never set a mask launches exactly what it did.
//   k_mask_features : one workgroup of 1024 threads per (sequence, eye).  The walk and its in-place compaction are compact_features (lvt_dev.h, which says why
//                     it is safe).  The rule fetches the mask byte under the pixel BRIEF samples at (an ordinary load: the kept corners of a frame touch a few
//                     thousand scattered bytes of a plane that stays in L2 from frame to frame).  Thread 0 stores the eye's kept / dropped counts
//                     (FeatCtl::mask_kept / mask_dropped).
// The per-sequence mask pointers and pitches travel BY VALUE like GrayTable / RectTable: blockIdx.z is the slot, slot k belongs to sequence z0 + k, and a
// sequence or an eye without a mask has a NULL pointer and leaves at the top.  No scratch.
#include "lvt_dev.h"

namespace lvt {

struct MaskSeq {
    const uint8_t *mask[2];  // u8 planes on the detector's pixel grid, != 0: key points allowed; NULL: the eye has no mask
    int pitch[2];            // bytes per row, >= W
};
constexpr int MASK_PACK = 32;  // sequences per launch (768 bytes of arguments); a batch with more takes further launches
struct MaskTable {
    MaskSeq s[MASK_PACK];
};
static_assert(sizeof(MaskTable) + 64 < 4096, "k_mask_features' arguments must stay under 4096 bytes");

// the rule (cv::KeyPointsFilter::runByPixelsMask): ix = (int)(bx + 0.5f), fp32, truncation; keep = 0 <= ix < W && 0 <= iy < H && mask[iy][ix] != 0.
// Decided on the fp32 sum so that no conversion leaves the range of an int: truncation sends exactly the sums in (-1, W) to 0 ... W - 1 (a NaN fails both tests)
__device__ __forceinline__ bool mask_keep(const uint8_t *mask, int pitch, int W, int H, float bx, float by) {
    const float fx = bx + 0.5f, fy = by + 0.5f;
    if (!(fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H)) return false;
    return mask[(size_t)(int)fy * pitch + (int)fx] != 0;
}

__global__ __launch_bounds__(1024) void k_mask_features(const Seq *seqs, MaskTable tab, int par, int z0) {
    const MaskSeq &M = tab.s[blockIdx.z];   // (uniform index: the descriptor stays in scalar registers)
    const int eye = blockIdx.y;
    const uint8_t *mask = eye ? M.mask[1] : M.mask[0];
    if (!mask) return;
    const int pitch = eye ? M.pitch[1] : M.pitch[0];
    const Seq &S = seq_const(seqs, z0 + blockIdx.z);
    if (eye == 1 && S.prm.sensor == 2) return;
    const FrameBuf &FB = S.fb[par];
    FeatCtl &ctl = *FB.fc;
    if (ctl.poison) return;
    __shared__ int scan[16];
    const Feat &F = FB.feat[eye];
    const int W = S.prm.W, H = S.prm.H;
    int n_in;
    const int n_out = compact_features(F, scan, &n_in, [&](float bx, float by) { return mask_keep(mask, pitch, W, H, bx, by); });
    if (threadIdx.x == 0) ctl.mask_kept[eye] = n_out, ctl.mask_dropped[eye] = n_in - n_out;
}

}  // namespace lvt
