// k_labelmask.hip -- per-frame label masks: a segmentation image that travels with a frame is turned into the u8 plane k_mask_features filters that eye of that
// frame with (lvt_amd_set_label_mask, lvt_amd_frame_labels*; include/lvt_amd_ext.h has the definition under LABEL MASKS, tests/label_mask_util.py restates it
// in numpy).  ONE launch at the head of the feature stage, beside the other properties' launches; no existing kernel body changes: k_mask_features is handed the
// built plane through its host-filled MaskTable.
//   k_label_mask : a workgroup of 256 threads owns a 32 x 32 tile of the destination; blockIdx.y is the image, the grid's x extent follows the largest image of
//                  the launch and surplus workgroups leave at the top.
//     1. 64 threads compute lx() of the tile's columns and 64 ly() of its rows, halo included, into LDS: the only integer divisions, one per thread.
//     2. dilate == 0: every thread looks up the four pixels of its word -- no halo, no ballot.
//        dilate  > 0: the tile plus its halo is at most 62 x 62, so ONE WAVE'S LANES ARE ONE ROW: lane i fetches the label under column x0 - dilate + i (a few
//        distinct bytes per row under upsampling: they coalesce), tests the drop set (eight words in LDS) and a ballot packs the row's f0 into 64 bits.  The
//        row OR is taken on that word with shifts by doubling (uniform per wave: scalar instructions), the column OR by each thread over the 2 dilate + 1 words
//        above and below its row (LDS reads the eight threads of a row share): 2 dilate + 1 LDS reads per WORD instead of (2 dilate + 1)^2 loads per pixel.
//     3. AND with the static mask where there is one, and one 32-bit store per thread, numbered over the destination pitch with the padding columns zero
//        (as k_gray_frames and k_clahe_apply store).
//   Why 32 x 32: with the largest halo the staged row still fits the 64 lanes of a wave, which makes the ballot the packing step; a 64 x 16 tile was NOT tried
//   (it needs two ballots per row with the second one less than half full).  A row of the tile is a 32-byte store segment.
// Loads: label bytes at lab[ly][lx] with lx < label_width, ly < label_height only for pixels inside the image; static bytes at [y][x] with x < W, y < H only;
// stores only to words < dst_pitch / 4 of rows < H.  No scratch.
#include "lvt_dev.h"

namespace lvt {

struct LabelImg {
    const uint8_t *lab;   // the label image: u8, any address, lab_pitch >= lw bytes per row
    const uint8_t *stat;  // the eye's static mask on the destination grid (!= 0: allowed), any address, stat_pitch >= W; NULL: none
    uint8_t *dst;         // the plane: 4-byte aligned, dst_pitch a multiple of 4 and >= W; 255: key points allowed, 0: forbidden or padding
    int lab_pitch, lw, lh, stat_pitch, dst_pitch, W, H, dilate;
    uint32_t drop[8];     // bit l: label l forbids key points
};
constexpr int LABEL_PACK = 32;  // images per launch (2 816 bytes of arguments); more take a further launch
struct LabelTable {
    LabelImg im[LABEL_PACK];
};
static_assert(sizeof(LabelTable) + 64 < 4096, "k_label_mask's arguments must stay under 4096 bytes");
constexpr int LABEL_TILE = 32, LABEL_MAX_DILATE = 15;
static_assert(LABEL_TILE + 2 * LABEL_MAX_DILATE <= 64, "a staged row is one wave's ballot");

// bit i of the result: OR of bits i ... i + n - 1 of m (n >= 1), by doubling
__device__ __forceinline__ unsigned long long or_window(unsigned long long m, int n) {
    int w = 1;
    while (2 * w <= n) m |= m >> w, w *= 2;
    return m | (m >> (n - w));
}

__global__ __launch_bounds__(256) void k_label_mask(LabelTable tab) {
    const LabelImg &I = tab.im[blockIdx.y];   // (uniform index: the descriptor stays in scalar registers)
    const int wpr = I.dst_pitch >> 2;         // words per destination row
    const int tiles_x = (wpr + 7) >> 3, tiles_y = (I.H + LABEL_TILE - 1) / LABEL_TILE;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int x0 = ((int)blockIdx.x % tiles_x) * LABEL_TILE, y0 = ((int)blockIdx.x / tiles_x) * LABEL_TILE;
    const int r = I.dilate, tid = threadIdx.x;
    __shared__ int s_lx[64], s_ly[64];            // label column / row under staged column / row i (x0 - r + i, y0 - r + i); -1: outside the image
    __shared__ uint32_t s_drop[8];
    __shared__ unsigned long long s_row[64];      // staged row j: bit i = OR of f0 over columns x0 + i - r ... x0 + i + r of row y0 - r + j
    if (tid < 64) {
        const int x = x0 - r + tid;
        s_lx[tid] = (x >= 0 && x < I.W) ? (int)((unsigned)(x * I.lw) / (unsigned)I.W) : -1;   // (products stay below 2^27)
    } else if (tid < 128) {
        const int y = y0 - r + (tid - 64);
        s_ly[tid - 64] = (y >= 0 && y < I.H) ? (int)((unsigned)(y * I.lh) / (unsigned)I.H) : -1;
    } else if (tid == 128) {
#pragma unroll
        for (int k = 0; k < 8; k++) s_drop[k] = I.drop[k];
    }
    __syncthreads();
    const int wx = tid & 7, wy = tid >> 3;   // the thread's word of the tile: columns x0 + 4 wx ... + 3 of row y0 + wy
    uint32_t f = 0;                          // bit k: pixel k of the word is forbidden
    if (r == 0) {
        const int ly = s_ly[wy];
        if (ly >= 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int lx = s_lx[4 * wx + k];
                if (lx < 0) continue;
                const uint32_t l = I.lab[(size_t)ly * I.lab_pitch + lx];
                f |= ((s_drop[l >> 5] >> (l & 31)) & 1u) << k;
            }
        }
    } else {
        const int rows = LABEL_TILE + 2 * r, lane = tid & 63, n = 2 * r + 1;
        const int lx = lane < rows ? s_lx[lane] : -1;
        // A load and its ballot per turn.  A second form that sent all of a wave's (up to 16) label loads out ahead of the first ballot, fully unrolled, was
        // built and measured as well: 12.2 / 16.9 us against this loop's 12.3 / 17.2 for a KITTI-shaped pair at dilate 4 / 15, 75 against 69 us for a batch of 16
        // at dilate 4, with 28 VGPRs and 58 SGPRs instead of 22 and 38 -- no gain, so the loop stays (profiles/label_masks.md has this form's figures).
        for (int j = tid >> 6; j < rows; j += 4) {   // (j is uniform in a wave: every lane takes part in the ballot)
            const int ly = s_ly[j];
            bool f0 = false;
            if (ly >= 0 && lx >= 0) {
                const uint32_t l = I.lab[(size_t)ly * I.lab_pitch + lx];
                f0 = (s_drop[l >> 5] >> (l & 31)) & 1u;
            }
            const unsigned long long m = or_window(__ballot(f0), n);
            if (lane == 0) s_row[j] = m;
        }
        __syncthreads();
        unsigned long long v = 0;
        for (int k = 0; k < n; k++) v |= s_row[wy + k];
        f = (uint32_t)(v >> (4 * wx)) & 15u;
    }
    const int x = x0 + 4 * wx, y = y0 + wy;
    if (y >= I.H || (x >> 2) >= wpr) return;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x + k >= I.W) continue;   // padding columns stay zero
        bool allowed = !((f >> k) & 1u);
        if (allowed && I.stat) allowed = I.stat[(size_t)y * I.stat_pitch + x + k] != 0;
        word |= (allowed ? 255u : 0u) << (8 * k);
    }
    reinterpret_cast<uint32_t *>(I.dst + (size_t)y * I.dst_pitch)[x >> 2] = word;
}

}  // namespace lvt
