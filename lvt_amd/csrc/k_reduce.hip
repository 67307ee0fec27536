// k_reduce.hip -- large frames inside the feature stage: one launch reduces every image of a step that has a reduction (lvt_amd_set_reduction) by its
// integer factor f = 2 ... 8, the mean of each f x f block:
//     S = sum over dy, dx in [0, f) of g[f y + dy][f x + dx],   out[y][x] = (S + (f f >> 1)) / (f f)          (integer division; include/lvt_amd_ext.h)
// The table travels BY VALUE like GrayTable / RectTable; blockIdx.y = image, the grid's x extent follows the largest image and a smaller image's surplus
// workgroups leave at the top.  A thread owns one 32-bit word of the destination (4 pixels; words are numbered row after row over the destination PITCH: the
// padding columns are written as zero without any load, no lane idles at a row's end).  Such a word is 4 f consecutive bytes of each of f source rows, and
// the lanes of a wave read consecutive segments: a row of the source streams through once, every byte of it in exactly one lane.
//  - THE VECTOR PATH.  Where the descriptor's base and pitch are multiples of 4 -- a test on the descriptor alone, so wave-uniform and kept in scalar
//    registers -- every segment starts on a dword of its row, and a thread loads its 4 f bytes of a row as f dwords in the widest vectors f allows (f = 2: one
//    8-byte load, f = 4: one 16-byte load, f = 8: two of them; odd f: 16 / 12 / 8 / 4-byte pieces).  The bytes of a dword are summed by v_sad_u8 against zero.
//  - THE BYTE PATH.  Any other base or pitch, and a row's last partial word on either path: byte loads of the pixels that exist.
//  Both paths read only [row start, row start + f bW) of source rows 0 ... f bH - 1: up to f - 1 trailing columns and rows of the frame are never touched, and
//  what lies behind a row's last block may be the caller's next allocation, or nobody's.  A full word's segment ends at 4 f (xw + 1) <= f bW, so the vector
//  path needs no second bound.
//  - f is a template argument picked per image (a uniform switch): the loops unroll, the byte-to-pixel assignment is fixed at compile time and the division by
//    f f is the compiler's multiply-shift, exact for every 32-bit numerator (S <= 255 * 64).  No LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lvt {

struct ReduceImg {
    const uint8_t *src;   // gray frame (any address, any pitch >= f * w)
    uint8_t *dst;         // reduced plane, 4-byte aligned, dst_pitch % 4 == 0
    int src_pitch, dst_pitch;
    int w, h, f;          // the DESTINATION's size (the base size bW x bH) and the factor, 2 ... 8
};
constexpr int REDUCE_MAX_FACTOR = 8, REDUCE_MAX_SIDE = 16384;   // a record's limits (lvt_amd_reduction)
constexpr int REDUCE_PACK = 64;     // images per launch (32 stereo sequences); a step with more takes a further launch
constexpr int REDUCE_THREADS = 64;   // one wave per workgroup: no LDS and no barrier hold a larger one together, and an f = 8 launch on a 4K pair has only 1 000 waves to spread over the CUs
struct ReduceTable {
    ReduceImg im[REDUCE_PACK];
};
static_assert(sizeof(ReduceTable) < 4096, "k_reduce_frames' arguments must stay under 4096 bytes");

// one destination word at (row y, pixels x4 ... x4 + 3) of image I
template <int F>
__device__ __forceinline__ uint32_t reduce_word(const ReduceImg &I, int y, int x4, bool vec) {
    constexpr uint32_t FF = F * F;
    const uint8_t *P = I.src + (size_t)(y * F) * I.src_pitch + (size_t)x4 * F;
    uint32_t s[4] = {0, 0, 0, 0};
    if (vec && x4 + 4 <= I.w) {
#pragma unroll
        for (int dy = 0; dy < F; dy++) {
            uint32_t wd[F];
            __builtin_memcpy(wd, __builtin_assume_aligned(P + (size_t)dy * I.src_pitch, 4), 4 * F);
#pragma unroll
            for (int d = 0; d < F; d++) {
#pragma unroll
                for (int k = 0; k < 4; k++) {   // the bytes of dword d that belong to pixel k: segment bytes [F k, F k + F) meet [4 d, 4 d + 4)
                    const int lo = (F * k > 4 * d ? F * k : 4 * d) - 4 * d, hi = (F * k + F < 4 * d + 4 ? F * k + F : 4 * d + 4) - 4 * d;
                    if (hi <= lo) continue;
                    const uint32_t mask = (hi - lo == 4) ? 0xFFFFFFFFu : (((1u << (8 * (hi - lo))) - 1u) << (8 * lo));
                    s[k] = __builtin_amdgcn_sad_u8(wd[d] & mask, 0u, s[k]);
                }
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (x4 + k >= I.w) continue;   // (the last byte read is byte F (x4 + k) + F - 1 < F w of the row)
#pragma unroll
            for (int dy = 0; dy < F; dy++) {
                const uint8_t *p = P + (size_t)dy * I.src_pitch + k * F;
#pragma unroll
                for (int dx = 0; dx < F; dx++) s[k] += p[dx];
            }
        }
    }
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (x4 + k < I.w) packed |= ((s[k] + (FF >> 1)) / FF) << (8 * k);
    return packed;
}

__global__ __launch_bounds__(REDUCE_THREADS) void k_reduce_frames(ReduceTable tab) {
    const ReduceImg &I = tab.im[blockIdx.y];   // (uniform index: the descriptor stays in scalar registers)
    const int wpr = I.dst_pitch >> 2;          // words per destination row
    const unsigned word = blockIdx.x * (unsigned)REDUCE_THREADS + threadIdx.x;
    if (word >= (unsigned)(wpr * I.h)) return;   // (a smaller image's surplus workgroups leave here as a whole)
    const int y = (int)(word / (unsigned)wpr), x4 = (int)(word - (unsigned)y * (unsigned)wpr) * 4;
    uint32_t packed = 0;
    if (x4 < I.w) {   // (a padding word: zero, nothing is loaded)
        const bool vec = (((uintptr_t)I.src | (uintptr_t)(unsigned)I.src_pitch) & 3) == 0;
        switch (I.f) {
        case 2: packed = reduce_word<2>(I, y, x4, vec); break;
        case 3: packed = reduce_word<3>(I, y, x4, vec); break;
        case 4: packed = reduce_word<4>(I, y, x4, vec); break;
        case 5: packed = reduce_word<5>(I, y, x4, vec); break;
        case 6: packed = reduce_word<6>(I, y, x4, vec); break;
        case 7: packed = reduce_word<7>(I, y, x4, vec); break;
        case 8: packed = reduce_word<8>(I, y, x4, vec); break;
        default: break;   // (no descriptor has another factor: the host builds them from checked records)
        }
    }
    *reinterpret_cast<uint32_t *>(I.dst + (size_t)y * I.dst_pitch + x4) = packed;
}

}  // namespace lvt
