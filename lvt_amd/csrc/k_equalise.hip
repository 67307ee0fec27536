// k_equalise.hip -- dim frames: CLAHE contrast equalisation inside the feature stage (lvt_amd_set_equalisation; include/lvt_amd_ext.h has the definition,
// tests/clahe_util.py restates it in numpy byte for byte).  What is equalised is the gray plane k_score would otherwise read: behind k_gray_frames and
// k_rectify_frames, in front of the buffer gate.
//   k_clahe_lut   : one workgroup of 256 threads per (tile, image).  The tile's 256-bin histogram is built in LDS with LDS atomics, one sub-histogram per
//                   wavefront (a dim frame puts most of a tile's pixels into a few bins: four copies quarter the contention), folded afterwards; thread i then
//                   owns bin i for the clip, the batch and the residual rule; the excess is summed with wave_reduce_scatter (integers below 2^53: the fp64
//                   sums are exact) and the 256-bin inclusive scan is an integer scan in LDS, so neither shape can change a bit.  256 bytes per tile go to
//                   the sequence's table buffer.  The source is read byte-wise at its own pitch: the mirror indices of the padded columns and rows lie inside
//                   the image by construction (pad < tiles <= size), so no load falls outside [row start, row start + W) of a source row.
//   k_clahe_apply : a thread owns one 32-bit word of the destination (4 pixels, one coalesced store; words are numbered row after row over the destination
//                   PITCH, so the padding columns are written as zero -- the shape of k_gray_frames and k_rectify_frames).  Per pixel four table bytes are
//                   gathered and interpolated in fp32, one IEEE operation per written operation (-ffp-contract=off).  The tables of the tile rows a
//                   workgroup's pixels touch are staged in LDS when there are at most two of them (<= 2 * 16 * 256 = 8 KB: every image whose pitch is at
//                   least a few hundred pixels); a workgroup that spans more tile rows (tiny images), or a descriptor that says `direct`, gathers from
//                   the table buffer through L1 -- the whole table set of an image is at most 64 KB.  Measured (profiles/equalisation.md): LDS 9.2 / 8.6 /
//                   7.0 us, L1 10.1 / 9.2 / 7.0 us on KITTI- / EuRoC- / TUM-shaped frames: the staging stays.
// The descriptors travel BY VALUE like GrayTable / RectTable; blockIdx.y = image, the grid's x extent follows the largest image of the launch and a smaller
// image's surplus workgroups leave at the top.  No scratch.
#include "lvt_dev.h"
#include "wave_reduce.h"

namespace lvt {

struct ClaheImg {
    const uint8_t *src;   // gray plane (any address, any pitch >= w; read byte-wise)
    uint8_t *dst;         // equalised plane, dst_pitch % 4 == 0, 4-byte aligned
    uint8_t *lut;         // tiles_x * tiles_y tables of 256 bytes, tile (tx, ty) at (ty * tiles_x + tx) * 256; 4-byte aligned
    int src_pitch, dst_pitch;
    int w, h;
    int tiles_x, tiles_y, tile_w, tile_h;
    int clip;             // the clip level (definition, step 2): computed on the host, lvt_amd_equalisation_plan
    float lut_scale;      // 255.0f / (float)area
    float inv_tw, inv_th; // 1.0f / (float)tile_w, 1.0f / (float)tile_h
    int direct;           // != 0: k_clahe_apply gathers from the table buffer, never from LDS
};
constexpr int CLAHE_PACK = 48;  // images per launch; a step with more equalised images takes further launches
struct ClaheTable {
    ClaheImg im[CLAHE_PACK];
};
static_assert(sizeof(ClaheTable) < 4096, "the equalisation kernels' arguments must stay under 4096 bytes");
constexpr int CLAHE_MAX_TILES = 16;
constexpr int CLAHE_STAGE_BYTES = 2 * CLAHE_MAX_TILES * 256;   // two tile rows of tables

__global__ __launch_bounds__(256) void k_clahe_lut(ClaheTable tab) {
    const ClaheImg &I = tab.im[blockIdx.y];   // (uniform index: the descriptor stays in scalar registers)
    if (blockIdx.x >= (unsigned)(I.tiles_x * I.tiles_y)) return;   // (an image with fewer tiles: its surplus workgroups leave here as a whole)
    __shared__ unsigned hist[4][256];
    __shared__ unsigned scan[2][256];
    __shared__ unsigned wave_excess[4];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int ty = (int)blockIdx.x / I.tiles_x, tx = (int)blockIdx.x - ty * I.tiles_x;
#pragma unroll
    for (int k = 0; k < 4; k++) hist[k][tid] = 0;
    __syncthreads();
    // the tile's area = tile_w * tile_h padded pixels; x >= w reads 2 (w - 1) - x (BORDER_REFLECT_101), likewise y
    // (pixels are numbered row after row over the TILE's width, so no lane idles at a tile row's end; area <= 8192 * 8192 fits an int)
    const int x0 = tx * I.tile_w, y0 = ty * I.tile_h, area = I.tile_w * I.tile_h;
    // (eight byte loads in flight per thread before their atomics -- a KITTI-shaped tile is 29 pixels per thread; with one load per round trip the launch
    //  measured 17.0 / 16.0 / 13.7 us between its HIP events on KITTI- / EuRoC- / TUM-shaped frames, with eight 14.5 / 12.2 / 10.8)
    constexpr int UNROLL = 8;
    for (int i0 = tid; i0 < area; i0 += 256 * UNROLL) {
        int v[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; k++) {
            const int i = i0 + 256 * k;
            v[k] = -1;
            if (i < area) {
                const int py = (int)((unsigned)i / (unsigned)I.tile_w);
                int x = x0 + (i - py * I.tile_w), y = y0 + py;
                if (x >= I.w) x = 2 * (I.w - 1) - x;
                if (y >= I.h) y = 2 * (I.h - 1) - y;
                v[k] = I.src[(size_t)y * I.src_pitch + x];
            }
        }
#pragma unroll
        for (int k = 0; k < UNROLL; k++)
            if (v[k] >= 0) atomicAdd(&hist[wave][v[k]], 1u);
    }
    __syncthreads();
    int h = (int)(hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid]);
    // clip, and the excess of all 256 bins
    const double mine[1] = {(double)max(h - I.clip, 0)};
    const double wsum = wave_reduce_scatter(mine);   // (lanes 0 and 1 of a wavefront hold value 0's total)
    if ((tid & 63) == 0) wave_excess[wave] = (unsigned)wsum;
    __syncthreads();
    const int excess = (int)(wave_excess[0] + wave_excess[1] + wave_excess[2] + wave_excess[3]);
    const int batch = excess / 256, residual = excess - 256 * batch;
    h = min(h, I.clip) + batch;
    if (residual > 0) {
        const int step = max(256 / residual, 1);
        if (tid % step == 0 && tid / step < residual) h++;
    }
    // inclusive integer prefix sum over the 256 bins
    int cur = 0;
    scan[0][tid] = (unsigned)h;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {
        unsigned v = scan[cur][tid];
        if (tid >= d) v += scan[cur][tid - d];
        scan[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    const float f = (float)(int)scan[cur][tid] * I.lut_scale;
    I.lut[(size_t)blockIdx.x * 256 + tid] = (uint8_t)min(max(__float2int_rn(f), 0), 255);
}

// floor(f) as a tile index and the weight of the NEXT tile: taken before the index is clamped
__device__ __forceinline__ void clahe_axis(int p, float inv, int tiles, int &t1, int &t2, float &a, float &a1) {
    const float f = (float)p * inv - 0.5f;
    const float fl = floorf(f);
    a = f - fl, a1 = 1.0f - a;
    const int i = (int)fl;
    t1 = min(max(i, 0), tiles - 1), t2 = min(max(i + 1, 0), tiles - 1);
}

__global__ __launch_bounds__(256) void k_clahe_apply(ClaheTable tab) {
    const ClaheImg &I = tab.im[blockIdx.y];   // (uniform index: the descriptor stays in scalar registers)
    const int wpr = I.dst_pitch >> 2;         // words per destination row
    const unsigned n_words = (unsigned)(wpr * I.h);
    const unsigned first = blockIdx.x * 256u;
    if (first >= n_words) return;             // (a smaller image's surplus workgroups leave here as a whole)
    __shared__ __attribute__((aligned(16))) uint8_t stage[CLAHE_STAGE_BYTES];
    // the tile rows this workgroup's destination rows touch: floor((float)y * inv_th - 0.5f) does not decrease with y, so the first and the last row bound them
    const unsigned last = min(first + 255u, n_words - 1u);
    int r0, r1, ru;
    float fu, fv;
    clahe_axis((int)(first / (unsigned)wpr), I.inv_th, I.tiles_y, r0, ru, fu, fv);
    clahe_axis((int)(last / (unsigned)wpr), I.inv_th, I.tiles_y, ru, r1, fu, fv);
    const bool staged = !I.direct && r1 - r0 <= 1;   // (uniform over the workgroup)
    const int row_bytes = I.tiles_x * 256;
    if (staged) {
        const uint32_t *g = reinterpret_cast<const uint32_t *>(I.lut + (size_t)r0 * row_bytes);
        uint32_t *s = reinterpret_cast<uint32_t *>(stage);
        const int n = (r1 - r0 + 1) * (row_bytes >> 2);   // <= CLAHE_STAGE_BYTES / 4
        for (int i = threadIdx.x; i < n; i += 256) s[i] = g[i];
        __syncthreads();
    }
    const unsigned word = first + threadIdx.x;
    if (word >= n_words) return;
    const int y = (int)(word / (unsigned)wpr), x4 = (int)(word - (unsigned)y * (unsigned)wpr) * 4;
    int y1, y2;
    float ya, ya1;
    clahe_axis(y, I.inv_th, I.tiles_y, y1, y2, ya, ya1);
    const uint8_t *L1 = staged ? stage + (y1 - r0) * row_bytes : I.lut + (size_t)y1 * row_bytes;
    const uint8_t *L2 = staged ? stage + (y2 - r0) * row_bytes : I.lut + (size_t)y2 * row_bytes;
    const uint8_t *P = I.src + (size_t)y * I.src_pitch;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x4 + k;
        if (x < I.w) {   // (the only source byte read: x < w of row y)
            int x1, x2;
            float xa, xa1;
            clahe_axis(x, I.inv_tw, I.tiles_x, x1, x2, xa, xa1);
            const int v = P[x];
            const float a = (float)L1[x1 * 256 + v] * xa1 + (float)L1[x2 * 256 + v] * xa;
            const float b = (float)L2[x1 * 256 + v] * xa1 + (float)L2[x2 * 256 + v] * xa;
            const float r = a * ya1 + b * ya;
            packed |= (uint32_t)min(max(__float2int_rn(r), 0), 255) << (8 * k);
        }
    }
    *reinterpret_cast<uint32_t *>(I.dst + (size_t)y * I.dst_pitch + x4) = packed;
}

}  // namespace lvt
