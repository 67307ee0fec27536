// k_rectify.hip -- EuRoC pre-step: cv::initUndistortRectifyMap + cv::remap(INTER_LINEAR) as the
// reference's example runs them before every track() (examples/euroc/euroc_example.cpp:95-107,142-143 there).
//
//   k_rectify_map : one thread per image ROW.  OpenCV accumulates the homogeneous coordinate along the row
//                   (_x += ir[0] per column), so the columns of a row are a sequential fp64 recurrence; rows are
//                   independent.  Runs once per rectifier; writes the two CV_32FC1 maps.
//   k_rectify_map_radtan / k_rectify_map_fisheye : the same builder for a twelve-coefficient RADTAN lens and for a FISHEYE (equidistant) lens, source and
//                   destination two sizes ("LENS MODELS", include/lvt_amd_ext.h; lvt_amd_rectifier_create_lens).
//   k_rectify     : one thread per 4 output pixels: map -> 1/32-px fixed point (round-half-even), 2x2 gather with
//                   BORDER_CONSTANT 0, 15-bit weights, one 32-bit coalesced store.  8 B of map + 1 B out + <= 4 B of source
//                   per pixel: HBM-bound by construction, but one 752x480 image is 4.7 MB -- 0.6 us at 8 TB/s -- so a
//                   single launch is latency-bound like the rest of the single-sequence chain.
//   k_rectify_fix / k_rectify_frames : the same remap as the first kernel of a tracker's feature stage (raw frames, lvt_amd_set_rectifiers):
//                   one launch for both eyes of every sequence of a step, from an interleaved fixed-point form of the maps.
//   k_gray_frames : in front of it, colour frames (lvt_amd_set_pixel_format): one launch converts every colour image of a step to gray.
#include "lvt_dev.h"

namespace lvt {

struct RectifyArgs {
    double ir[9];             // (Pnew * R)^-1
    double fx, fy, u0, v0;    // distorted camera
    double k1, k2, p1, p2, k3;
    int w, h;
};

__global__ __launch_bounds__(64) void k_rectify_map(RectifyArgs a, float *map1, float *map2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.h) return;
    const double *ir = a.ir;
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    for (int j = 0; j < a.w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        const double iw = 1. / _w, x = _x * iw, y = _y * iw;
        const double x2 = x * x, y2 = y * y;
        const double r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = (1 + ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2) / (1 + ((0 * r2 + 0) * r2 + 0) * r2);
        const double xd = (x * kr + a.p1 * _2xy + a.p2 * (r2 + 2 * x2) + 0 * r2 + 0 * r2 * r2);
        const double yd = (y * kr + a.p1 * (r2 + 2 * y2) + a.p2 * _2xy + 0 * r2 + 0 * r2 * r2);
        const double u = a.fx * 1. * xd + a.u0;
        const double v = a.fy * 1. * yd + a.v0;
        map1[(size_t)i * a.w + j] = (float)u;
        map2[(size_t)i * a.w + j] = (float)v;
    }
}

// ---- lens models ("LENS MODELS", include/lvt_amd_ext.h): the maps of a twelve-coefficient RADTAN lens and of a FISHEYE (equidistant) lens -------
// Source and destination are two sizes: w x h is the DESTINATION's (the maps'); the source's enters only through K and, later, the remap.
// One thread per destination ROW, as k_rectify_map.  The row recurrence stays sequential because it is the definition: _x, _y, _w of column j are
// the result of j rounded fp64 adds of iR[0], iR[3], iR[6] onto the row's start.  fp64 addition is not associative -- start + j * step, or a scan
// that adds partial sums in another order, rounds differently in the last bit --, and an ulp of _x survives 1 / _w, the polynomial and the fp32
// narrowing often enough that the maps would stop being equal to the text (and to OpenCV's).  Rows share nothing, so they run side by side.
// Built once per rectifier: a 480-row destination is eight waves, an 8192-row one 128; the stores of a wave go to 64 different rows (uncoalesced),
// which costs a one-time build some hundred microseconds and no frame anything.
// hipcc (gfx950, -O3): k_rectify_map_radtan 42 VGPRs (8 waves / SIMD), k_rectify_map_fisheye 72 VGPRs (7 waves / SIMD; atan's polynomial); 0 bytes of LDS,
// 0 bytes of scratch, no spill in either.
struct LensArgs {
    double ir[9];             // (Pnew * R)^-1
    double fx, fy, u0, v0;    // the distorted (raw) camera
    double d[12];             // RADTAN: k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4; FISHEYE: k1 k2 k3 k4
    int w, h;                 // the destination
};

__global__ __launch_bounds__(64) void k_rectify_map_radtan(LensArgs a, float *map1, float *map2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.h) return;
    const double *ir = a.ir;
    const double k1 = a.d[0], k2 = a.d[1], p1 = a.d[2], p2 = a.d[3], k3 = a.d[4], k4 = a.d[5], k5 = a.d[6], k6 = a.d[7];
    const double s1 = a.d[8], s2 = a.d[9], s3 = a.d[10], s4 = a.d[11];
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    for (int j = 0; j < a.w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        const double iw = 1. / _w, x = _x * iw, y = _y * iw;
        const double x2 = x * x, y2 = y * y;
        const double r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
        const double xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2);
        const double yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2);
        const double u = a.fx * xd + a.u0;
        const double v = a.fy * yd + a.v0;
        map1[(size_t)i * a.w + j] = (float)u;
        map2[(size_t)i * a.w + j] = (float)v;
    }
}

__global__ __launch_bounds__(64) void k_rectify_map_fisheye(LensArgs a, float *map1, float *map2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.h) return;
    const double *ir = a.ir;
    const double k1 = a.d[0], k2 = a.d[1], k3 = a.d[2], k4 = a.d[3];
    const double inf = __builtin_huge_val();
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    for (int j = 0; j < a.w; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        double u, v;
        if (_w <= 0) {   // a ray from behind the camera (or on its horizon): outside every source
            u = (_x > 0) ? -inf : inf;
            v = (_y > 0) ? -inf : inf;
        } else {
            const double x = _x / _w, y = _y / _w;
            const double r = sqrt(x * x + y * y);
            const double theta = atan(r);
            const double t2 = theta * theta, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double theta_d = theta * (1 + k1 * t2 + k2 * t4 + k3 * t6 + k4 * t8);
            const double scale = (r == 0) ? 1.0 : theta_d / r;
            u = a.fx * x * scale + a.u0;
            v = a.fy * y * scale + a.v0;
        }
        map1[(size_t)i * a.w + j] = (float)u;
        map2[(size_t)i * a.w + j] = (float)v;
    }
}

// one output pixel from the map entry in 1/32-px fixed point (sxf, syf): 2x2 gather with BORDER_CONSTANT 0, 15-bit weights
__device__ __forceinline__ int remap_fixed(const uint8_t *src, int sw, int sh, int sstep, int sxf, int syf) {
    const int sx = min(max(sxf >> 5, -32768), 32767), sy = min(max(syf >> 5, -32768), 32767), ax = sxf & 31, ay = syf & 31;
    int w0 = (32 - ax) * (32 - ay) * 32, w1 = ax * (32 - ay) * 32, w2 = (32 - ax) * ay * 32, w3 = ax * ay * 32;
    if (ax == 0 && ay == 0) w0 = 32767, w3 = 1;  // initInterTab2D: 32768 saturates to short, the sum fix-up lands on the last weight
    int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if ((unsigned)sx < (unsigned)max(sw - 1, 0) && (unsigned)sy < (unsigned)max(sh - 1, 0)) {
        const uint8_t *S = src + (size_t)sy * sstep + sx;
        v0 = S[0], v1 = S[1], v2 = S[sstep], v3 = S[sstep + 1];
    } else if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
        return 0;
    } else {
        const uint8_t *S0 = src + (ptrdiff_t)sy * sstep, *S1 = src + (ptrdiff_t)(sy + 1) * sstep;
        if (sx >= 0 && sy >= 0) v0 = S0[sx];
        if (sx + 1 < sw && sy >= 0) v1 = S0[sx + 1];
        if (sx >= 0 && sy + 1 < sh) v2 = S1[sx];
        if (sx + 1 < sw && sy + 1 < sh) v3 = S1[sx + 1];
    }
    const int r = (v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3 + (1 << 14)) >> 15;
    return min(max(r, 0), 255);
}
// float map -> 1/32-px fixed point: cvRound, round half to even, where the fp32 product is finite and inside (-2^31, 2^31); INT_MIN otherwise (NaN fails both
// comparisons), which >> 5 and the clamp put at -32768: outside every source, the pixel is 0 ("RECTIFICATION", include/lvt_amd_ext.h).  A pure function of the
// map value: k_rectify_fix stores exactly what k_rectify computes per pixel
__device__ __forceinline__ int map_to_fixed(float m) {
    const float p = m * 32.f;
    return (p > -2147483648.f && p < 2147483648.f) ? __float2int_rn(p) : INT_MIN;
}
__device__ __forceinline__ int remap_one(const uint8_t *src, int sw, int sh, int sstep, float mx, float my) {
    return remap_fixed(src, sw, sh, sstep, map_to_fixed(mx), map_to_fixed(my));
}

// dst_pitch % 4 == 0; the padding columns of dst (if any) are written as zero
__global__ __launch_bounds__(256) void k_rectify(const uint8_t *src, int sw, int sh, int sstep, const float *map1, const float *map2, int dw, int dh,
                                                 uint8_t *dst, int dst_pitch) {
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y;
    if (x4 >= dst_pitch || y >= dh) return;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x4 + k;
        if (x < dw) packed |= (uint32_t)remap_one(src, sw, sh, sstep, map1[(size_t)y * dw + x], map2[(size_t)y * dw + x]) << (8 * k);
    }
    *reinterpret_cast<uint32_t *>(dst + (size_t)y * dst_pitch + x4) = packed;
}

// the two float maps as ONE interleaved fixed-point map (x, y per pixel): built once per rectifier, one 8-byte load per pixel in k_rectify_frames
__global__ __launch_bounds__(256) void k_rectify_fix(const float *map1, const float *map2, int2 *fix, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) fix[i] = make_int2(map_to_fixed(map1[i]), map_to_fixed(map2[i]));
}

// ---- raw frames inside the feature stage: one launch rectifies both eyes of every sequence that brought a raw frame -----------------------
// One descriptor per image; the table travels BY VALUE in the kernel arguments (like FrameArgsPack): no device read of host memory in front of
// the frame.  blockIdx.y = image; the grid's x extent is sized by the largest image of the table and an image's surplus workgroups leave at the top.
// A thread owns one 32-bit word of the destination (4 pixels; words are numbered row after row over the destination PITCH, so the padding
// columns are written as zero and no lane idles at a row's end); per pixel one 8-byte map load and remap_fixed -- byte for byte k_rectify's output.
struct RectImg {
    const uint8_t *src;   // raw image (any pitch >= sw; read byte-wise)
    const int2 *map;      // dw x dh fixed-point entries (Rectifier::d_fix)
    uint8_t *dst;         // rectified plane, dst_pitch % 4 == 0
    int src_pitch, dst_pitch;
    int sw, sh, dw, dh;
};
constexpr int RECT_PACK = 64;   // images per launch (32 stereo sequences); larger batches take several launches
struct RectTable {
    RectImg im[RECT_PACK];
};
static_assert(sizeof(RectTable) < 4096, "k_rectify_frames' arguments must stay under 4096 bytes");

__global__ __launch_bounds__(256) void k_rectify_frames(RectTable tab) {
    const RectImg &I = tab.im[blockIdx.y];   // (uniform index: the descriptor stays in scalar registers)
    const int wpr = I.dst_pitch >> 2;        // words per destination row
    const unsigned word = blockIdx.x * 256u + threadIdx.x;
    if (blockIdx.x * 256u >= (unsigned)(wpr * I.dh)) return;   // a workgroup outside this image
    if (word >= (unsigned)(wpr * I.dh)) return;
    const int y = (int)(word / (unsigned)wpr), x4 = (int)(word - (unsigned)y * (unsigned)wpr) * 4;
    const int2 *M = I.map + (size_t)y * I.dw;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int x = x4 + k;
        if (x < I.dw) {
            const int2 m = M[x];
            packed |= (uint32_t)remap_fixed(I.src, I.sw, I.sh, I.src_pitch, m.x, m.y) << (8 * k);
        }
    }
    *reinterpret_cast<uint32_t *>(I.dst + (size_t)y * I.dst_pitch + x4) = packed;
}

// ---- colour frames inside the feature stage: one launch converts every colour image of a step to gray (lvt_amd_set_pixel_format) ---------------
// gray = (R 4899 + G 9617 + B 1868 + 8192) >> 14: cv::cvtColor's 8-bit BGR2GRAY, the weights examples/image_io.h uses.  The table travels BY VALUE like
// RectTable; blockIdx.y = image, the grid's x extent follows the largest image and a smaller image's surplus workgroups leave at the top.  A thread owns one
// 32-bit word of the destination (4 pixels; words are numbered row after row over the destination PITCH: the padding columns are written as zero, no lane
// idles at a row's end).  The source is read byte by byte, three bytes per pixel that exists: it may start at any address and have any pitch, and no load
// reaches outside [row start, row start + W bpp) of a source row -- what lies behind a row's last pixel may be the caller's next allocation, or nobody's.
// The format enters through the pixel stride and the byte offsets of R and B only (G is byte 1 of every format; an alpha byte is never loaded).
constexpr int PIX_GRAY8 = 0, PIX_BGR8 = 1, PIX_RGB8 = 2, PIX_BGRA8 = 3, PIX_RGBA8 = 4;   // LVT_AMD_PIX_* (include/lvt_amd_ext.h)
__host__ __device__ constexpr int pix_bpp(int fmt) { return fmt == PIX_GRAY8 ? 1 : (fmt >= PIX_BGRA8 ? 4 : 3); }
struct GrayImg {
    const uint8_t *src;   // interleaved colour image (any address, any pitch >= w * bpp; read byte-wise)
    uint8_t *dst;         // gray plane, dst_pitch % 4 == 0
    int src_pitch, dst_pitch;
    int w, h, fmt;
};
constexpr int GRAY_PACK = 64;   // images per launch; a step with more colour images takes several launches
struct GrayTable {
    GrayImg im[GRAY_PACK];
};
static_assert(sizeof(GrayTable) < 4096, "k_gray_frames' arguments must stay under 4096 bytes");

__global__ __launch_bounds__(256) void k_gray_frames(GrayTable tab) {
    const GrayImg &I = tab.im[blockIdx.y];   // (uniform index: the descriptor stays in scalar registers)
    const int wpr = I.dst_pitch >> 2;        // words per destination row
    const unsigned word = blockIdx.x * 256u + threadIdx.x;
    if (word >= (unsigned)(wpr * I.h)) return;   // (a smaller image's surplus workgroups leave here as a whole)
    const int y = (int)(word / (unsigned)wpr), x4 = (int)(word - (unsigned)y * (unsigned)wpr) * 4;
    const int bpp = pix_bpp(I.fmt);
    const int ro = (I.fmt == PIX_BGR8 || I.fmt == PIX_BGRA8) ? 2 : 0, bo = 2 - ro;
    const uint8_t *P = I.src + (size_t)y * I.src_pitch + (size_t)x4 * bpp;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x4 + k < I.w) {   // (the last byte read is byte (x4 + k) bpp + 2 < w bpp of the row)
            const uint8_t *p = P + k * bpp;
            const uint32_t r = p[ro], g = p[1], b = p[bo];
            packed |= ((r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14) << (8 * k);
        }
    }
    *reinterpret_cast<uint32_t *>(I.dst + (size_t)y * I.dst_pitch + x4) = packed;
}

}  // namespace lvt
