// k_sensor.hip -- sensor formats inside the feature stage: one launch turns every image of a step whose sequence has a sensor format
// (lvt_amd_set_sensor_format) into the 8-bit gray plane the tracker runs on.  Integer arithmetic throughout (include/lvt_amd_ext.h, SENSOR FORMATS;
// tests/sensor_util.py restates it in numpy):
//   BAYER (RGGB, BGGR, GRBG, GBRG; 8 bit)  missing channels are the mean of the nearest samples of that colour, kept unscaled as X4 = 4 x the value (the sum
//       of four, twice the sum of two, four times the own sample); neighbours outside the image are mirrored without repeating the edge (-1 -> 1, W -> W - 2:
//       the colour phase is kept);  gray = (4899 R4 + 9617 G4 + 1868 B4 + 32768) >> 16
//   YUYV / UYVY                            gray[y][x] = row[2 x] / row[2 x + 1]
//   MONO16 (little-endian uint16)          g = min(max(v, lo), hi);  out = ((g - lo) 255 + ((hi - lo) >> 1)) / (hi - lo), truncating
//       [lo, hi] is the record's, or -- auto_window -- found per image and per frame by k_sensor_hist + k_sensor_levels in front of the conversion.
// The table travels BY VALUE like GrayTable / ReduceTable; blockIdx.y = image, the grid's x extent follows the largest image and a smaller image's surplus
// workgroups leave at the top.  A thread owns one 32-bit word of the destination (4 pixels; words are numbered row after row over the destination PITCH: the
// padding columns are written as zero without any load).  The format is a field of the descriptor, so it is wave-uniform, stays in scalar registers, and is
// switched on once.
//  - LOADS.  Where the descriptor's base and pitch are multiples of 4 -- a test on the descriptor alone -- a full word's source bytes are loaded as dwords
//    (Bayer: one per row of the 3-row window plus the two flanking bytes; the 16-bit formats: two).  Any other base or pitch, and a row's last partial word on
//    either path: loads of the single samples that exist (bytes; MONO16: 16-bit words, its base and pitch are even by contract).
//  - BOUNDS.  No load falls outside [row start, row start + row bytes) of source rows 0 ... H - 1.  The 16-bit formats read bytes [8 xw, 8 xw + 8) of a full
//    word's row, and 8 xw + 8 <= 2 W.  Bayer reads columns mir(x - 1) ... mir(x + 1) of rows mir(y - 1) ... mir(y + 1) for the pixels x < W it writes, with
//    mir(-1) = 1 and mir(n) = n - 2: inside [0, n) for every n >= 2 (the setter refuses smaller images); columns that belong to no written pixel are clamped
//    into the row before they are loaded.
//  - THE DIVISION by the wave-uniform d = hi - lo: the quotient is at most 255 (g - lo <= d), the numerator is below 2^24 and so exact as a float; the
//    estimate trunc(n * (1 / d)) is off by at most one either way and is corrected by the remainder.  tests/test_gpu_sensor_formats.py runs every
//    v for five windows.
// No LDS and no scratch in k_sensor_frames; k_sensor_hist keeps one sub-histogram per wavefront in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lvt {

constexpr int SENSOR_NONE = 0, SENSOR_BAYER_RGGB8 = 16, SENSOR_BAYER_BGGR8 = 17, SENSOR_BAYER_GRBG8 = 18, SENSOR_BAYER_GBRG8 = 19, SENSOR_YUYV = 24, SENSOR_UYVY = 25,
              SENSOR_MONO16 = 32;   // LVT_AMD_SENSOR_* (include/lvt_amd_ext.h)
__host__ __device__ constexpr bool sensor_is_bayer(int f) { return f >= SENSOR_BAYER_RGGB8 && f <= SENSOR_BAYER_GBRG8; }
__host__ __device__ constexpr bool sensor_known(int f) { return sensor_is_bayer(f) || f == SENSOR_YUYV || f == SENSOR_UYVY || f == SENSOR_MONO16; }
__host__ __device__ constexpr int sensor_bpp(int f) { return (f == SENSOR_YUYV || f == SENSOR_UYVY || f == SENSOR_MONO16) ? 2 : 1; }

struct SensorImg {
    const uint8_t *src;   // the sensor's plane (any address, any pitch >= w * bpp; MONO16: both even)
    uint8_t *dst;         // gray plane, 4-byte aligned, dst_pitch % 4 == 0
    const int *win;       // MONO16 auto window: {lo, hi} as k_sensor_levels wrote them (nullptr: the fixed window below)
    uint32_t *hist;       // MONO16 auto window: 4096 bins, zero between frames (k_sensor_levels clears what it has read)
    int src_pitch, dst_pitch;
    int w, h, fmt;
    int lo, hi;           // MONO16 fixed window
    int lo_pm, hi_pm, min_span;   // MONO16 auto window (k_sensor_levels); its result goes to `win`, which is then spelled int * there
};
constexpr int SENSOR_PACK = 48;       // images per launch (24 stereo sequences); a step with more takes a further launch
constexpr int SENSOR_BINS = 4096;     // histogram bins of v >> 4
constexpr int SENSOR_HIST_THREADS = 128, SENSOR_HIST_WORDS = 16;   // k_sensor_hist: 2 wavefronts, each thread takes 16 dwords (32 pixels)
struct SensorTable {
    SensorImg im[SENSOR_PACK];
};
static_assert(sizeof(SensorTable) < 4096, "k_sensor_frames' arguments must stay under 4096 bytes");

// mirror without repeating the edge, then (for columns no written pixel needs) a clamp into [0, n)
__device__ __forceinline__ int sensor_mir(int x, int n) {
    x = x < 0 ? -x : (x >= n ? 2 * (n - 1) - x : x);
    return x < 0 ? 0 : (x >= n ? n - 1 : x);
}

// Bayer: 4 pixels of row y from x4 on.  c[r][j] = sample at (mir(x4 - 1 + j), mir(y - 1 + r))
__device__ __forceinline__ uint32_t sensor_bayer_word(const SensorImg &I, int y, int x4, bool vec) {
    const int rx = (I.fmt == SENSOR_BAYER_BGGR8 || I.fmt == SENSOR_BAYER_GRBG8) ? 1 : 0;   // the red sample's column and row parity
    const int ry = (I.fmt == SENSOR_BAYER_BGGR8 || I.fmt == SENSOR_BAYER_GBRG8) ? 1 : 0;
    uint32_t c[3][6];
    const bool full = vec && x4 + 4 <= I.w;
    const int xl = sensor_mir(x4 - 1, I.w), xr = sensor_mir(x4 + 4, I.w);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const uint8_t *row = I.src + (size_t)sensor_mir(y - 1 + r, I.h) * I.src_pitch;
        if (full) {
            const uint32_t wd = *reinterpret_cast<const uint32_t *>(__builtin_assume_aligned(row + x4, 4));
            c[r][0] = row[xl], c[r][5] = row[xr];
#pragma unroll
            for (int k = 0; k < 4; k++) c[r][1 + k] = (wd >> (8 * k)) & 0xFFu;
        } else {
#pragma unroll
            for (int j = 0; j < 6; j++) c[r][j] = row[sensor_mir(x4 - 1 + j, I.w)];
        }
    }
    const bool red_row = (y & 1) == ry;
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (x4 + k >= I.w) continue;
        const uint32_t C4 = 4u * c[1][1 + k], Hs = c[1][k] + c[1][2 + k], Vs = c[0][1 + k] + c[2][1 + k], Ds = c[0][k] + c[0][2 + k] + c[2][k] + c[2][2 + k];
        const bool red_col = (k & 1) == rx;   // (x4 is a multiple of 4: the column parity is k's)
        uint32_t R4, G4, B4;
        if (red_row == red_col) {   // a red or a blue sample: the other colour on the diagonals, green on the axes
            G4 = Hs + Vs;
            R4 = red_row ? C4 : Ds, B4 = red_row ? Ds : C4;
        } else {                    // a green sample: the row's colour left and right, the other above and below
            G4 = C4;
            R4 = red_row ? 2u * Hs : 2u * Vs, B4 = red_row ? 2u * Vs : 2u * Hs;
        }
        packed |= ((4899u * R4 + 9617u * G4 + 1868u * B4 + 32768u) >> 16) << (8 * k);
    }
    return packed;
}

// the 4 samples of a 16-bit-per-pixel row from pixel x4 on, as 16-bit values (pixels >= w: 0, never loaded)
__device__ __forceinline__ void sensor_load16(const SensorImg &I, int y, int x4, bool vec, uint32_t v[4]) {
    const uint8_t *row = I.src + (size_t)y * I.src_pitch;
    if (vec && x4 + 4 <= I.w) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(__builtin_assume_aligned(row + 2 * (size_t)x4, 4));
        const uint32_t a = p[0], b = p[1];
        v[0] = a & 0xFFFFu, v[1] = a >> 16, v[2] = b & 0xFFFFu, v[3] = b >> 16;
    } else if (I.fmt == SENSOR_MONO16) {
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (x4 + k < I.w) ? *reinterpret_cast<const uint16_t *>(row + 2 * (size_t)(x4 + k)) : 0u;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint8_t *p = row + 2 * (size_t)(x4 + k);
            v[k] = (x4 + k < I.w) ? (uint32_t)p[0] | ((uint32_t)p[1] << 8) : 0u;
        }
    }
}

// ((g - lo) 255 + (d >> 1)) / d for d = hi - lo in 1 ... 65535, exactly: see the head of this file
__device__ __forceinline__ uint32_t sensor_map16(uint32_t v, uint32_t lo, uint32_t hi, uint32_t d, float rd) {
    const uint32_t g = v < lo ? lo : (v > hi ? hi : v);
    const uint32_t n = (g - lo) * 255u + (d >> 1);
    uint32_t q = (uint32_t)((float)n * rd);
    int r = (int)n - (int)(q * d);
    if (r < 0) q--, r += (int)d;
    if (r >= (int)d) q++;
    return q;
}

__global__ __launch_bounds__(256) void k_sensor_frames(SensorTable tab) {
    const SensorImg &I = tab.im[blockIdx.y];   // (uniform index: the descriptor stays in scalar registers)
    const int wpr = I.dst_pitch >> 2;          // words per destination row
    const unsigned word = blockIdx.x * 256u + threadIdx.x;
    if (word >= (unsigned)(wpr * I.h)) return;   // (a smaller image's surplus workgroups leave here as a whole)
    const int y = (int)(word / (unsigned)wpr), x4 = (int)(word - (unsigned)y * (unsigned)wpr) * 4;
    uint32_t packed = 0;
    if (x4 < I.w) {   // (a padding word: zero, nothing is loaded)
        const bool vec = (((uintptr_t)I.src | (uintptr_t)(unsigned)I.src_pitch) & 3) == 0;
        switch (I.fmt) {
        case SENSOR_BAYER_RGGB8:
        case SENSOR_BAYER_BGGR8:
        case SENSOR_BAYER_GRBG8:
        case SENSOR_BAYER_GBRG8: packed = sensor_bayer_word(I, y, x4, vec); break;
        case SENSOR_YUYV:
        case SENSOR_UYVY: {
            uint32_t v[4];
            sensor_load16(I, y, x4, vec, v);
            const int sh = (I.fmt == SENSOR_UYVY) ? 8 : 0;
#pragma unroll
            for (int k = 0; k < 4; k++) packed |= ((v[k] >> sh) & 0xFFu) << (8 * k);
            break;
        }
        case SENSOR_MONO16: {
            uint32_t v[4];
            sensor_load16(I, y, x4, vec, v);
            const uint32_t lo = (uint32_t)(I.win ? I.win[0] : I.lo), hi = (uint32_t)(I.win ? I.win[1] : I.hi), d = hi - lo;
            const float rd = 1.0f / (float)d;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (x4 + k < I.w) packed |= sensor_map16(v[k], lo, hi, d, rd) << (8 * k);
            break;
        }
        default: break;   // (no descriptor has another format: the host builds them from checked records)
        }
    }
    *reinterpret_cast<uint32_t *>(I.dst + (size_t)y * I.dst_pitch + x4) = packed;
}

// ---- MONO16 auto window: the histogram of v >> 4 over the W x H pixels of every such image of the step ----------------------------------------------------
// A thread takes SENSOR_HIST_WORDS dwords (2 pixels each; dwords are numbered row after row over ceil(W / 2) per row), a wavefront counts into its own LDS
// sub-histogram with integer atomics, and the workgroup adds the bins it touched to the image's histogram in memory with integer atomics: integer sums in any
// order are the same sums, so the result is deterministic.  Loads: a dword where base and pitch are multiples of 4 and both pixels exist, else 16-bit words.
__global__ __launch_bounds__(SENSOR_HIST_THREADS) void k_sensor_hist(SensorTable tab) {
    __shared__ uint32_t sub[SENSOR_HIST_THREADS / 64][SENSOR_BINS];
    const SensorImg &I = tab.im[blockIdx.y];
    const int wpr = (I.w + 1) >> 1;
    const unsigned total = (unsigned)(wpr * I.h), first = blockIdx.x * (unsigned)(SENSOR_HIST_THREADS * SENSOR_HIST_WORDS);
    if (first >= total) return;   // (uniform: the whole workgroup leaves, ahead of every barrier)
    uint32_t *flat = &sub[0][0];
    for (int i = threadIdx.x; i < (SENSOR_HIST_THREADS / 64) * SENSOR_BINS; i += SENSOR_HIST_THREADS) flat[i] = 0;
    __syncthreads();
    uint32_t *mine = sub[threadIdx.x >> 6];
    const bool vec = (((uintptr_t)I.src | (uintptr_t)(unsigned)I.src_pitch) & 3) == 0;
    for (int it = 0; it < SENSOR_HIST_WORDS; it++) {
        const unsigned word = first + (unsigned)it * SENSOR_HIST_THREADS + threadIdx.x;   // (consecutive lanes, consecutive dwords)
        if (word >= total) break;
        const int y = (int)(word / (unsigned)wpr), x2 = (int)(word - (unsigned)y * (unsigned)wpr) * 2;
        const uint8_t *p = I.src + (size_t)y * I.src_pitch + 2 * (size_t)x2;
        if (x2 + 2 <= I.w) {
            uint32_t a, b;
            if (vec) {
                const uint32_t wd = *reinterpret_cast<const uint32_t *>(__builtin_assume_aligned(p, 4));
                a = wd & 0xFFFFu, b = wd >> 16;
            } else {
                a = reinterpret_cast<const uint16_t *>(p)[0], b = reinterpret_cast<const uint16_t *>(p)[1];
            }
            atomicAdd(&mine[a >> 4], 1u);
            atomicAdd(&mine[b >> 4], 1u);
        } else {
            atomicAdd(&mine[*reinterpret_cast<const uint16_t *>(p) >> 4], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SENSOR_BINS; b += SENSOR_HIST_THREADS) {
        uint32_t n = 0;
#pragma unroll
        for (int wv = 0; wv < SENSOR_HIST_THREADS / 64; wv++) n += sub[wv][b];
        if (n) atomicAdd(&I.hist[b], n);
    }
}

// ---- ... and the two levels: one workgroup per image, an integer scan over the 4096 bins (a thread owns 16 consecutive bins) ---------------------------------
//   cum(b) = pixels in bins <= b, N = W H, 64-bit products:   lo_bin = min b with cum(b) 1000 > lo_pm N,   hi_bin = min b with cum(b) 1000 >= (1000 - hi_pm) N
//   lo = 16 lo_bin, hi = 16 hi_bin + 15;  where hi - lo < min_span:  mid = (lo + hi) >> 1, lo = max(0, mid - (min_span >> 1)), hi = lo + min_span, and if
//   hi > 65535: hi = 65535, lo = hi - min_span.
// Both bins exist (cum(4095) = N and the shares are below 500).  The bins are cleared as they are read: the next frame's k_sensor_hist finds zeros.
__global__ __launch_bounds__(256) void k_sensor_levels(SensorTable tab) {
    __shared__ uint32_t part[256];
    __shared__ int bins[2];
    const SensorImg &I = tab.im[blockIdx.x];
    const int t = threadIdx.x;
    uint32_t h[16], own = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        h[k] = I.hist[16 * t + k];
        I.hist[16 * t + k] = 0;
        own += h[k];
    }
    part[t] = own;
    if (t < 2) bins[t] = SENSOR_BINS;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // inclusive integer scan of the 256 partial sums
        const uint32_t add = (t >= off) ? part[t - off] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    const unsigned long long N = (unsigned long long)I.w * (unsigned long long)I.h;
    const unsigned long long lo_need = (unsigned long long)I.lo_pm * N, hi_need = (unsigned long long)(1000 - I.hi_pm) * N;
    unsigned long long cum = part[t] - own;
    int lo_b = SENSOR_BINS, hi_b = SENSOR_BINS;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        cum += h[k];
        if (lo_b == SENSOR_BINS && cum * 1000ull > lo_need) lo_b = 16 * t + k;
        if (hi_b == SENSOR_BINS && cum * 1000ull >= hi_need) hi_b = 16 * t + k;
    }
    if (lo_b < SENSOR_BINS) atomicMin(&bins[0], lo_b);
    if (hi_b < SENSOR_BINS) atomicMin(&bins[1], hi_b);
    __syncthreads();
    if (t == 0) {
        int lo = 16 * bins[0], hi = 16 * bins[1] + 15;
        if (hi - lo < I.min_span) {
            const int mid = (lo + hi) >> 1;
            lo = mid - (I.min_span >> 1);
            lo = lo < 0 ? 0 : lo;
            hi = lo + I.min_span;
            if (hi > 65535) hi = 65535, lo = hi - I.min_span;
        }
        int *out = const_cast<int *>(I.win);
        out[0] = lo, out[1] = hi;
    }
}

}  // namespace lvt
