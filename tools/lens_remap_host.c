/* The remap of "RECTIFICATION" (include/lvt_amd_ext.h) on one host core: what a caller of the parent commit has to run in front of the gray entry points for a
 * lens the library does not know (tools/lens_models.py compiles this file and times that route).  8-bit source of sw x sh at any pitch, float maps of
 * dw x dh, destination tightly packed.  Float map -> 1/32-px fixed point once per pixel, 2 x 2 gather with a constant-0 border, 15-bit weights. */
#include <limits.h>
#include <math.h>
#include <stdint.h>

static int to_fixed(float m) {
    const float p = m * 32.f;
    return (p > -2147483648.f && p < 2147483648.f) ? (int)lrintf(p) : INT_MIN;
}

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

void lens_remap_host(const uint8_t *src, int sw, int sh, int sstep, const float *map1, const float *map2, int dw, int dh, uint8_t *dst) {
    for (int y = 0; y < dh; y++)
        for (int x = 0; x < dw; x++) {
            const int fx = to_fixed(map1[(long)y * dw + x]), fy = to_fixed(map2[(long)y * dw + x]);
            const int sx = clampi(fx >> 5, -32768, 32767), sy = clampi(fy >> 5, -32768, 32767), ax = fx & 31, ay = fy & 31;
            int w0 = (32 - ax) * (32 - ay) * 32, w1 = ax * (32 - ay) * 32, w2 = (32 - ax) * ay * 32, w3 = ax * ay * 32;
            if (ax == 0 && ay == 0) w0 = 32767, w3 = 1;
            int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
            if (sx >= 0 && sy >= 0 && sx < sw - 1 && sy < sh - 1) {
                const uint8_t *S = src + (long)sy * sstep + sx;
                v0 = S[0], v1 = S[1], v2 = S[sstep], v3 = S[sstep + 1];
            } else if (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0) {
                dst[(long)y * dw + x] = 0;
                continue;
            } else {
                if (sx >= 0 && sy >= 0) v0 = src[(long)sy * sstep + sx];
                if (sx + 1 < sw && sy >= 0) v1 = src[(long)sy * sstep + sx + 1];
                if (sx >= 0 && sy + 1 < sh) v2 = src[(long)(sy + 1) * sstep + sx];
                if (sx + 1 < sw && sy + 1 < sh) v3 = src[(long)(sy + 1) * sstep + sx + 1];
            }
            dst[(long)y * dw + x] = (uint8_t)clampi((v0 * w0 + v1 * w1 + v2 * w2 + v3 * w3 + (1 << 14)) >> 15, 0, 255);
        }
}
