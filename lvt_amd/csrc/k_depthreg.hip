// k_depthreg.hip -- RGB-D from unaligned sensors: the depth plane of a second camera registered to the colour image inside the feature stage
// (lvt_amd_set_depth_camera; include/lvt_amd_ext.h has the definition, tests/depth_reg_util.py restates it in numpy bit for bit).
//   k_depth_clear    : every fp32 word of the registered plane(s) of a step, padding included, becomes +inf.
//   k_depth_register : a z-buffered scatter.  A thread owns one depth pixel: it projects the pixel's two corners and its centre into the raw (distorted)
//                      colour pixel grid -- where k_gather samples the plane --, and every colour pixel centre inside the half-open footprint box takes
//                      min(current, Zc of the centre).  Positive finite floats order like their bit patterns, so the minimum is an unsigned integer
//                      minimum taken by device-scope atomics (workgroups on different XCDs meet on one pixel): the result does not depend on arrival order.
// All arithmetic is fp32, one IEEE operation per written operation (the library is built with -ffp-contract=off; divisions are correctly rounded).
// The descriptors travel BY VALUE like RectTable / GrayTable; blockIdx.y = image, the grid's x extent follows the largest image of the launch and a smaller
// image's surplus workgroups leave at the top.  No LDS, no scratch.
#include "lvt_dev.h"

namespace lvt {

struct DepthRegImg {
    const void *src;       // the sensor's depth plane: float (DEPTH_F32) or uint16_t (DEPTH_U16) elements, aligned to its element
    float *dst;            // registered plane, fp32, on the colour pixel grid
    int src_pitch;         // ELEMENTS of the source format
    int fmt;               // DEPTH_F32 / DEPTH_U16
    float scale;           // DEPTH_U16: metres per raw unit
    int dw, dh;            // the depth camera's image
    float fx, fy, cx, cy;  // ... its pinhole
    float R[9], t[3];      // p_colour = R p_depth + t
    float cfx, cfy, ccx, ccy, k1, k2, p1, p2, k3;  // the colour camera
    int W, H;              // ... its image
    int dst_pitch;         // ELEMENTS (fp32 words) per row of dst
};
constexpr int DEPTHREG_PACK = 24;  // images per launch; a step with more registered sequences takes several launches
struct DepthRegTable {
    DepthRegImg im[DEPTHREG_PACK];
};
static_assert(sizeof(DepthRegTable) < 4096, "the depth registration kernels' arguments must stay under 4096 bytes");
constexpr int DEPTHREG_MAX_SPAN = 16;  // a footprint this many pixels wide or tall is a calibration error: skipped (and the cap bounds the loop)

// a thread owns four consecutive words of rows x pitch (a 16-byte store where the plane's base allows it)
__global__ __launch_bounds__(256) void k_depth_clear(DepthRegTable tab) {
    const DepthRegImg &I = tab.im[blockIdx.y];  // (uniform index: the descriptor stays in scalar registers)
    const size_t n = (size_t)I.dst_pitch * I.H;
    const size_t w0 = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4;
    if (w0 >= n) return;  // (a smaller image's surplus workgroups leave here as a whole)
    const uint32_t inf = 0x7F800000u;
    uint32_t *d = reinterpret_cast<uint32_t *>(I.dst) + w0;
    if (w0 + 4 <= n && ((uintptr_t)I.dst & 15) == 0) {
        *reinterpret_cast<uint4 *>(d) = make_uint4(inf, inf, inf, inf);
    } else {
        for (size_t k = 0; k < 4 && w0 + k < n; k++) d[k] = inf;
    }
}

// depth pixel (a, b) with depth z -> the colour camera: the raw pixel (u, v) and the depth Zc there
__device__ __forceinline__ void depthreg_proj(const DepthRegImg &I, float a, float b, float z, float &u, float &v, float &Zc) {
    const float X = ((a - I.cx) / I.fx) * z;
    const float Y = ((b - I.cy) / I.fy) * z;
    const float Xc = (I.R[0] * X + I.R[1] * Y) + I.R[2] * z + I.t[0];
    const float Yc = (I.R[3] * X + I.R[4] * Y) + I.R[5] * z + I.t[1];
    Zc = (I.R[6] * X + I.R[7] * Y) + I.R[8] * z + I.t[2];
    const float x = Xc / Zc, y = Yc / Zc;
    const float r2 = x * x + y * y;
    const float rad = 1.f + r2 * (I.k1 + r2 * (I.k2 + r2 * I.k3));
    const float xd = x * rad + (2.f * I.p1 * x * y + I.p2 * (r2 + 2.f * x * x));
    const float yd = y * rad + (I.p1 * (r2 + 2.f * y * y) + 2.f * I.p2 * x * y);
    u = xd * I.cfx + I.ccx;
    v = yd * I.cfy + I.ccy;
}
__device__ __forceinline__ bool depthreg_small(float f) { return fabsf(f) < 1e6f; }  // (false for NaN and infinities)

__global__ __launch_bounds__(256) void k_depth_register(DepthRegTable tab) {
    const DepthRegImg &I = tab.im[blockIdx.y];
    const unsigned px = blockIdx.x * 256u + threadIdx.x;  // (dw, dh <= 8192: dw * dh fits)
    if (px >= (unsigned)(I.dw * I.dh)) return;  // (a smaller image's surplus workgroups leave here as a whole)
    const int j = (int)(px / (unsigned)I.dw), i = (int)(px - (unsigned)j * (unsigned)I.dw);
    // consecutive lanes read consecutive elements of a source row, at the source's own pitch and format
    const size_t si = (size_t)j * I.src_pitch + i;
    const float z = (I.fmt == DEPTH_U16) ? __fmul_rn((float)static_cast<const uint16_t *>(I.src)[si], I.scale) : static_cast<const float *>(I.src)[si];
    if (!(z > 0.f && z < __builtin_inff())) return;  // (NaN fails the first comparison)
    float u0, v0, u1, v1, uc, vc, zq, Zc;
    depthreg_proj(I, (float)i - 0.5f, (float)j - 0.5f, z, u0, v0, zq);
    depthreg_proj(I, (float)i + 0.5f, (float)j + 0.5f, z, u1, v1, zq);
    depthreg_proj(I, (float)i, (float)j, z, uc, vc, Zc);
    if (!(Zc > 0.f && Zc < __builtin_inff())) return;
    if (!(depthreg_small(u0) && depthreg_small(v0) && depthreg_small(u1) && depthreg_small(v1))) return;
    int x0 = (int)ceilf(u0), x1 = (int)ceilf(u1) - 1;  // the pixel centres in [u0, u1) x [v0, v1): the top-left rule
    int y0 = (int)ceilf(v0), y1 = (int)ceilf(v1) - 1;
    if (x1 - x0 >= DEPTHREG_MAX_SPAN || y1 - y0 >= DEPTHREG_MAX_SPAN) return;
    x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, I.W - 1), y1 = min(y1, I.H - 1);  // (every write lies inside W x H of the destination)
    const unsigned zb = __float_as_uint(Zc);
    unsigned *D = reinterpret_cast<unsigned *>(I.dst);
    for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++)
            (void)__hip_atomic_fetch_min(D + (size_t)y * I.dst_pitch + x, zb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace lvt
