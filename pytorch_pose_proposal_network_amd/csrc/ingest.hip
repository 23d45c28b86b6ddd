// Frame ingest on the device (/root/reference/rt_test.py:150-157 grab_frame): camera frame BGR u8
// [B,Hs,Ws,3] -> cv2.resize(INTER_LINEAR) -> flip vertically and horizontally -> RGB u8 [B,Hd,Wd,3], written
// straight into the conv plan's input buffer (the stem kernel normalises on load).  One thread per output pixel;
// the interpolation coefficients are recomputed per thread with OpenCV's own float/double operations
// (-ffp-contract=off: no fused multiply-add may change a rounding), so there are no tables to upload.
// HBM-bound: reads <= 4 source pixels per output pixel (L2 serves the overlap), writes 3 bytes.
// Arithmetic: oracle/ingest_ref.py states the rule (OpenCV's 8-bit fixed-point bilinear; PARITY UNPINNED, cv2 is not
// available in this image).
#include "common.h"

namespace {

struct Axis {
    int s;          // first source index
    int a0, a1;     // 2^11 fixed-point weights of s and s + 1
};

__device__ __forceinline__ Axis axis_coeff(int d, int n_src, double scale) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
    Axis a;
    a.s = s;
    // saturate_cast<short>(cvRound(v * 2048)): round half to even, values are within [0, 2048]
    a.a0 = (int)rintf((1.f - f) * 2048.f);
    a.a1 = (int)rintf(f * 2048.f);
    return a;
}

__global__ void __launch_bounds__(256)
ingest_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int B, int Hs, int Ws, int Hd,
              int Wd, double scale_x, double scale_y, int flip, int swap_rb, int area2) {
    const int ox = blockIdx.x * blockDim.x + threadIdx.x;
    const int oy = blockIdx.y;
    const int b = blockIdx.z;
    if (ox >= Wd) return;
    // output (oy, ox) shows resized pixel (ry, rx): both flips of rt_test.py:154-155 = a rotation by 180 degrees
    const int ry = flip ? Hd - 1 - oy : oy, rx = flip ? Wd - 1 - ox : ox;
    const unsigned char* img = src + (size_t)b * Hs * Ws * 3;
    int v[3];
    if (area2) {
        const unsigned char* p0 = img + ((size_t)(2 * ry) * Ws + 2 * rx) * 3;
        const unsigned char* p1 = p0 + (size_t)Ws * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2;
    } else {
        const Axis ax = axis_coeff(rx, Ws, scale_x), ay = axis_coeff(ry, Hs, scale_y);
        const int x1 = min(ax.s + 1, Ws - 1), y1 = min(ay.s + 1, Hs - 1);
        const unsigned char* r0 = img + (size_t)ay.s * Ws * 3;
        const unsigned char* r1 = img + (size_t)y1 * Ws * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int t0 = r0[ax.s * 3 + c] * ax.a0 + r0[x1 * 3 + c] * ax.a1;
            const int t1 = r1[ax.s * 3 + c] * ax.a0 + r1[x1 * 3 + c] * ax.a1;
            v[c] = (((ay.a0 * (t0 >> 4)) >> 16) + ((ay.a1 * (t1 >> 4)) >> 16) + 2) >> 2;
        }
    }
    unsigned char* o = dst + (((size_t)b * Hd + oy) * Wd + ox) * 3;
    o[0] = (unsigned char)min(max(v[swap_rb ? 2 : 0], 0), 255);
    o[1] = (unsigned char)min(max(v[1], 0), 255);
    o[2] = (unsigned char)min(max(v[swap_rb ? 0 : 2], 0), 255);
}

}  // namespace

extern "C" int ppn_ingest_frames(const void* src_bgr, int32_t batch, int32_t src_h, int32_t src_w, void* dst_rgb,
                                 int32_t dst_h, int32_t dst_w, int32_t flip, int32_t swap_rb, void* stream) {
    if (!src_bgr || !dst_rgb) return ppn::fail(PPN_E_INVALID, "ppn_ingest_frames: NULL buffer");
    if (batch < 1 || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1 || batch > 65535 || dst_h > 65535)
        return ppn::fail(PPN_E_INVALID, "ppn_ingest_frames: bad geometry %d x %dx%d -> %dx%d", batch, src_h, src_w, dst_h,
                         dst_w);
    const int area2 = (src_h == 2 * dst_h && src_w == 2 * dst_w) ? 1 : 0;
    const dim3 grid((dst_w + 255) / 256, dst_h, batch);
    hipLaunchKernelGGL(ingest_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const unsigned char*>(src_bgr), static_cast<unsigned char*>(dst_rgb), batch, src_h,
                       src_w, dst_h, dst_w, (double)src_w / (double)dst_w, (double)src_h / (double)dst_h, flip ? 1 : 0,
                       swap_rb ? 1 : 0, area2);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

// ---- raw YUV frames (include/ppn.h: ppn_ingest_yuv) --------------------------------------------------------------------
// NV12 / I420 / YUYV planes -> RGB u8 [B,Hd,Wd,3] in one launch: the output pixel is what ingest_kernel's resize rule gives
// on the colour-converted full-resolution picture, so only the 4 taps an output pixel needs are converted (OpenCV's
// fixed-point YUV -> RGB, saturated per tap, then the interpolation above).  One thread makes 4 consecutive pixels of a
// row and stores them as three dwords where the row layout allows it; the taps are byte loads (planes of any alignment).
// No LDS, no atomics; L2 serves the taps that neighbouring pixels share.
namespace {

// round(c * 2^20) of the three-decimal constants; row 0 is OpenCV's ITUR_BT_601_{CY,CVR,CVG,CUG,CUB} (color_yuv.simd.hpp)
//                                          CY       CVR      CVG      CUG      CUB   yoff
constexpr int32_t kYuvCoeff[4][6] = {{1220542, 1673527, -852492, -409993, 2116026, 16},    // bt601 limited
                                     {1220542, 1880097, -558891, -223347, 2214593, 16},    // bt709 limited
                                     {1048576, 1470104, -748826, -360853, 1858077, 0},     // bt601 full
                                     {1048576, 1651297, -490864, -196423, 1945738, 0}};    // bt709 full

struct YuvCoeff {
    int cy, cvr, cvg, cug, cub, yoff;
};

struct YuvSrc {
    const unsigned char *y, *u, *v;     // frame 0 of each plane
    long long frame_stride;
    int pitch, pitch_c;
};

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// Where pixel (y, x)'s three bytes are: the only thing the format decides.
template <int FMT>
__device__ __forceinline__ void yuv_bytes(const unsigned char* py, const unsigned char* pu, const unsigned char* pv,
                                          int pitch, int pitch_c, int y, int x, int& Y, int& U, int& V) {
    if (FMT == PPN_PIX_NV12) {
        const unsigned char* c = pu + (size_t)(y >> 1) * pitch_c + (x >> 1) * 2;
        Y = py[(size_t)y * pitch + x];
        U = c[0];
        V = c[1];
    } else if (FMT == PPN_PIX_I420) {
        const size_t o = (size_t)(y >> 1) * pitch_c + (x >> 1);
        Y = py[(size_t)y * pitch + x];
        U = pu[o];
        V = pv[o];
    } else {
        const unsigned char* r = py + (size_t)y * pitch;
        Y = r[2 * x];
        U = r[(x >> 1) * 4 + 1];
        V = r[(x >> 1) * 4 + 3];
    }
}

template <int FMT>
__device__ __forceinline__ void yuv_tap(const unsigned char* py, const unsigned char* pu, const unsigned char* pv,
                                        int pitch, int pitch_c, const YuvCoeff& k, int y, int x, int (&rgb)[3]) {
    int Y, U, V;
    yuv_bytes<FMT>(py, pu, pv, pitch, pitch_c, y, x, Y, U, V);
    const int l = max(0, Y - k.yoff) * k.cy + (1 << 19), uu = U - 128, vv = V - 128;
    rgb[0] = sat8((l + k.cvr * vv) >> 20);
    rgb[1] = sat8((l + k.cvg * vv + k.cug * uu) >> 20);
    rgb[2] = sat8((l + k.cub * uu) >> 20);
}

template <int FMT>
__global__ void __launch_bounds__(256)
ingest_yuv_kernel(YuvSrc s, YuvCoeff k, unsigned char* __restrict__ dst, int Hs, int Ws, int Hd, int Wd, double scale_x,
                  double scale_y, int flip, int bgr, int area2, int dwords) {
    const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int oy = blockIdx.y * blockDim.y + threadIdx.y;
    const int b = blockIdx.z;
    if (ox0 >= Wd || oy >= Hd) return;
    const unsigned char* py = s.y + (long long)b * s.frame_stride;
    const unsigned char* pu = s.u ? s.u + (long long)b * s.frame_stride : nullptr;
    const unsigned char* pv = s.v ? s.v + (long long)b * s.frame_stride : nullptr;
    const int ry = flip ? Hd - 1 - oy : oy;
    int y0, y1;
    Axis ay = {0, 0, 0};
    if (area2) {
        y0 = 2 * ry;
        y1 = y0 + 1;
    } else {
        ay = axis_coeff(ry, Hs, scale_y);
        y0 = ay.s;
        y1 = min(ay.s + 1, Hs - 1);
    }
    unsigned char px[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ox = min(ox0 + i, Wd - 1);              // a tail thread recomputes the last pixel and does not store it
        const int rx = flip ? Wd - 1 - ox : ox;
        int x0, x1;
        Axis ax = {0, 0, 0};
        if (area2) {
            x0 = 2 * rx;
            x1 = x0 + 1;
        } else {
            ax = axis_coeff(rx, Ws, scale_x);
            x0 = ax.s;
            x1 = min(ax.s + 1, Ws - 1);
        }
        int p00[3], p01[3], p10[3], p11[3];
        yuv_tap<FMT>(py, pu, pv, s.pitch, s.pitch_c, k, y0, x0, p00);
        yuv_tap<FMT>(py, pu, pv, s.pitch, s.pitch_c, k, y0, x1, p01);
        yuv_tap<FMT>(py, pu, pv, s.pitch, s.pitch_c, k, y1, x0, p10);
        yuv_tap<FMT>(py, pu, pv, s.pitch, s.pitch_c, k, y1, x1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int v;
            if (area2) {
                v = (p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2;
            } else {
                const int t0 = p00[c] * ax.a0 + p01[c] * ax.a1;
                const int t1 = p10[c] * ax.a0 + p11[c] * ax.a1;
                v = (((ay.a0 * (t0 >> 4)) >> 16) + ((ay.a1 * (t1 >> 4)) >> 16) + 2) >> 2;
            }
            px[i * 3 + (bgr ? 2 - c : c)] = (unsigned char)sat8(v);
        }
    }
    unsigned char* o = dst + (((size_t)b * Hd + oy) * Wd + ox0) * 3;
    if (dwords) {                                         // Wd % 4 == 0 and dst 4-byte aligned: o is, and all 4 pixels exist
        unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o4[j] = (unsigned)px[4 * j] | (unsigned)px[4 * j + 1] << 8 | (unsigned)px[4 * j + 2] << 16 |
                    (unsigned)px[4 * j + 3] << 24;
    } else {
        const int n = min(4, Wd - ox0) * 3;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < n) o[j] = px[j];
    }
}

}  // namespace

extern "C" int ppn_yuv_coefficients(int32_t matrix, int32_t full_range, int32_t out6[6]) {
    if (!out6) return ppn::fail(PPN_E_INVALID, "ppn_yuv_coefficients: NULL output");
    if (matrix != 0 && matrix != 1) return ppn::fail(PPN_E_INVALID, "ppn_yuv_coefficients: unknown matrix %d", matrix);
    for (int i = 0; i < 6; ++i) out6[i] = kYuvCoeff[(full_range ? 2 : 0) + matrix][i];
    return PPN_OK;
}

extern "C" int ppn_ingest_yuv(const ppn_ingest_desc* d, void* stream) {
    if (!d) return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: NULL descriptor");
    const int fmt = d->format;
    if (fmt != PPN_PIX_NV12 && fmt != PPN_PIX_I420 && fmt != PPN_PIX_YUYV)
        return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: unknown format %d", fmt);
    if (d->matrix != 0 && d->matrix != 1) return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: unknown matrix %d", d->matrix);
    if (!d->dst || !d->y || (fmt != PPN_PIX_YUYV && !d->u) || (fmt == PPN_PIX_I420 && !d->v))
        return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: NULL buffer");
    if (d->batch < 1 || d->src_h < 1 || d->src_w < 1 || d->dst_h < 1 || d->dst_w < 1 || d->batch > 65535 ||
        d->dst_h > 65535 || d->src_h > 16384 || d->src_w > 16384)
        return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: bad geometry %d x %dx%d -> %dx%d", d->batch, d->src_h, d->src_w,
                         d->dst_h, d->dst_w);
    const bool is420 = fmt != PPN_PIX_YUYV;
    if ((d->src_w & 1) || (is420 && (d->src_h & 1)))
        return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: odd source size %dx%d", d->src_h, d->src_w);
    // bytes of one row and of one frame's plane (last row tight), luma / packed and chroma
    const int64_t row = is420 ? d->src_w : 2 * (int64_t)d->src_w;
    const int64_t row_c = fmt == PPN_PIX_NV12 ? d->src_w : d->src_w / 2;
    if (d->pitch < row || (is420 && d->pitch_c < row_c))
        return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: pitch %d / %d below the row's %lld / %lld bytes", d->pitch,
                         d->pitch_c, (long long)row, (long long)row_c);
    const int64_t plane = (int64_t)(d->src_h - 1) * d->pitch + row;
    const int64_t plane_c = is420 ? (int64_t)(d->src_h / 2 - 1) * d->pitch_c + row_c : 0;
    if (d->frame_stride < plane || d->frame_stride < plane_c)
        return ppn::fail(PPN_E_INVALID, "ppn_ingest_yuv: frame_stride %lld smaller than a plane (%lld bytes)",
                         (long long)d->frame_stride, (long long)(plane > plane_c ? plane : plane_c));
    const int32_t* c = kYuvCoeff[(d->full_range ? 2 : 0) + d->matrix];
    const YuvCoeff k = {c[0], c[1], c[2], c[3], c[4], c[5]};
    const YuvSrc s = {static_cast<const unsigned char*>(d->y), is420 ? static_cast<const unsigned char*>(d->u) : nullptr,
                      fmt == PPN_PIX_I420 ? static_cast<const unsigned char*>(d->v) : nullptr, d->frame_stride, d->pitch,
                      is420 ? d->pitch_c : 0};
    const int area2 = (d->src_h == 2 * d->dst_h && d->src_w == 2 * d->dst_w) ? 1 : 0;
    const int dwords = (d->dst_w % 4 == 0 && (reinterpret_cast<uintptr_t>(d->dst) & 3) == 0) ? 1 : 0;
    // 32 x 8 threads = 128 x 8 output pixels per workgroup; a wave stores two 384-byte row pieces
    const dim3 block(32, 8), grid((d->dst_w + 127) / 128, (d->dst_h + 7) / 8, d->batch);
    const double sx = (double)d->src_w / (double)d->dst_w, sy = (double)d->src_h / (double)d->dst_h;
    unsigned char* dst = static_cast<unsigned char*>(d->dst);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define PPN_YUV_LAUNCH(F)                                                                                             \
    hipLaunchKernelGGL(ingest_yuv_kernel<F>, grid, block, 0, st, s, k, dst, d->src_h, d->src_w, d->dst_h, d->dst_w, sx, \
                       sy, d->flip ? 1 : 0, d->dst_bgr ? 1 : 0, area2, dwords)
    if (fmt == PPN_PIX_NV12) PPN_YUV_LAUNCH(PPN_PIX_NV12);
    else if (fmt == PPN_PIX_I420) PPN_YUV_LAUNCH(PPN_PIX_I420);
    else PPN_YUV_LAUNCH(PPN_PIX_YUYV);
#undef PPN_YUV_LAUNCH
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
