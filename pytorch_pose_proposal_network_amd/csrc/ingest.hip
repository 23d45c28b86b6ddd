// Frame ingest on the device (/root/reference/rt_test.py:150-157 grab_frame): camera frame BGR u8
// [B,Hs,Ws,3] -> cv2.resize(INTER_LINEAR) -> flip vertically and horizontally -> RGB u8 [B,Hd,Wd,3], written
// straight into the conv plan's input buffer (the stem kernel normalises on load).  One thread per output pixel;
// the interpolation coefficients are recomputed per thread with OpenCV's own float/double operations
// (-ffp-contract=off: no fused multiply-add may change a rounding), so there are no tables to upload.
// HBM-bound: reads <= 4 source pixels per output pixel (L2 serves the overlap), writes 3 bytes.
// Arithmetic: oracle/ingest_ref.py states the rule (OpenCV's 8-bit fixed-point bilinear; PARITY UNPINNED, cv2 is not
// available in this image).
#include "common.h"
#include "windows.h"

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
// No LDS, no atomics; L2 serves the taps that neighbouring pixels share.  ppn_ingest_windows (further down) runs the same
// body on windows of the frames, and on packed BGR (PPN_PIX_BGR24: the tap is the pixel's three bytes).
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
    if (FMT == PPN_PIX_BGR24) {                           // packed B, G, R: the tap is the three bytes
        const unsigned char* r = py + (size_t)y * pitch + 3 * x;
        rgb[0] = r[2];
        rgb[1] = r[1];
        rgb[2] = r[0];
        return;
    }
    int Y, U, V;
    yuv_bytes<FMT>(py, pu, pv, pitch, pitch_c, y, x, Y, U, V);
    const int l = max(0, Y - k.yoff) * k.cy + (1 << 19), uu = U - 128, vv = V - 128;
    rgb[0] = sat8((l + k.cvr * vv) >> 20);
    rgb[1] = sat8((l + k.cvg * vv + k.cug * uu) >> 20);
    rgb[2] = sat8((l + k.cub * uu) >> 20);
}

// Four consecutive pixels (oy, ox0 .. ox0 + 3) of output image `img` from the picture of Hs x Ws pixels whose planes start at
// py / pu / pv: the whole body of both kernels below.  A window is a picture whose plane pointers are moved to its origin.
template <int FMT>
__device__ __forceinline__ void yuv_quad(const unsigned char* py, const unsigned char* pu, const unsigned char* pv, int pitch,
                                         int pitch_c, const YuvCoeff& k, unsigned char* __restrict__ dst, int img, int Hs,
                                         int Ws, int Hd, int Wd, double scale_x, double scale_y, int flip, int bgr, int area2,
                                         int dwords, int oy, int ox0) {
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
        yuv_tap<FMT>(py, pu, pv, pitch, pitch_c, k, y0, x0, p00);
        yuv_tap<FMT>(py, pu, pv, pitch, pitch_c, k, y0, x1, p01);
        yuv_tap<FMT>(py, pu, pv, pitch, pitch_c, k, y1, x0, p10);
        yuv_tap<FMT>(py, pu, pv, pitch, pitch_c, k, y1, x1, p11);
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
    unsigned char* o = dst + (((size_t)img * Hd + oy) * Wd + ox0) * 3;
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
    yuv_quad<FMT>(py, pu, pv, s.pitch, s.pitch_c, k, dst, b, Hs, Ws, Hd, Wd, scale_x, scale_y, flip, bgr, area2, dwords, oy,
                  ox0);
}

// ---- windows of raw frames (include/ppn.h: ppn_ingest_windows) ---------------------------------------------------------
// Image f * n + i is window i of frame f.  The layout travels by value in the kernel arguments (a uniform index: scalar
// loads); per window the host supplies the two scales and the exact-halving choice.
struct WinArgs {
    int n;
    ppn_window win[PPN_MAX_WINDOWS];
    double scale_x[PPN_MAX_WINDOWS], scale_y[PPN_MAX_WINDOWS];
    int area2[PPN_MAX_WINDOWS];
};

template <int FMT>
__global__ void __launch_bounds__(256)
ingest_windows_kernel(YuvSrc s, YuvCoeff k, WinArgs wa, unsigned char* __restrict__ dst, int Hd, int Wd, int flip, int bgr,
                      int dwords) {
    const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int oy = blockIdx.y * blockDim.y + threadIdx.y;
    const int img = blockIdx.z;
    if (ox0 >= Wd || oy >= Hd) return;
    const int f = img / wa.n, i = img - f * wa.n;
    const ppn_window w = wa.win[i];
    // the window's planes: y0 and x0 are even wherever chroma is shared, so sample (y >> 1, x >> 1) of the window is the
    // frame's sample of the same pixel
    const unsigned char* py = s.y + (long long)f * s.frame_stride + (long long)w.y0 * s.pitch;
    const unsigned char *pu = nullptr, *pv = nullptr;
    if (FMT == PPN_PIX_NV12) {
        py += w.x0;
        pu = s.u + (long long)f * s.frame_stride + (long long)(w.y0 >> 1) * s.pitch_c + w.x0;
    } else if (FMT == PPN_PIX_I420) {
        py += w.x0;
        const long long o = (long long)f * s.frame_stride + (long long)(w.y0 >> 1) * s.pitch_c + (w.x0 >> 1);
        pu = s.u + o;
        pv = s.v + o;
    } else if (FMT == PPN_PIX_YUYV) {
        py += 2 * w.x0;
    } else {
        py += 3 * w.x0;
    }
    yuv_quad<FMT>(py, pu, pv, s.pitch, s.pitch_c, k, dst, img, w.h, w.w, Hd, Wd, wa.scale_x[i], wa.scale_y[i], flip, bgr,
                  wa.area2[i], dwords, oy, ox0);
}

// ---- regions of interest of raw frames (include/ppn.h: ppn_ingest_rois) ------------------------------------------------
// Image f * max_rois + r is ROI r of frame f.  The rectangles are a table in device memory (ppn_people_rois writes it), read
// per workgroup at a uniform address; nothing about it is known on the host, so the workgroup judges its rectangle before
// any tap and the two scales are divided here.  An empty or bad slot gets zero bytes and never touches the source.
template <int FMT>
__global__ void __launch_bounds__(256)
ingest_rois_kernel(YuvSrc s, YuvCoeff k, const int* __restrict__ roi, int* __restrict__ status, int max_rois, int Hs, int Ws,
                   unsigned char* __restrict__ dst, int Hd, int Wd, int flip, int bgr, int dwords) {
    const int ox0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int oy = blockIdx.y * blockDim.y + threadIdx.y;
    const int img = blockIdx.z;
    const int* q = roi + (size_t)img * 4;
    const int y0 = q[0], x0 = q[1], h = q[2], w = q[3];
    int bits = 0;
    if ((y0 | x0 | h | w) == 0) {
        bits = PPN_ROI_EMPTY;
    } else {
        bool bad = y0 < 0 || x0 < 0 || h < 1 || w < 1 || h > Hs || w > Ws || y0 > Hs - h || x0 > Ws - w;
        if (FMT != PPN_PIX_BGR24) bad = bad || ((x0 | w) & 1);
        if (FMT == PPN_PIX_NV12 || FMT == PPN_PIX_I420) bad = bad || ((y0 | h) & 1);
        if (bad) bits = PPN_ROI_BAD;
    }
    if (bits) {                                            // uniform: the whole workgroup leaves without a tap
        if (status && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) status[img] |= bits;
        if (ox0 >= Wd || oy >= Hd) return;
        unsigned char* o = dst + (((size_t)img * Hd + oy) * Wd + ox0) * 3;
        if (dwords) {
            unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
            o4[0] = 0u;
            o4[1] = 0u;
            o4[2] = 0u;
        } else {
            const int n = min(4, Wd - ox0) * 3;
            for (int j = 0; j < n; ++j) o[j] = 0;
        }
        return;
    }
    if (ox0 >= Wd || oy >= Hd) return;
    const int f = img / max_rois;
    const unsigned char* py = s.y + (long long)f * s.frame_stride + (long long)y0 * s.pitch;
    const unsigned char *pu = nullptr, *pv = nullptr;
    if (FMT == PPN_PIX_NV12) {
        py += x0;
        pu = s.u + (long long)f * s.frame_stride + (long long)(y0 >> 1) * s.pitch_c + x0;
    } else if (FMT == PPN_PIX_I420) {
        py += x0;
        const long long o = (long long)f * s.frame_stride + (long long)(y0 >> 1) * s.pitch_c + (x0 >> 1);
        pu = s.u + o;
        pv = s.v + o;
    } else if (FMT == PPN_PIX_YUYV) {
        py += 2 * x0;
    } else {
        py += 3 * x0;
    }
    const int area2 = (h == 2 * Hd && w == 2 * Wd) ? 1 : 0;
    yuv_quad<FMT>(py, pu, pv, s.pitch, s.pitch_c, k, dst, img, h, w, Hd, Wd, (double)w / (double)Wd, (double)h / (double)Hd,
                  flip, bgr, area2, dwords, oy, ox0);
}

}  // namespace

extern "C" int ppn_yuv_coefficients(int32_t matrix, int32_t full_range, int32_t out6[6]) {
    if (!out6) return ppn::fail(PPN_E_INVALID, "ppn_yuv_coefficients: NULL output");
    if (matrix != 0 && matrix != 1) return ppn::fail(PPN_E_INVALID, "ppn_yuv_coefficients: unknown matrix %d", matrix);
    for (int i = 0; i < 6; ++i) out6[i] = kYuvCoeff[(full_range ? 2 : 0) + matrix][i];
    return PPN_OK;
}

namespace {

// The refusals both raw-frame entries share; `who` names the entry in the message.  bgr_ok: PPN_PIX_BGR24 is a format.
int check_desc(const char* who, const ppn_ingest_desc* d, bool bgr_ok) {
    if (!d) return ppn::fail(PPN_E_INVALID, "%s: NULL descriptor", who);
    const int fmt = d->format;
    if (fmt != PPN_PIX_NV12 && fmt != PPN_PIX_I420 && fmt != PPN_PIX_YUYV && !(bgr_ok && fmt == PPN_PIX_BGR24))
        return ppn::fail(PPN_E_INVALID, "%s: unknown format %d", who, fmt);
    if (d->matrix != 0 && d->matrix != 1) return ppn::fail(PPN_E_INVALID, "%s: unknown matrix %d", who, d->matrix);
    const bool is420 = fmt == PPN_PIX_NV12 || fmt == PPN_PIX_I420;
    if (!d->dst || !d->y || (is420 && !d->u) || (fmt == PPN_PIX_I420 && !d->v))
        return ppn::fail(PPN_E_INVALID, "%s: NULL buffer", who);
    if (d->batch < 1 || d->src_h < 1 || d->src_w < 1 || d->dst_h < 1 || d->dst_w < 1 || d->batch > 65535 ||
        d->dst_h > 65535 || d->src_h > 16384 || d->src_w > 16384)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry %d x %dx%d -> %dx%d", who, d->batch, d->src_h, d->src_w, d->dst_h,
                         d->dst_w);
    if (fmt != PPN_PIX_BGR24 && ((d->src_w & 1) || (is420 && (d->src_h & 1))))
        return ppn::fail(PPN_E_INVALID, "%s: odd source size %dx%d", who, d->src_h, d->src_w);
    // bytes of one row and of one frame's plane (last row tight), luma / packed and chroma
    const int64_t row = is420 ? d->src_w : (fmt == PPN_PIX_YUYV ? 2 : 3) * (int64_t)d->src_w;
    const int64_t row_c = fmt == PPN_PIX_NV12 ? d->src_w : d->src_w / 2;
    if (d->pitch < row || (is420 && d->pitch_c < row_c))
        return ppn::fail(PPN_E_INVALID, "%s: pitch %d / %d below the row's %lld / %lld bytes", who, d->pitch, d->pitch_c,
                         (long long)row, (long long)row_c);
    const int64_t plane = (int64_t)(d->src_h - 1) * d->pitch + row;
    const int64_t plane_c = is420 ? (int64_t)(d->src_h / 2 - 1) * d->pitch_c + row_c : 0;
    if (d->frame_stride < plane || d->frame_stride < plane_c)
        return ppn::fail(PPN_E_INVALID, "%s: frame_stride %lld smaller than a plane (%lld bytes)", who,
                         (long long)d->frame_stride, (long long)(plane > plane_c ? plane : plane_c));
    return PPN_OK;
}

YuvCoeff coeff_of(const ppn_ingest_desc* d) {
    const int32_t* c = kYuvCoeff[(d->full_range ? 2 : 0) + d->matrix];
    return {c[0], c[1], c[2], c[3], c[4], c[5]};
}

YuvSrc planes_of(const ppn_ingest_desc* d) {
    const bool is420 = d->format == PPN_PIX_NV12 || d->format == PPN_PIX_I420;
    return {static_cast<const unsigned char*>(d->y), is420 ? static_cast<const unsigned char*>(d->u) : nullptr,
            d->format == PPN_PIX_I420 ? static_cast<const unsigned char*>(d->v) : nullptr, d->frame_stride, d->pitch,
            is420 ? d->pitch_c : 0};
}

}  // namespace

extern "C" int ppn_ingest_yuv(const ppn_ingest_desc* d, void* stream) {
    if (const int rc = check_desc("ppn_ingest_yuv", d, false)) return rc;
    const int fmt = d->format;
    const YuvCoeff k = coeff_of(d);
    const YuvSrc s = planes_of(d);
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

extern "C" int ppn_ingest_windows(const ppn_ingest_desc* d, const ppn_window_layout* lay, void* stream) {
    static const char who[] = "ppn_ingest_windows";
    if (const int rc = check_desc(who, d, true)) return rc;
    if (const int rc = ppn::check_layout(who, lay)) return rc;
    const int fmt = d->format;
    const bool yuv = fmt != PPN_PIX_BGR24, is420 = fmt == PPN_PIX_NV12 || fmt == PPN_PIX_I420;
    WinArgs wa;
    wa.n = lay->n;
    for (int i = 0; i < PPN_MAX_WINDOWS; ++i) {
        const ppn_window w = i < lay->n ? lay->win[i] : lay->win[0];      // unused entries: a copy of the first
        if (i < lay->n) {
            if ((int64_t)w.y0 + w.h > d->src_h || (int64_t)w.x0 + w.w > d->src_w)
                return ppn::fail(PPN_E_INVALID, "%s: window %d (%d, %d) %dx%d leaves the %dx%d picture", who, i, w.y0, w.x0,
                                 w.h, w.w, d->src_h, d->src_w);
            if ((yuv && ((w.x0 | w.w) & 1)) || (is420 && ((w.y0 | w.h) & 1)))
                return ppn::fail(PPN_E_INVALID, "%s: window %d (%d, %d) %dx%d must be even where chroma is shared", who, i,
                                 w.y0, w.x0, w.h, w.w);
        }
        wa.win[i] = w;
        wa.scale_x[i] = (double)w.w / (double)d->dst_w;
        wa.scale_y[i] = (double)w.h / (double)d->dst_h;
        wa.area2[i] = (w.h == 2 * d->dst_h && w.w == 2 * d->dst_w) ? 1 : 0;
    }
    if ((int64_t)d->batch * lay->n > 65535)
        return ppn::fail(PPN_E_INVALID, "%s: %d frames x %d windows exceed 65535 images", who, d->batch, lay->n);
    const YuvCoeff k = coeff_of(d);
    const YuvSrc s = planes_of(d);
    const int dwords = (d->dst_w % 4 == 0 && (reinterpret_cast<uintptr_t>(d->dst) & 3) == 0) ? 1 : 0;
    const dim3 block(32, 8), grid((d->dst_w + 127) / 128, (d->dst_h + 7) / 8, d->batch * lay->n);
    unsigned char* dst = static_cast<unsigned char*>(d->dst);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define PPN_WIN_LAUNCH(F)                                                                                                \
    hipLaunchKernelGGL(ingest_windows_kernel<F>, grid, block, 0, st, s, k, wa, dst, d->dst_h, d->dst_w, d->flip ? 1 : 0, \
                       d->dst_bgr ? 1 : 0, dwords)
    if (fmt == PPN_PIX_NV12) PPN_WIN_LAUNCH(PPN_PIX_NV12);
    else if (fmt == PPN_PIX_I420) PPN_WIN_LAUNCH(PPN_PIX_I420);
    else if (fmt == PPN_PIX_YUYV) PPN_WIN_LAUNCH(PPN_PIX_YUYV);
    else PPN_WIN_LAUNCH(PPN_PIX_BGR24);
#undef PPN_WIN_LAUNCH
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_ingest_rois(const ppn_ingest_desc* d, const int32_t* roi, int32_t max_rois, int32_t* status,
                               void* stream) {
    static const char who[] = "ppn_ingest_rois";
    if (const int rc = check_desc(who, d, true)) return rc;
    if (!roi) return ppn::fail(PPN_E_INVALID, "%s: NULL roi table", who);
    if (max_rois < 1) return ppn::fail(PPN_E_INVALID, "%s: max_rois %d below 1", who, max_rois);
    if ((int64_t)d->batch * max_rois > 65535)
        return ppn::fail(PPN_E_INVALID, "%s: %d frames x %d ROIs exceed 65535 images", who, d->batch, max_rois);
    const int fmt = d->format;
    const YuvCoeff k = coeff_of(d);
    const YuvSrc s = planes_of(d);
    const int dwords = (d->dst_w % 4 == 0 && (reinterpret_cast<uintptr_t>(d->dst) & 3) == 0) ? 1 : 0;
    const dim3 block(32, 8), grid((d->dst_w + 127) / 128, (d->dst_h + 7) / 8, d->batch * max_rois);
    unsigned char* dst = static_cast<unsigned char*>(d->dst);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define PPN_ROI_LAUNCH(F)                                                                                               \
    hipLaunchKernelGGL(ingest_rois_kernel<F>, grid, block, 0, st, s, k, roi, status, max_rois, d->src_h, d->src_w, dst, \
                       d->dst_h, d->dst_w, d->flip ? 1 : 0, d->dst_bgr ? 1 : 0, dwords)
    if (fmt == PPN_PIX_NV12) PPN_ROI_LAUNCH(PPN_PIX_NV12);
    else if (fmt == PPN_PIX_I420) PPN_ROI_LAUNCH(PPN_PIX_I420);
    else if (fmt == PPN_PIX_YUYV) PPN_ROI_LAUNCH(PPN_PIX_YUYV);
    else PPN_ROI_LAUNCH(PPN_PIX_BGR24);
#undef PPN_ROI_LAUNCH
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
