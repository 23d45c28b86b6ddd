// Rectangles of the detected people, written on the device for ppn_ingest_rois (contract in include/ppn.h, ppn_people_rois;
// NumPy restatement tests/crops_ref.py).  One work item per (frame, slot): slot r is person r, so there is nothing to sort or
// to compact, and a slot without a person still gets its (0, 0, 0, 0) and PPN_ROI_EMPTY -- every slot of both tables is
// written by exactly one work item with plain vector stores.  No LDS, no atomics.  The file is built with -ffp-contract=off
// and IEEE division: hh + hh * margin stays a multiply and an add, hw / aspect is rounded as NumPy rounds it.
#include "common.h"

#include <cmath>

namespace {

constexpr int THREADS = 64;

struct RoiArgs {
    ppn_roi_cfg c;
    const int* count;            // [F]
    const int* kp_cell;          // [F][M][K]
    const float* bbox;           // [F][M][K][4] ymin, xmin, ymax, xmax in box pixels
    int frames;
    int* roi;                    // [F][max_rois][4] y0, x0, h, w
    int* status;                 // [F][max_rois]
};

__device__ __forceinline__ bool finite4(const float4& b) {
    return fabsf(b.x) <= 3.402823466e38f && fabsf(b.y) <= 3.402823466e38f && fabsf(b.z) <= 3.402823466e38f &&
           fabsf(b.w) <= 3.402823466e38f;                                    // false for a NaN
}

// Rules 4 to 6 along one axis: lo, hi mapped box edges -> [e0, e1) in pixels; false: an edge is not finite.
struct Span {
    float c, half;
};

__device__ __forceinline__ Span centre(float lo, float hi, float margin) {
    const float c = (lo + hi) * 0.5f;
    float half = (hi - lo) * 0.5f;
    half = half + half * margin;
    return {c, half};
}

__device__ __forceinline__ bool edges(const Span& s, int size, int align, int& e0, int& e1) {
    const float lo = floorf(s.c - s.half), hi = ceilf(s.c + s.half);
    if (!(fabsf(lo) <= 3.402823466e38f && fabsf(hi) <= 3.402823466e38f)) return false;
    const float fs = (float)size;
    const int i0 = (int)fminf(fmaxf(lo, 0.0f), fs), i1 = (int)fminf(fmaxf(hi, 0.0f), fs);
    e0 = i0 & ~(align - 1);
    e1 = (i1 + align - 1) & ~(align - 1);
    return true;
}

__global__ __launch_bounds__(THREADS) void people_rois_kernel(RoiArgs a) {
    const int R = a.c.max_rois, M = a.c.max_humans, K = a.c.K;
    const int q = blockIdx.x * THREADS + threadIdx.x;
    if (q >= a.frames * R) return;
    const int f = q / R, r = q - f * R;

    int st = PPN_ROI_EMPTY;
    int4 out = make_int4(0, 0, 0, 0);
    const int P = min(max(a.count[f], 0), M);
    const size_t row = ((size_t)f * M + r) * K;                              // read only when r < P <= M
    if (r < P && a.kp_cell[row] >= 0) {
        st = PPN_ROI_DEGENERATE;
        const float4* boxes = reinterpret_cast<const float4*>(a.bbox) + row;
        float4 b = boxes[0];
        bool fin = finite4(b);
        if (a.c.mode == PPN_ROI_MODE_PEOPLE) {
            for (int j = 1; j < K; ++j) {
                if (a.kp_cell[row + j] < 0) continue;
                const float4 v = boxes[j];
                fin = fin && finite4(v);
                b.x = v.x < b.x ? v.x : b.x;
                b.y = v.y < b.y ? v.y : b.y;
                b.z = v.z > b.z ? v.z : b.z;
                b.w = v.w > b.w ? v.w : b.w;
            }
        }
        if (fin) {
            Span sy = centre(b.x * a.c.sy, b.z * a.c.sy, a.c.margin);
            Span sx = centre(b.y * a.c.sx, b.w * a.c.sx, a.c.margin);
            if (a.c.aspect > 0.0f) {
                const float want = sy.half * a.c.aspect;
                if (sx.half < want) sx.half = want;
                else sy.half = sx.half / a.c.aspect;
            }
            int y0, y1, x0, x1;
            if (edges(sy, a.c.src_h, a.c.align_y, y0, y1) && edges(sx, a.c.src_w, a.c.align_x, x0, x1)) {
                const int h = y1 - y0, w = x1 - x0;
                if (h >= a.c.min_size && w >= a.c.min_size) {
                    st = PPN_ROI_OK;
                    out = make_int4(y0, x0, h, w);
                }
            }
        }
    }
    reinterpret_cast<int4*>(a.roi)[q] = out;
    a.status[q] = st;
}

}  // namespace

extern "C" int ppn_people_rois(const ppn_roi_cfg* cfg, const int32_t* count, const int32_t* kp_cell, const float* bbox,
                               int32_t frames, int32_t* roi, int32_t* status, void* stream) {
    static const char who[] = "ppn_people_rois";
    if (!cfg || !count || !kp_cell || !bbox || !roi || !status) return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", who);
    const ppn_roi_cfg& c = *cfg;
    if (c.K < 1 || c.K > PPN_MAX_KP) return ppn::fail(PPN_E_INVALID, "%s: K %d outside 1..%d", who, c.K, PPN_MAX_KP);
    if (c.max_humans < 1 || c.max_humans > PPN_MATCH_MAX_PEOPLE || c.max_rois < 1 || frames < 1 || c.src_h < 1 ||
        c.src_w < 1 || c.src_h > 16384 || c.src_w > 16384 || (int64_t)frames * c.max_rois > INT32_MAX)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry (%d frames, max_humans %d outside 1..%d, max_rois %d, picture %dx%d)",
                         who, frames, c.max_humans, PPN_MATCH_MAX_PEOPLE, c.max_rois, c.src_h, c.src_w);
    if ((c.align_y != 1 && c.align_y != 2) || (c.align_x != 1 && c.align_x != 2) || c.src_h % c.align_y || c.src_w % c.align_x)
        return ppn::fail(PPN_E_INVALID, "%s: alignment %d x %d must be 1 or 2 and divide the %dx%d picture", who, c.align_y,
                         c.align_x, c.src_h, c.src_w);
    if (c.min_size < 1 || c.min_size < c.align_y || c.min_size < c.align_x)
        return ppn::fail(PPN_E_INVALID, "%s: min_size %d below 1 or below the alignment %d x %d", who, c.min_size, c.align_y,
                         c.align_x);
    if (c.mode != PPN_ROI_MODE_ROOT && c.mode != PPN_ROI_MODE_PEOPLE)
        return ppn::fail(PPN_E_INVALID, "%s: unknown mode %d", who, c.mode);
    if (!std::isfinite(c.sy) || !std::isfinite(c.sx) || !(c.sy > 0.0f) || !(c.sx > 0.0f))
        return ppn::fail(PPN_E_INVALID, "%s: scales %g, %g must be finite and positive", who, (double)c.sy, (double)c.sx);
    if (!std::isfinite(c.margin) || c.margin < 0.0f || !std::isfinite(c.aspect) || c.aspect < 0.0f)
        return ppn::fail(PPN_E_INVALID, "%s: margin %g and aspect %g must be finite and not negative", who, (double)c.margin,
                         (double)c.aspect);
    if (reinterpret_cast<uintptr_t>(bbox) % 16 || reinterpret_cast<uintptr_t>(roi) % 16)
        return ppn::fail(PPN_E_INVALID, "%s: bbox and roi must be 16-byte aligned", who);
    const RoiArgs a{c, count, kp_cell, bbox, frames, roi, status};
    const unsigned blocks = (unsigned)(((int64_t)frames * c.max_rois + THREADS - 1) / THREADS);
    people_rois_kernel<<<blocks, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
