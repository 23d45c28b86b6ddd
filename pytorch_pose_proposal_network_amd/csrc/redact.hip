// Redaction of the detected people in raw video frames (contract in include/ppn.h, ppn_redact_cells / ppn_redact_yuv; NumPy
// restatement tests/redact_ref.py).  Two kernels, no atomics, plain vector stores.
//
//   redact_cells_kernel   one workgroup per (stream, 256 mask words).  It stages the cell rectangles of a group of frames in
//                         LDS (at most 1024 x int4), then every work item ORs the rectangles into ITS mask word of each of
//                         those frames and counts its own 32 ttl bytes, which stay in registers over the frames of the call:
//                         a cell's history depends on no other cell, so the frames of a stream need no ordering between
//                         workgroups.  The file is built with -ffp-contract=off: hh + hh * margin stays a multiply and an
//                         add, as in crops.hip.
//   redact_kernel         one wave per cell: the wave reads the cell's samples, reduces one integer sum per channel across
//                         its lanes, and stores the rounded means (or the fill bytes); out of place it copies an unmasked
//                         cell.  A plane's part of a cell is a byte rectangle whose channels repeat with period 1 (a luma or
//                         I420 chroma plane), 2 (NV12's UV), 3 (packed BGR) or 4 (YUYV: Y U Y V), so one device function
//                         serves every plane of every format, with dword or byte accesses.
#include "common.h"

#include <cmath>

namespace {

constexpr int CELLS_THREADS = 256;         // four waves stage a group's people; each wave scans the group's counts itself
constexpr int MAX_PEOPLE = 1024;
constexpr int WAVES = 4;                   // cells (waves) per workgroup of redact_kernel

struct CellsArgs {
    ppn_redact_cells_cfg c;
    unsigned char* ttl;          // [S][CH][CW] or NULL (hold == 0)
    const int* count;            // [S * T]
    const int* kp_cell;          // [S * T][M][K]
    const float* bbox;           // [S * T][M][K][4]
    int frames;
    unsigned* mask;              // [S * T][CH][MW]
    int* flags;                  // [S * T]
    int CH, CW, MW;
};

__device__ __forceinline__ bool finite1(float v) { return fabsf(v) <= 3.402823466e38f; }     // false for a NaN
__device__ __forceinline__ bool finite4(const float4& b) { return finite1(b.x) && finite1(b.y) && finite1(b.z) && finite1(b.w); }

struct Span {
    float c, half;
};

__device__ __forceinline__ Span centre(float lo, float hi, float margin) {
    const float c = (lo + hi) * 0.5f;
    float half = (hi - lo) * 0.5f;
    half = half + half * margin;
    return {c, half};
}

// Rule 4 along one axis: [e0, e1) in pixels, limited to the picture; false: an edge is not finite.
__device__ __forceinline__ bool edges(const Span& s, int size, int& e0, int& e1) {
    const float lo = floorf(s.c - s.half), hi = ceilf(s.c + s.half);
    if (!(finite1(lo) && finite1(hi))) return false;
    const float fs = (float)size;
    e0 = (int)fminf(fmaxf(lo, 0.0f), fs);
    e1 = (int)fminf(fmaxf(hi, 0.0f), fs);
    return true;
}

// Rules 1 to 5 for person `row` of an image: (first row, last row, first column, last column) in cells, (1, 0, 1, 0) for
// nothing (no root included).  The loads do not depend on each other's values: kp_cell as one batch, the boxes six at a time
// (a box outside the set is loaded and dropped).
__device__ int4 person_cells(const CellsArgs& a, size_t row, bool& bad) {
    const int4 nothing = make_int4(1, 0, 1, 0);
    const int K = a.c.K;
    unsigned present = 0;
#pragma unroll
    for (int j = 0; j < PPN_MAX_KP; ++j) {
        const int v = a.kp_cell[row + min(j, K - 1)];
        present |= j < K && v >= 0 ? 1u << j : 0u;
    }
    if (!(present & 1u)) return nothing;
    unsigned set = present & a.c.kp_mask;
    if (!set) {
        if (a.c.fallback == PPN_REDACT_FALLBACK_NONE) return nothing;
        set = present;
    }
    const float4* boxes = reinterpret_cast<const float4*>(a.bbox) + row;
    float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool first = true, fin = true;
#pragma unroll 6
    for (int j = 0; j < K; ++j) {
        const float4 v = boxes[j];
        if (!(set >> j & 1u)) continue;
        fin = fin && finite4(v);
        if (first) {
            b = v;
            first = false;
        } else {
            b.x = v.x < b.x ? v.x : b.x;
            b.y = v.y < b.y ? v.y : b.y;
            b.z = v.z > b.z ? v.z : b.z;
            b.w = v.w > b.w ? v.w : b.w;
        }
    }
    if (!fin) {
        bad = true;
        return nothing;
    }
    const Span sy = centre(b.x * a.c.sy, b.z * a.c.sy, a.c.margin);
    const Span sx = centre(b.y * a.c.sx, b.w * a.c.sx, a.c.margin);
    int t, bt, l, r;
    if (!(edges(sy, a.c.src_h, t, bt) && edges(sx, a.c.src_w, l, r))) {
        bad = true;
        return nothing;
    }
    if (t >= bt || l >= r) return nothing;
    const int cell = a.c.cell;
    return make_int4(t / cell, (bt - 1) / cell, l / cell, (r - 1) / cell);
}

// The frames of a stream are taken in groups: as many consecutive frames (at most 64) as have MAX_PEOPLE people together,
// at least one.  A group's people are staged in one pass over (frame, person) pairs, so a quiet stream pays the latency of
// the loads once per call, not once per frame.
__global__ __launch_bounds__(CELLS_THREADS) void redact_cells_kernel(CellsArgs a) {
    __shared__ int4 rect[MAX_PEOPLE];
    __shared__ int first[64 + 1];                                            // where a frame's people start in rect
    __shared__ unsigned bad_of[CELLS_THREADS / 64][2];                       // per wave: the frames with a bad box, as bits
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.y, M = a.c.max_humans, K = a.c.K, hold = a.c.hold;
    const int q = blockIdx.x * CELLS_THREADS + tid;                          // this work item's mask word of every frame
    const bool own = q < a.CH * a.MW;
    const int cy = own ? q / a.MW : 0, wx = own ? q - cy * a.MW : 0, c0 = wx * 32;
    const int nbits = own ? min(32, a.CW - c0) : 0;
    unsigned char* ttl = hold > 0 ? a.ttl + ((size_t)s * a.CH + cy) * a.CW + c0 : nullptr;
    unsigned char life[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) life[k] = hold > 0 && k < nbits ? ttl[k] : 0;

    for (int t0 = 0; t0 < a.frames;) {
        const size_t b0 = (size_t)s * a.frames + t0;
        const int avail = min(64, a.frames - t0);
        const int P = lane < avail ? min(max(a.count[b0 + lane], 0), M) : 0; // lane i of every wave: frame t0 + i
        int incl = P;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d) incl += v;
        }
        const unsigned long long fits = __ballot(lane < avail && incl <= MAX_PEOPLE);     // a prefix of the lanes; lane 0 is in it
        const int G = ~fits ? __ffsll((long long)~fits) - 1 : 64;
        if (wave == 0 && lane < G) first[lane] = incl - P;
        if (wave == 0 && lane == G - 1) first[G] = incl;
        __syncthreads();
        const int n = first[G];
        unsigned bad_lo = 0, bad_hi = 0;
        for (int g = tid; g < n; g += CELLS_THREADS) {
            int lo = 0, hi = G - 1;                                          // the last frame that starts at or before g
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (first[mid] <= g) lo = mid;
                else hi = mid - 1;
            }
            bool bad = false;
            rect[g] = person_cells(a, ((b0 + lo) * M + (g - first[lo])) * K, bad);
            if (bad) (lo < 32 ? bad_lo : bad_hi) |= 1u << (lo & 31);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            bad_lo |= __shfl_xor(bad_lo, m);
            bad_hi |= __shfl_xor(bad_hi, m);
        }
        if (lane == 0) {
            bad_of[wave][0] = bad_lo;
            bad_of[wave][1] = bad_hi;
        }
        __syncthreads();
        if (blockIdx.x == 0 && tid < G) {
            unsigned bad = 0;
            for (int w = 0; w < CELLS_THREADS / 64; ++w) bad |= bad_of[w][tid >> 5];
            a.flags[b0 + tid] = bad >> (tid & 31) & 1u ? PPN_REDACT_FLAG_BAD_BOX : 0;
        }
        if (own) {
            for (int i = 0; i < G; ++i) {
                unsigned bits = 0;
                for (int p = first[i]; p < first[i + 1]; ++p) {
                    const int4 r = rect[p];                                  // one address for the wave: a broadcast
                    const int lo = max(r.z, c0) - c0, hi = min(r.w, c0 + 31) - c0;
                    if (cy >= r.x && cy <= r.y && lo <= hi) bits |= (0xffffffffu >> (31 - (hi - lo))) << lo;
                }
                if (hold > 0) {
                    unsigned held = 0;
#pragma unroll
                    for (int k = 0; k < 32; ++k) {
                        if (k < nbits) {
                            const int v = bits >> k & 1u ? hold + 1 : (life[k] > 0 ? life[k] - 1 : 0);
                            life[k] = (unsigned char)v;
                            held |= v > 0 ? 1u << k : 0u;
                        }
                    }
                    bits = held;
                }
                a.mask[((b0 + i) * a.CH + cy) * a.MW + wx] = bits;
            }
        }
        __syncthreads();                                                     // the next group overwrites rect and first
        t0 += G;
    }
    if (hold > 0) {
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < nbits) ttl[k] = life[k];
    }
}

// ---- masks -> surfaces --------------------------------------------------------------------------------------------------
struct Planes {
    unsigned char *y, *u, *v;
    int64_t frame_stride;
    int pitch, pitch_c;
};

struct RedactArgs {
    Planes s, d;
    const unsigned* mask;        // [batch][CH][MW]
    int height, width, cell, CH, CW, MW, mode;
    unsigned fill;               // fill[0] | fill[1] << 8 | fill[2] << 16
};

// the channel of byte k of a period of P bytes
template <int P>
__device__ __forceinline__ int chan(int k) {
    return P == 1 ? 0 : P == 4 ? ((k & 1) ? 1 + (k >> 1) : 0) : k;          // YUYV: Y U Y V -> 0 1 0 2
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Integer divisions are the bulk of a cell's instructions when done in integers; the operands here are small enough for
// one f32 multiply.  u / n for 0 <= u < 2^16 and 1 <= n <= 4096, rcp = 1 / n to an ulp: (u + 0.5) / n lies at least 0.5 / n
// from an integer and the product is off by less than 2^-22 of its value, so the truncation is exact.
__device__ __forceinline__ float rcp_of(int n) { return __builtin_amdgcn_rcpf((float)n); }
__device__ __forceinline__ int div_small(int u, float rcp) { return (int)(((float)u + 0.5f) * rcp); }

// (s + (n >> 1)) / n for a sum of n <= 1024 bytes: the numerator stays below 2^18 and the quotient below 256, so the same
// argument holds with a margin of 0.5 / 1024 against an error below 256 * 2^-22.
__device__ __forceinline__ unsigned rounded_mean(int s, int n) { return (unsigned)div_small(s + (n >> 1), rcp_of(n)); }

// V bytes (the row's last unit: nb < V of them) at p, byte i in bits 8 i .. 8 i + 7
template <int V>
__device__ __forceinline__ unsigned load_unit(const unsigned char* p, int nb) {
    if (V == 4 && nb == 4) return *reinterpret_cast<const unsigned*>(p);
    unsigned w = 0;
    for (int i = 0; i < nb; ++i) w |= (unsigned)p[i] << (8 * i);
    return w;
}

template <int V>
__device__ __forceinline__ void store_unit(unsigned char* p, int nb, unsigned w) {
    if (V == 4 && nb == 4) {
        *reinterpret_cast<unsigned*>(p) = w;
        return;
    }
    for (int i = 0; i < nb; ++i) p[i] = (unsigned char)(w >> (8 * i));
}

// One plane's part of a cell: `rows` rows of `wbytes` bytes at s (pitch ps) -> d (pitch pd), channels of period P starting
// with channel 0 at byte 0, accessed V bytes at a time (V == 4: s, d and both pitches are multiples of 4; a row's last
// wbytes % 4 bytes go as bytes).  `fill`: the FILL bytes of channels 0, 1, 2 in bits 0..23.  All 64 lanes of the wave call
// every member.  The work is cut into partial (loads), finish (cross-lane sums) and store so that a cell's planes can be
// loaded together, before the first reduction.
template <int P, int V>
struct Region {
    const unsigned char* s;
    unsigned char* d;
    int ps, pd, rows, wbytes;
    unsigned fill;

    __device__ __forceinline__ int upr() const { return (wbytes + V - 1) / V; }

    // this lane's share of the channels' sums
    __device__ __forceinline__ void partial(int lane, int (&acc)[3]) const {
        const int n = upr(), total = rows * n;
        const float rn = rcp_of(n);
        for (int u = lane; u < total; u += 64) {
            const int r = div_small(u, rn), o = (u - r * n) * V, nb = min(V, wbytes - o);
            const unsigned w = load_unit<V>(s + (size_t)r * ps + o, nb);     // bytes beyond nb are 0: they add nothing
            int k = o % P;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int byte = (int)(w >> (8 * i) & 255u), ch = chan<P>(k);
                acc[0] += ch == 0 ? byte : 0;
                if (P > 1) acc[1] += ch == 1 ? byte : 0;
                if (P > 2) acc[2] += ch == 2 ? byte : 0;
                k = k + 1 == P ? 0 : k + 1;
            }
        }
    }

    // the rounded means of channels 0, 1, 2 in bits 0..23; the reads of the region end here
    __device__ __forceinline__ unsigned finish(const int (&acc)[3]) const {
        const int per = rows * (wbytes / P);                                 // samples of a channel that stands once in the period
        const int n0 = P == 4 ? 2 * per : per;
        unsigned val = rounded_mean(wave_sum(acc[0]), n0);
        if (P > 1) val |= rounded_mean(wave_sum(acc[1]), per) << 8;
        if (P > 2) val |= rounded_mean(wave_sum(acc[2]), per) << 16;
        return val;
    }

    __device__ __forceinline__ void store(unsigned val, int lane) const {
        const int n = upr(), total = rows * n;
        const float rn = rcp_of(n);
        for (int u = lane; u < total; u += 64) {
            const int r = div_small(u, rn), o = (u - r * n) * V, nb = min(V, wbytes - o);
            unsigned w = 0;
            int k = o % P;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                w |= (val >> (8 * chan<P>(k)) & 255u) << (8 * i);
                k = k + 1 == P ? 0 : k + 1;
            }
            store_unit<V>(d + (size_t)r * pd + o, nb, w);
        }
    }

    // out of place only: the surfaces do not overlap
    __device__ __forceinline__ void copy(int lane) const {
        const unsigned char* __restrict__ from = s;
        unsigned char* __restrict__ to = d;
        const int n = upr(), total = rows * n;
        const float rn = rcp_of(n);
        for (int u = lane; u < total; u += 64) {
            const int r = div_small(u, rn), o = (u - r * n) * V, nb = min(V, wbytes - o);
            store_unit<V>(to + (size_t)r * pd + o, nb, load_unit<V>(from + (size_t)r * ps + o, nb));
        }
    }
};

// A cell's regions: all loads, then the reductions, then the stores.
template <class... R>
__device__ __forceinline__ void redact_cell(bool masked, int mode, int lane, const R&... r) {
    if (!masked) {
        (r.copy(lane), ...);
        return;
    }
    if (mode == PPN_REDACT_FILL) {
        (r.store(r.fill, lane), ...);
        return;
    }
    int acc[sizeof...(R)][3] = {};
    unsigned val[sizeof...(R)];
    int i = 0;
    (r.partial(lane, acc[i++]), ...);
    i = 0;
    ((val[i] = r.finish(acc[i]), ++i), ...);
    i = 0;
    (r.store(val[i++], lane), ...);
}

template <int FMT, int V, bool INPLACE>
__global__ __launch_bounds__(WAVES * 64) void redact_kernel(RedactArgs a) {
    const int lane = threadIdx.x & 63;
    const int cx = blockIdx.x * WAVES + (threadIdx.x >> 6), cy = blockIdx.y;
    const size_t b = blockIdx.z;
    if (cx >= a.CW) return;                                                  // whole waves: cx is the wave's
    const unsigned word = a.mask[(b * a.CH + cy) * a.MW + (cx >> 5)];
    const bool masked = __builtin_amdgcn_readfirstlane((int)(word >> (cx & 31) & 1u)) != 0;
    if (INPLACE && !masked) return;
    const int x0 = cx * a.cell, y0 = cy * a.cell;
    const int cols = min(a.cell, a.width - x0), rows = min(a.cell, a.height - y0);
    const size_t fs = b * (size_t)a.s.frame_stride, fd = b * (size_t)a.d.frame_stride;
    const unsigned f0 = a.fill & 255u, f1 = a.fill >> 8 & 255u, f2 = a.fill >> 16 & 255u;
    if (FMT == PPN_PIX_YUYV) {
        redact_cell(masked, a.mode, lane,
                    Region<4, V>{a.s.y + fs + (size_t)y0 * a.s.pitch + 2 * x0, a.d.y + fd + (size_t)y0 * a.d.pitch + 2 * x0,
                                 a.s.pitch, a.d.pitch, rows, 2 * cols, a.fill});
    } else if (FMT == PPN_PIX_BGR24) {
        redact_cell(masked, a.mode, lane,
                    Region<3, V>{a.s.y + fs + (size_t)y0 * a.s.pitch + 3 * x0, a.d.y + fd + (size_t)y0 * a.d.pitch + 3 * x0,
                                 a.s.pitch, a.d.pitch, rows, 3 * cols, a.fill});
    } else {
        const Region<1, V> luma{a.s.y + fs + (size_t)y0 * a.s.pitch + x0, a.d.y + fd + (size_t)y0 * a.d.pitch + x0, a.s.pitch,
                                a.d.pitch, rows, cols, f0};
        const size_t cs = fs + (size_t)(y0 / 2) * a.s.pitch_c, cd = fd + (size_t)(y0 / 2) * a.d.pitch_c;
        if (FMT == PPN_PIX_NV12) {
            redact_cell(masked, a.mode, lane, luma,
                        Region<2, V>{a.s.u + cs + x0, a.d.u + cd + x0, a.s.pitch_c, a.d.pitch_c, rows / 2, cols, f1 | f2 << 8});
        } else {
            redact_cell(masked, a.mode, lane, luma,
                        Region<1, V>{a.s.u + cs + x0 / 2, a.d.u + cd + x0 / 2, a.s.pitch_c, a.d.pitch_c, rows / 2, cols / 2, f1},
                        Region<1, V>{a.s.v + cs + x0 / 2, a.d.v + cd + x0 / 2, a.s.pitch_c, a.d.pitch_c, rows / 2, cols / 2, f2});
        }
    }
}

// what ppn_redact_yuv refuses of one surface: ppn_draw_humans_yuv's list, with packed BGR accepted
int check_surface(const char* who, const char* name, const ppn_yuv_surface* s) {
    if (!s) return ppn::fail(PPN_E_INVALID, "%s: NULL %s surface", who, name);
    const int fmt = s->format;
    if (fmt != PPN_PIX_NV12 && fmt != PPN_PIX_I420 && fmt != PPN_PIX_YUYV && fmt != PPN_PIX_BGR24)
        return ppn::fail(PPN_E_INVALID, "%s: %s: unknown format %d", who, name, fmt);
    const bool bgr = fmt == PPN_PIX_BGR24, is420 = fmt == PPN_PIX_NV12 || fmt == PPN_PIX_I420;
    if (!bgr && s->matrix != 0 && s->matrix != 1) return ppn::fail(PPN_E_INVALID, "%s: %s: unknown matrix %d", who, name, s->matrix);
    if (!s->y || (is420 && !s->u) || (fmt == PPN_PIX_I420 && !s->v)) return ppn::fail(PPN_E_INVALID, "%s: %s: NULL plane", who, name);
    if (s->height < 1 || s->width < 1 || s->height > 16384 || s->width > 16384)
        return ppn::fail(PPN_E_INVALID, "%s: %s: bad size %dx%d (1..16384)", who, name, s->height, s->width);
    if (!bgr && ((s->width & 1) || (is420 && (s->height & 1))))
        return ppn::fail(PPN_E_INVALID, "%s: %s: odd size %dx%d", who, name, s->height, s->width);
    const int64_t row = bgr ? 3 * (int64_t)s->width : is420 ? s->width : 2 * (int64_t)s->width;
    const int64_t row_c = fmt == PPN_PIX_NV12 ? s->width : s->width / 2;
    if (s->pitch < row || (is420 && s->pitch_c < row_c))
        return ppn::fail(PPN_E_INVALID, "%s: %s: pitch %d / %d below the row's %lld / %lld bytes", who, name, s->pitch, s->pitch_c,
                         (long long)row, (long long)row_c);
    const int64_t plane = (int64_t)(s->height - 1) * s->pitch + row;
    const int64_t plane_c = is420 ? (int64_t)(s->height / 2 - 1) * s->pitch_c + row_c : 0;
    if (s->frame_stride < plane || s->frame_stride < plane_c)
        return ppn::fail(PPN_E_INVALID, "%s: %s: frame_stride %lld smaller than a plane (%lld bytes)", who, name,
                         (long long)s->frame_stride, (long long)(plane > plane_c ? plane : plane_c));
    return PPN_OK;
}

Planes planes_of(const ppn_yuv_surface* s) {
    const bool is420 = s->format == PPN_PIX_NV12 || s->format == PPN_PIX_I420;
    return {static_cast<unsigned char*>(s->y), is420 ? static_cast<unsigned char*>(s->u) : nullptr,
            s->format == PPN_PIX_I420 ? static_cast<unsigned char*>(s->v) : nullptr, s->frame_stride, s->pitch,
            is420 ? s->pitch_c : 0};
}

// every plane, pitch and stride of the surface allows dword accesses to a cell's rows (a cell's row starts at a multiple of
// 4 bytes in every plane of every format)
bool dword_aligned(const Planes& p) {
    auto off = [](const void* q) { return reinterpret_cast<uintptr_t>(q) % 4 != 0; };
    return !(off(p.y) || off(p.u) || off(p.v) || p.pitch % 4 || p.pitch_c % 4 || p.frame_stride % 4);
}

template <int FMT>
void launch_redact(bool inplace, bool dwords, dim3 grid, hipStream_t st, const RedactArgs& a) {
    if (inplace && dwords) redact_kernel<FMT, 4, true><<<grid, WAVES * 64, 0, st>>>(a);
    else if (inplace) redact_kernel<FMT, 1, true><<<grid, WAVES * 64, 0, st>>>(a);
    else if (dwords) redact_kernel<FMT, 4, false><<<grid, WAVES * 64, 0, st>>>(a);
    else redact_kernel<FMT, 1, false><<<grid, WAVES * 64, 0, st>>>(a);
}

bool cell_ok(int cell) { return cell == 8 || cell == 16 || cell == 32; }

}  // namespace

extern "C" int ppn_redact_cells(const ppn_redact_cells_cfg* cfg, uint8_t* ttl, const int32_t* count, const int32_t* kp_cell,
                                const float* bbox, int32_t streams, int32_t frames, uint32_t* mask, int32_t* flags,
                                void* stream) {
    static const char who[] = "ppn_redact_cells";
    if (!cfg || !count || !kp_cell || !bbox || !mask || !flags) return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", who);
    const ppn_redact_cells_cfg& c = *cfg;
    if (c.hold < 0 || c.hold > 254) return ppn::fail(PPN_E_INVALID, "%s: hold %d outside 0..254", who, c.hold);
    if (c.hold > 0 && !ttl) return ppn::fail(PPN_E_INVALID, "%s: NULL ttl with hold %d", who, c.hold);
    if (c.K < 1 || c.K > PPN_MAX_KP) return ppn::fail(PPN_E_INVALID, "%s: K %d outside 1..%d", who, c.K, PPN_MAX_KP);
    if (c.max_humans < 1 || c.max_humans > MAX_PEOPLE || streams < 1 || streams > 65535 || frames < 1 || c.src_h < 1 ||
        c.src_w < 1 || c.src_h > 16384 || c.src_w > 16384 || (int64_t)streams * frames > INT32_MAX)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry (%d streams x %d frames, max_humans %d outside 1..%d, picture %dx%d)",
                         who, streams, frames, c.max_humans, MAX_PEOPLE, c.src_h, c.src_w);
    if (!cell_ok(c.cell)) return ppn::fail(PPN_E_INVALID, "%s: cell %d is not 8, 16 or 32", who, c.cell);
    if (!std::isfinite(c.sy) || !std::isfinite(c.sx) || !(c.sy > 0.0f) || !(c.sx > 0.0f))
        return ppn::fail(PPN_E_INVALID, "%s: scales %g, %g must be finite and positive", who, (double)c.sy, (double)c.sx);
    if (!std::isfinite(c.margin) || c.margin < 0.0f)
        return ppn::fail(PPN_E_INVALID, "%s: margin %g must be finite and not negative", who, (double)c.margin);
    if (c.fallback != PPN_REDACT_FALLBACK_PERSON && c.fallback != PPN_REDACT_FALLBACK_NONE)
        return ppn::fail(PPN_E_INVALID, "%s: unknown fallback %d", who, c.fallback);
    if (!(c.kp_mask & (c.K >= 32 ? 0xffffffffu : (1u << c.K) - 1u)))
        return ppn::fail(PPN_E_INVALID, "%s: kp_mask 0x%x names no keypoint below K %d", who, c.kp_mask, c.K);
    if (reinterpret_cast<uintptr_t>(bbox) % 16) return ppn::fail(PPN_E_INVALID, "%s: bbox must be 16-byte aligned", who);
    CellsArgs a{c, ttl, count, kp_cell, bbox, frames, mask, flags, 0, 0, 0};
    a.CH = (c.src_h + c.cell - 1) / c.cell;
    a.CW = (c.src_w + c.cell - 1) / c.cell;
    a.MW = (a.CW + 31) / 32;
    const dim3 grid((unsigned)((a.CH * a.MW + CELLS_THREADS - 1) / CELLS_THREADS), (unsigned)streams);
    redact_cells_kernel<<<grid, CELLS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_redact_yuv(const ppn_redact_cfg* cfg, const ppn_yuv_surface* src, const ppn_yuv_surface* dst, int32_t batch,
                              const uint32_t* mask, void* stream) {
    static const char who[] = "ppn_redact_yuv";
    if (!cfg || !mask) return ppn::fail(PPN_E_INVALID, "%s: NULL cfg or mask", who);
    if (!cell_ok(cfg->cell)) return ppn::fail(PPN_E_INVALID, "%s: cell %d is not 8, 16 or 32", who, cfg->cell);
    if (cfg->mode != PPN_REDACT_MOSAIC && cfg->mode != PPN_REDACT_FILL)
        return ppn::fail(PPN_E_INVALID, "%s: unknown mode %d", who, cfg->mode);
    if (batch < 1 || batch > 65535) return ppn::fail(PPN_E_INVALID, "%s: batch %d outside 1..65535", who, batch);
    if (int rc = check_surface(who, "src", src)) return rc;
    if (int rc = check_surface(who, "dst", dst)) return rc;
    const bool yuv = src->format != PPN_PIX_BGR24;
    if (src->format != dst->format || src->height != dst->height || src->width != dst->width ||
        (yuv && (src->matrix != dst->matrix || !src->full_range != !dst->full_range)))
        return ppn::fail(PPN_E_INVALID, "%s: src and dst differ in format, size, matrix or range", who);
    const Planes ps = planes_of(src), pd = planes_of(dst);
    const bool all = ps.y == pd.y && ps.u == pd.u && ps.v == pd.v && ps.pitch == pd.pitch && ps.pitch_c == pd.pitch_c &&
                     ps.frame_stride == pd.frame_stride;
    const bool any = ps.y == pd.y || (ps.u && ps.u == pd.u) || (ps.v && ps.v == pd.v);
    if (any && !all)
        return ppn::fail(PPN_E_INVALID, "%s: dst shares a plane with src but not every plane and the geometry (in place means all)",
                         who);
    RedactArgs a{ps, pd, mask, src->height, src->width, cfg->cell, 0, 0, 0, cfg->mode,
                 (unsigned)cfg->fill[0] | (unsigned)cfg->fill[1] << 8 | (unsigned)cfg->fill[2] << 16};
    a.CH = (a.height + a.cell - 1) / a.cell;
    a.CW = (a.width + a.cell - 1) / a.cell;
    a.MW = (a.CW + 31) / 32;
    const bool dwords = dword_aligned(ps) && dword_aligned(pd);
    const dim3 grid((unsigned)((a.CW + WAVES - 1) / WAVES), (unsigned)a.CH, (unsigned)batch);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (src->format == PPN_PIX_NV12) launch_redact<PPN_PIX_NV12>(all, dwords, grid, st, a);
    else if (src->format == PPN_PIX_I420) launch_redact<PPN_PIX_I420>(all, dwords, grid, st, a);
    else if (src->format == PPN_PIX_YUYV) launch_redact<PPN_PIX_YUYV>(all, dwords, grid, st, a);
    else launch_redact<PPN_PIX_BGR24>(all, dwords, grid, st, a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
