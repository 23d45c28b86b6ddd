// Draw the decoded people onto u8 RGB frames on the device (datatest.py:162-232, draw_humans): a tiled rasteriser over the
// compact decode result, bit-exact with what PIL's ImageDraw paints for the same calls (rules in include/ppn.h, NumPy
// restatement tests/render_ref.py).
//
//   draw_setup_kernel    one thread per (image, person, slot): slot < K is the keypoint kp_order[slot], slot >= K the limb
//                        slot - K.  Writes an integer primitive record (four parameters, the coverage box clipped to the
//                        frame, type / colour / quad offsets) at index person * (K + E) + slot, which IS the paint order.
//                        Absent, skipped and wholly clipped primitives get an empty coverage box.
//   draw_raster_kernel   one workgroup per (image, tile of 32 * V x 8 pixels), one thread per V adjacent pixels of a row.
//                        256 primitives at a time are tested against the tile, a wave ballot + per-wave counts compact
//                        the hits into LDS in paint order; when the next 256 would not fit the list's CAP entries the list
//                        is resolved first (order-preserving chunks: a list is never truncated).  Resolving walks a chunk
//                        from its last entry down and stops at the first primitive covering the pixel; a later chunk
//                        overrides an earlier one.  In place only the drawn pixels are stored (3 bytes each); out of place
//                        every pixel is written, 12 bytes per thread as three dwords when the rows allow it (V = 4).
// All f32 arithmetic (midpoints, the scan line's x = (y - y0) * slope + x0, the slope's division) is written out in a fixed
// order and the file is built with -ffp-contract=off and IEEE division.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE_H = 8;        // rows of a tile; 32 threads (V pixels each) per row
constexpr int CAP = 256;         // LDS bin list entries (48 bytes each); a fuller list is drawn in chunks
enum { PRIM_NONE = 0, PRIM_ROOT = 1, PRIM_RECT = 2, PRIM_DISC = 3, PRIM_LINE = 4 };

struct DrawTables {
    int edge_src[PPN_MAX_EDGES], edge_dst[PPN_MAX_EDGES], kp_order[PPN_MAX_KP];
    unsigned colour[PPN_MAX_KP];                 // r | g << 8 | b << 16
};

struct SetupArgs {
    const int* count;            // [B]
    const int* kp_cell;          // [B][M][K]
    const float* bbox;           // [B][M][K][4] ymin, xmin, ymax, xmax
    int4* bb;                    // workspace: [B][N] coverage boxes, [B][N] parameters, [B][N] type / colour / offsets
    int4* par;
    int4* meta;
    int B, M, K, E, H, W, visbbox;
    DrawTables t;
};

// a keypoint takes part when it is present and its four box values are finite and below 2^20 in magnitude
__device__ __forceinline__ bool usable(const SetupArgs& a, size_t person, int k, float* box) {
    if (a.kp_cell[person * a.K + k] < 0) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        box[i] = a.bbox[(person * a.K + k) * 4 + i];
        ok = ok && fabsf(box[i]) < 1048576.f;                     // false for NaN and infinities
    }
    return ok;
}

// the record of primitive g = (image * M + person) * (K + E) + slot
__device__ __forceinline__ void build_primitive(const SetupArgs& a, long long g) {
    const int S = a.K + a.E;
    const long long N = (long long)a.M * S;
    if (g >= N * a.B) return;
    const int b = (int)(g / N);
    const int i = (int)(g % N);
    const int m = i / S, slot = i % S;
    if (m >= min(max(a.count[b], 0), a.M)) return;                // the raster pass never reads beyond the counted people
    const size_t person = (size_t)b * a.M + m;
    int4 par = make_int4(0, 0, 0, 0), meta = make_int4(PRIM_NONE, 0, 0, 0);
    int cx0 = 0, cy0 = 0, cx1 = -1, cy1 = -1;                     // coverage box before clipping (empty)
    float box[4], box2[4];
    if (slot < a.K) {
        const int k = a.t.kp_order[slot];
        if (usable(a, person, k, box)) {
            meta.y = (int)a.t.colour[k];
            if (k == 0 || a.visbbox) {
                par = make_int4((int)box[1], (int)box[0], (int)box[3], (int)box[2]);      // x0, y0, x1, y1
                if (par.z >= par.x && par.w >= par.y) {
                    meta.x = k == 0 ? PRIM_ROOT : PRIM_RECT;
                    cx0 = par.x; cy0 = par.y; cx1 = par.z; cy1 = par.w;
                }
            } else {
                const float x = (box[1] + box[3]) / 2.f, y = (box[0] + box[2]) / 2.f;
                const int bx0 = (int)(x - 2.f), by0 = (int)(y - 2.f), bx1 = (int)(x + 2.f), by1 = (int)(y + 2.f);
                par = make_int4(bx0, by0, bx1 - bx0, by1 - by0);
                meta.x = PRIM_DISC;
                cx0 = bx0; cy0 = by0; cx1 = bx1; cy1 = by1;
            }
        }
    } else {
        const int s = a.t.edge_src[slot - a.K], t = a.t.edge_dst[slot - a.K];
        if (usable(a, person, s, box) && usable(a, person, t, box2)) {
            const int x0 = (int)((box[1] + box[3]) / 2.f), y0 = (int)((box[0] + box[2]) / 2.f);
            const int x1 = (int)((box2[1] + box2[3]) / 2.f), y1 = (int)((box2[0] + box2[2]) / 2.f);
            meta.y = (int)a.t.colour[s];
            par = make_int4(x0, y0, x1, y1);
            if (x0 == x1 && y0 == y1) {
                meta.x = PRIM_RECT;                               // a zero vector is one pixel
                cx0 = cx1 = x0; cy0 = cy1 = y0;
            } else {
                // dxmax = RD(dy / hypot), dymax = RU(dx / hypot): +-1 exactly when 3 dy^2 > dx^2 (3 dx^2 > dy^2) -- a
                // tie would need 3 a^2 = b^2 in integers -- so the quad needs no square root
                const long long dx = (long long)x1 - x0, dy = (long long)y1 - y0;
                meta.x = PRIM_LINE;
                meta.z = 3 * dy * dy > dx * dx ? (dy > 0 ? 1 : -1) : 0;
                meta.w = 3 * dx * dx > dy * dy ? (dx > 0 ? 1 : -1) : 0;
                cx0 = min(x0, x1) - 1; cx1 = max(x0, x1) + 1; cy0 = min(y0, y1) - 1; cy1 = max(y0, y1) + 1;
            }
        }
    }
    cx0 = max(cx0, 0); cy0 = max(cy0, 0); cx1 = min(cx1, a.W - 1); cy1 = min(cy1, a.H - 1);
    if (cx0 > cx1 || cy0 > cy1) { cx0 = cy0 = 0x7fffffff; cx1 = cy1 = -1; meta.x = PRIM_NONE; }
    a.bb[g] = make_int4(cx0, cy0, cx1, cy1);
    a.par[g] = par;
    a.meta[g] = meta;
}

__global__ void __launch_bounds__(THREADS) draw_setup_kernel(SetupArgs a) {
    build_primitive(a, (long long)blockIdx.x * THREADS + threadIdx.x);
}

__device__ __forceinline__ int round_up(float f) { return f >= 0.f ? (int)floorf(f + 0.5f) : -(int)floorf(fabsf(f) + 0.5f); }
__device__ __forceinline__ int round_down(float f) { return f >= 0.f ? (int)ceilf(f - 0.5f) : -(int)ceilf(fabsf(f) - 0.5f); }

// bit j set: lo <= px + j <= hi
template <int V>
__device__ __forceinline__ unsigned span_mask(int lo, int hi, int px) {
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) m |= (px + j >= lo && px + j <= hi) ? 1u << j : 0u;
    return m;
}

__device__ __forceinline__ void cmpswap(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo; b = hi;
}

// PIL's polygon scan line over the quad of a width-2 line, row py: the pixels px .. px + V - 1 it fills
template <int V>
__device__ unsigned line_cover(int4 p, int dxmax, int dymax, int px, int py, int H) {
    const int vx[4] = {p.x, p.z, p.z + dxmax, p.x + dxmax};
    const int vy[4] = {p.y + dymax, p.w + dymax, p.w, p.y};
    int ymin = min(min(min(vy[0], vy[1]), min(vy[2], vy[3])), H - 1);
    int ymax = max(max(max(vy[0], vy[1]), max(vy[2], vy[3])), 0);
    ymin = max(ymin, 0); ymax = min(ymax, H);
    unsigned mask = 0;
    float xs[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ax = vx[e], ay = vy[e], bx = vx[(e + 1) & 3], by = vy[(e + 1) & 3];
        xs[2 * e] = xs[2 * e + 1] = INFINITY;
        if (ay == by) {                                           // a horizontal edge is its own line
            if (py == ay) mask |= span_mask<V>(min(ax, bx), max(ax, bx), px);
        } else if (py >= min(ay, by) && py <= max(ay, by) && py >= ymin && py <= ymax) {
            const float slope = (float)(bx - ax) / (float)(by - ay);
            const float x = (float)(py - ay) * slope + (float)ax;
            xs[2 * e] = x;
            if (py == max(ay, by) && py < ymax) xs[2 * e + 1] = x;
        }
    }
    // odd-even transposition sort of the eight slots (absent ones are +inf and end up last)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int i = r & 1; i + 1 < 8; i += 2) cmpswap(xs[i], xs[i + 1]);
    }
#pragma unroll
    for (int i = 1; i < 8; i += 2) {
        if (xs[i] < INFINITY) {
            const int lo = round_up(xs[i - 1]), hi = round_down(xs[i]);
            mask |= span_mask<V>(min(lo, hi), max(lo, hi), px);
        }
    }
    return mask;
}

template <int V>
__device__ __forceinline__ unsigned outline_mask(int x0, int y0, int x1, int y1, int px, int py) {
    if (x1 < x0 || y1 < y0 || py < y0 || py > y1) return 0;
    if (py == y0 || py == y1) return span_mask<V>(x0, x1, px);
    return span_mask<V>(x0, x0, px) | span_mask<V>(x1, x1, px);
}

template <int V>
__device__ __forceinline__ unsigned cover(int4 p, int4 m, int px, int py, int H) {
    switch (m.x) {
        case PRIM_ROOT:
            return outline_mask<V>(p.x, p.y, p.z, p.w, px, py) | outline_mask<V>(p.x + 1, p.y + 1, p.z - 1, p.w - 1, px, py);
        case PRIM_RECT:
            return outline_mask<V>(p.x, p.y, p.z, p.w, px, py);
        case PRIM_DISC: {
            const int dy = py - p.y;
            if (dy < 0 || dy > p.w) return 0;
            const bool end = dy == 0 || dy == p.w;                // the first and last row lose their corner pixels
            return span_mask<V>(p.x + (end ? 1 : 0), p.x + p.z - (end ? 1 : 0), px);
        }
        case PRIM_LINE:
            return line_cover<V>(p, m.z, m.w, px, py, H);
        default:
            return 0;
    }
}

struct RasterArgs {
    const unsigned char* src;    // [B][H][W][3]
    unsigned char* dst;
    const int* count;
    const int4* bb;
    const int4* par;
    const int4* meta;
    int B, M, S, H, W, grid, grid_step;
};

template <int V, bool INPLACE>
__global__ void __launch_bounds__(THREADS) draw_raster_kernel(RasterArgs a) {
    __shared__ int4 s_bb[CAP], s_par[CAP], s_meta[CAP];
    __shared__ int s_wave[THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * 32 * V, ty0 = blockIdx.y * TILE_H;
    const int tx1 = min(tx0 + 32 * V, a.W) - 1, ty1 = min(ty0 + TILE_H, a.H) - 1;
    const int px = tx0 + (t & 31) * V, py = ty0 + (t >> 5);
    unsigned inside = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) inside |= (px + j < a.W && py < a.H) ? 1u << j : 0u;
    unsigned hit = 0;
    unsigned col[V];
#pragma unroll
    for (int j = 0; j < V; ++j) col[j] = 0;

    // the last primitive of the list's first `cnt` entries that covers each pixel
    auto resolve = [&](int cnt) {
        unsigned todo = inside;
        for (int i = cnt - 1; i >= 0 && todo; --i) {
            const int4 bb = s_bb[i];
            if (py < bb.y || py > bb.w || px + V - 1 < bb.x || px > bb.z) continue;
            const int4 m = s_meta[i];
            const unsigned c = cover<V>(s_par[i], m, px, py, a.H) & todo;
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (c >> j & 1) col[j] = (unsigned)m.y;
            hit |= c;
            todo &= ~c;
        }
    };

    const int n = min(max(a.count[b], 0), a.M) * a.S;
    const size_t base = (size_t)b * a.M * a.S;
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += THREADS) {
        const int i = i0 + t;
        bool ov = false;
        int4 bb = make_int4(0, 0, -1, -1);
        if (i < n) {
            bb = a.bb[base + i];
            ov = bb.x <= tx1 && bb.z >= tx0 && bb.y <= ty1 && bb.w >= ty0;
        }
        const unsigned long long ballot = __ballot(ov);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (cnt + total > CAP) {                                  // uniform: draw what is binned, then start a new chunk
            resolve(cnt);
            cnt = 0;
            __syncthreads();
        }
        if (ov) {
            const int at = cnt + before + __popcll(ballot & ((1ull << lane) - 1ull));
            s_bb[at] = bb;
            s_par[at] = a.par[base + i];
            s_meta[at] = a.meta[base + i];
        }
        cnt += total;
        __syncthreads();
    }
    resolve(cnt);

    if (a.grid) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if ((inside >> j & 1) && ((px + j) % a.grid_step == 0 || py % a.grid_step == 0)) {
                col[j] = 110u | 110u << 8 | 110u << 16;
                hit |= 1u << j;
            }
        }
    }

    const size_t o = (((size_t)b * a.H + py) * a.W + px) * 3;
    if constexpr (INPLACE) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (hit >> j & 1) {
                a.dst[o + 3 * j] = (unsigned char)col[j];
                a.dst[o + 3 * j + 1] = (unsigned char)(col[j] >> 8);
                a.dst[o + 3 * j + 2] = (unsigned char)(col[j] >> 16);
            }
        }
    } else if constexpr (V == 4) {
        if (inside) {                                             // W % 4 == 0: the four pixels are in the frame together
            const unsigned* s4 = reinterpret_cast<const unsigned*>(a.src + o);
            unsigned q[3] = {s4[0], s4[1], s4[2]};
#pragma unroll
            for (int n8 = 0; n8 < 12; ++n8) {                     // byte n8 of the twelve: channel n8 % 3 of pixel n8 / 3
                if (hit >> (n8 / 3) & 1) {
                    const unsigned v = col[n8 / 3] >> (8 * (n8 % 3)) & 0xffu;
                    q[n8 / 4] = (q[n8 / 4] & ~(0xffu << (8 * (n8 % 4)))) | v << (8 * (n8 % 4));
                }
            }
            unsigned* d4 = reinterpret_cast<unsigned*>(a.dst + o);
            d4[0] = q[0]; d4[1] = q[1]; d4[2] = q[2];
        }
    } else {
        if (inside) {
            const bool h = hit & 1;
            a.dst[o] = h ? (unsigned char)col[0] : a.src[o];
            a.dst[o + 1] = h ? (unsigned char)(col[0] >> 8) : a.src[o + 1];
            a.dst[o + 2] = h ? (unsigned char)(col[0] >> 16) : a.src[o + 2];
        }
    }
}

int check_cfg(const ppn_draw_cfg* cfg, const char* who) {
    if (!cfg) return ppn::fail(PPN_E_INVALID, "%s: NULL cfg", who);
    if (cfg->K < 1 || cfg->K > PPN_MAX_KP || cfg->E < 0 || cfg->E > PPN_MAX_EDGES)
        return ppn::fail(PPN_E_INVALID, "%s: K %d / E %d out of range", who, cfg->K, cfg->E);
    for (int i = 0; i < cfg->K; ++i)
        if (cfg->kp_order[i] < 0 || cfg->kp_order[i] >= cfg->K)
            return ppn::fail(PPN_E_INVALID, "%s: kp_order[%d] = %d is no keypoint", who, i, cfg->kp_order[i]);
    for (int i = 0; i < cfg->E; ++i)
        if (cfg->edge_src[i] < 0 || cfg->edge_src[i] >= cfg->K || cfg->edge_dst[i] < 0 || cfg->edge_dst[i] >= cfg->K)
            return ppn::fail(PPN_E_INVALID, "%s: edge %d joins no two keypoints", who, i);
    if (cfg->grid && cfg->grid_step < 1) return ppn::fail(PPN_E_INVALID, "%s: grid_step %d < 1", who, cfg->grid_step);
    return PPN_OK;
}

}  // namespace

extern "C" size_t ppn_draw_workspace_bytes(const ppn_draw_cfg* cfg, int32_t batch, int32_t max_humans) {
    if (check_cfg(cfg, "ppn_draw_workspace_bytes") != PPN_OK || batch < 1 || max_humans < 1) return 0;
    return (size_t)batch * max_humans * (cfg->K + cfg->E) * 3 * sizeof(int4);
}

extern "C" int ppn_draw_humans(const ppn_draw_cfg* cfg, const uint8_t* src, uint8_t* dst, int32_t batch, int32_t height,
                               int32_t width, const int32_t* count, const int32_t* kp_cell, const float* bbox,
                               int32_t max_humans, void* workspace, void* stream) {
    if (int rc = check_cfg(cfg, "ppn_draw_humans")) return rc;
    if (!src || !dst || !count || !kp_cell || !bbox || !workspace)
        return ppn::fail(PPN_E_INVALID, "ppn_draw_humans: NULL pointer");
    if (batch < 1 || height < 1 || width < 1 || max_humans < 1)
        return ppn::fail(PPN_E_INVALID, "ppn_draw_humans: bad geometry (batch %d, %dx%d, max_humans %d)", batch, height, width,
                         max_humans);
    const int S = cfg->K + cfg->E;
    const long long prims = (long long)batch * max_humans * S;
    if (batch > 65535 || height > 32768 || width > 32768 || (long long)max_humans * S > 0x7fffffffLL / 2 ||
        (prims + THREADS - 1) / THREADS > 0x7fffffffLL)
        return ppn::fail(PPN_E_UNSUPPORTED, "ppn_draw_humans: batch %d, frame %dx%d or %d people x %d slots beyond the limits",
                         batch, height, width, max_humans, S);
    if (reinterpret_cast<uintptr_t>(workspace) % 16)
        return ppn::fail(PPN_E_INVALID, "ppn_draw_humans: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int4* ws = static_cast<int4*>(workspace);
    SetupArgs sa{count, kp_cell, bbox, ws, ws + prims, ws + 2 * prims, batch, max_humans, cfg->K, cfg->E, height, width,
                 cfg->visbbox ? 1 : 0, {}};
    for (int i = 0; i < cfg->E; ++i) { sa.t.edge_src[i] = cfg->edge_src[i]; sa.t.edge_dst[i] = cfg->edge_dst[i]; }
    for (int i = 0; i < cfg->K; ++i) {
        sa.t.kp_order[i] = cfg->kp_order[i];
        sa.t.colour[i] = (unsigned)cfg->palette[i][0] | (unsigned)cfg->palette[i][1] << 8 | (unsigned)cfg->palette[i][2] << 16;
    }
    draw_setup_kernel<<<(unsigned)((prims + THREADS - 1) / THREADS), THREADS, 0, st>>>(sa);
    PPN_LAUNCH_CHECK();
    RasterArgs ra{src, dst, count, sa.bb, sa.par, sa.meta, batch, max_humans, S, height, width, cfg->grid ? 1 : 0,
                  cfg->grid ? cfg->grid_step : 1};
    const bool inplace = src == dst;
    const bool vec = width % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    const int V = inplace || vec ? 4 : 1;
    const dim3 grid((width + 32 * V - 1) / (32 * V), (height + TILE_H - 1) / TILE_H, batch);
    if (inplace) draw_raster_kernel<4, true><<<grid, THREADS, 0, st>>>(ra);
    else if (vec) draw_raster_kernel<4, false><<<grid, THREADS, 0, st>>>(ra);
    else draw_raster_kernel<1, false><<<grid, THREADS, 0, st>>>(ra);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
