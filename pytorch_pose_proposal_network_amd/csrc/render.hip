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
//   draw_raster_yuv_kernel   the same tiles, binning and resolve (the device function paint<V>) on raw NV12, I420 or YUYV
//                        surfaces: luma per pixel, chroma per 2 x 2 group (per row pair in YUYV) from the group's first painted
//                        pixel, exchanged between the two rows' lanes of a wave (ppn_draw_humans_yuv, further down).
//   draw_scene_setup_kernel   (ppn_draw_scene) the people's records plus one thread per slot of the overlay's list -- zones,
//                        counting lines, id labels: lines, filled boxes and glyph runs, rules in include/ppn.h -- which the
//                        OV instantiations of the raster kernels bin behind the people's list, before the grid.
// All f32 arithmetic (midpoints, the scan line's x = (y - y0) * slope + x0, the slope's division) is written out in a fixed
// order and the file is built with -ffp-contract=off and IEEE division.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int TILE_H = 8;        // rows of a tile; 32 threads (V pixels each) per row
constexpr int CAP = 256;         // LDS bin list entries (48 bytes each); a fuller list is drawn in chunks
enum { PRIM_NONE = 0, PRIM_ROOT = 1, PRIM_RECT = 2, PRIM_DISC = 3, PRIM_LINE = 4, PRIM_FILL = 5, PRIM_TEXT = 6 };

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

// the record of PIL's width-2 line between integer end points: parameters, type and quad offsets, unclipped coverage box
__device__ __forceinline__ void line_record(int x0, int y0, int x1, int y1, int4& par, int4& meta, int& cx0, int& cy0, int& cx1,
                                            int& cy1) {
    par = make_int4(x0, y0, x1, y1);
    if (x0 == x1 && y0 == y1) {
        meta.x = PRIM_RECT;                                       // a zero vector is one pixel
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
            line_record(x0, y0, x1, y1, par, meta, cx0, cy0, cx1, cy1);
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

// ---- the overlay (ppn_draw_scene): zones, counting lines and id labels as a second primitive list per image ------------
// Slot layout per image, the slot index being the paint order: zone z at 10 z (8 edges, plate, text), line l at 160 + 4 l
// (segment, tick, plate, text), person p at 224 + 3 p (root outline, plate, text).
constexpr int OV_ZONE_SLOTS = 10, OV_LINE_SLOTS = 4, OV_PERSON_SLOTS = 3;
constexpr int OV_FIXED = PPN_ZONE_MAX * OV_ZONE_SLOTS + PPN_LINE_MAX * OV_LINE_SLOTS;      // 224
enum { OV_ZONE = 0, OV_LINE = 16, OV_ID = 32, OV_ACTIVE = 48, OV_ALERT = 49, OV_TEXT = 50, OV_PLATE = 51, OV_COLOURS = 52 };
enum { GLYPH_COLON = 10 };

struct OverlayArgs {
    const int* ids;              // [B][M] or NULL: no id part
    const int* zone_n;           // NULL: no zone part (then none of the seven below is read)
    const int* zone_nv;
    const float* zone_xy;
    const int* line_n;
    const float* line_xy;
    const int* out_zone;         // [B][16][4]
    const int* out_line;         // [B][16][2]
    const int* line_total;       // [S][16][2]
    const int* n_frames;         // [S] or NULL
    int4* bb;                    // workspace behind the people's: [B][NOV] boxes, parameters, type / colour / glyph codes
    int4* par;
    int4* meta;
    int frames, scale, plates;
    float tick;
    unsigned colour[OV_COLOURS];
};

__device__ __forceinline__ bool in_range(float v) { return fabsf(v) < 1048576.f; }

// the decimal digits of v (no leading zeros) appended to the 4-bit glyph codes `codes`, n glyphs so far
__device__ __forceinline__ void put_number(unsigned v, unsigned long long& codes, int& n) {
    unsigned div = 1000000000u;
    while (div > 1 && v / div == 0) div /= 10;
    for (; div; div /= 10) {
        codes |= (unsigned long long)(v / div % 10) << (4 * n);
        ++n;
    }
}

__device__ __forceinline__ unsigned shown_count(int v) { return (unsigned)min(max(v, 0), 999999); }

// the overlay record of slot i of image b
__device__ __forceinline__ void build_overlay(const SetupArgs& a, const OverlayArgs& o, long long g) {
    const int NOV = OV_FIXED + OV_PERSON_SLOTS * a.M;
    if (g >= (long long)NOV * a.B) return;
    const int b = (int)(g / NOV), i = (int)(g % NOV);
    const int s = b / o.frames, t = b % o.frames, sc = o.scale;
    int4 par = make_int4(0, 0, 0, 0), meta = make_int4(PRIM_NONE, 0, 0, 0);
    int cx0 = 0, cy0 = 0, cx1 = -1, cy1 = -1;
    // a label: the text at (tx, ty) when `text`, its plate otherwise
    unsigned long long codes = 0;
    int n = 0, tx = 0, ty = 0, part = -1;                         // part: 0 plate, 1 text of a label that is drawn
    const bool processed = !o.n_frames || t < o.n_frames[s];

    if (!processed) {
    } else if (i < OV_FIXED) {
        if (o.zone_n) {
            if (i < PPN_ZONE_MAX * OV_ZONE_SLOTS) {
                const int z = i / OV_ZONE_SLOTS, k = i % OV_ZONE_SLOTS;
                const int nv = min(max(o.zone_nv[s * PPN_ZONE_MAX + z], 0), PPN_ZONE_MAX_VERT);
                const float* xy = o.zone_xy + ((size_t)s * PPN_ZONE_MAX + z) * PPN_ZONE_MAX_VERT * 2;
                bool ok = z < min(max(o.zone_n[s], 0), PPN_ZONE_MAX) && nv >= 3;
                for (int v = 0; v < nv; ++v) ok = ok && in_range(xy[2 * v]) && in_range(xy[2 * v + 1]);
                if (ok) {
                    const int* oz = o.out_zone + ((size_t)b * PPN_ZONE_MAX + z) * 4;
                    if (k < PPN_ZONE_MAX_VERT) {
                        if (k < nv) {
                            const int k1 = k + 1 == nv ? 0 : k + 1;
                            meta.y = (int)(oz[3] > 0 ? o.colour[OV_ALERT] : oz[0] > 0 ? o.colour[OV_ACTIVE] : o.colour[OV_ZONE + z]);
                            line_record((int)xy[2 * k], (int)xy[2 * k + 1], (int)xy[2 * k1], (int)xy[2 * k1 + 1], par, meta, cx0,
                                        cy0, cx1, cy1);
                        }
                    } else {
                        part = k - PPN_ZONE_MAX_VERT;
                        tx = (int)xy[0] + 3; ty = (int)xy[1] + 3;
                        put_number(shown_count(oz[0]), codes, n);
                    }
                }
            } else {
                const int l = (i - PPN_ZONE_MAX * OV_ZONE_SLOTS) / OV_LINE_SLOTS, k = (i - PPN_ZONE_MAX * OV_ZONE_SLOTS) % OV_LINE_SLOTS;
                const float* xy = o.line_xy + ((size_t)s * PPN_LINE_MAX + l) * 4;
                const float ax = xy[0], ay = xy[1], bx = xy[2], by = xy[3];
                if (l < min(max(o.line_n[s], 0), PPN_LINE_MAX) && in_range(ax) && in_range(ay) && in_range(bx) && in_range(by)) {
                    const int* ol = o.out_line + ((size_t)b * PPN_LINE_MAX + l) * 2;
                    const float mx = (ax + bx) / 2.f, my = (ay + by) / 2.f;
                    meta.y = (int)((int)((unsigned)ol[0] + (unsigned)ol[1]) > 0 ? o.colour[OV_ACTIVE] : o.colour[OV_LINE + l]);
                    if (k == 0) {
                        line_record((int)ax, (int)ay, (int)bx, (int)by, par, meta, cx0, cy0, cx1, cy1);
                    } else if (k == 1) {
                        const float dx = bx - ax, dy = by - ay;
                        const float len = sqrtf(dx * dx + dy * dy);
                        if (len != 0.f) {
                            const float q = o.tick / len;
                            const float ex = mx + (-dy) * q, ey = my + dx * q;
                            if (in_range(ex) && in_range(ey)) line_record((int)mx, (int)my, (int)ex, (int)ey, par, meta, cx0, cy0, cx1, cy1);
                        }
                    } else {
                        part = k - 2;
                        tx = (int)mx + 3; ty = (int)my + 3;
                        unsigned tot[2];                          // the totals as of this frame: the later frames' crossings taken off
                        for (int d = 0; d < 2; ++d) {
                            tot[d] = (unsigned)o.line_total[((size_t)s * PPN_LINE_MAX + l) * 2 + d];
                            for (int t2 = t + 1; t2 < o.frames; ++t2)
                                tot[d] -= (unsigned)o.out_line[((size_t)(s * o.frames + t2) * PPN_LINE_MAX + l) * 2 + d];
                        }
                        put_number(shown_count((int)tot[0]), codes, n);
                        codes |= (unsigned long long)GLYPH_COLON << (4 * n);
                        ++n;
                        put_number(shown_count((int)tot[1]), codes, n);
                    }
                }
            }
        }
    } else if (o.ids) {
        const int p = (i - OV_FIXED) / OV_PERSON_SLOTS, k = (i - OV_FIXED) % OV_PERSON_SLOTS;
        float box[4];
        if (p < min(max(a.count[b], 0), a.M)) {
            const int id = o.ids[(size_t)b * a.M + p];
            if (id > 0 && usable(a, (size_t)b * a.M + p, 0, box)) {
                const int x0 = (int)box[1], y0 = (int)box[0];
                if (k == 0) {
                    par = make_int4(x0, y0, (int)box[3], (int)box[2]);
                    meta.y = (int)o.colour[OV_ID + (id & 15)];
                    if (par.z >= par.x && par.w >= par.y) {
                        meta.x = PRIM_ROOT;
                        cx0 = par.x; cy0 = par.y; cx1 = par.z; cy1 = par.w;
                    }
                } else {
                    part = k - 1;
                    tx = x0; ty = y0 - 7 * sc - 1;
                    if (ty - 1 < 0) ty = y0 + 3;                  // no room above the box: inside it
                    put_number((unsigned)id, codes, n);
                }
            }
        }
    }
    if (part == 1) {
        meta = make_int4(PRIM_TEXT, (int)o.colour[OV_TEXT], (int)(unsigned)codes, (int)(unsigned)(codes >> 32));
        par = make_int4(tx, ty, sc, n);
        cx0 = tx; cy0 = ty; cx1 = tx + 6 * sc * n - sc - 1; cy1 = ty + 7 * sc - 1;
    } else if (part == 0 && o.plates) {
        meta = make_int4(PRIM_FILL, (int)o.colour[OV_PLATE], 0, 0);
        par = make_int4(tx - 1, ty - 1, tx + 6 * sc * n - sc, ty + 7 * sc);
        cx0 = par.x; cy0 = par.y; cx1 = par.z; cy1 = par.w;
    }
    cx0 = max(cx0, 0); cy0 = max(cy0, 0); cx1 = min(cx1, a.W - 1); cy1 = min(cy1, a.H - 1);
    if (cx0 > cx1 || cy0 > cy1) { cx0 = cy0 = 0x7fffffff; cx1 = cy1 = -1; meta.x = PRIM_NONE; }
    o.bb[g] = make_int4(cx0, cy0, cx1, cy1);
    o.par[g] = par;
    o.meta[g] = meta;
}

// the people's records, then the overlay's: still one setup launch
__global__ void __launch_bounds__(THREADS) draw_scene_setup_kernel(SetupArgs a, OverlayArgs o, long long prims) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (g < prims) build_primitive(a, g);
    else build_overlay(a, o, g - prims);
}

// The project's 5 x 7 font (include/ppn.h): seven row bytes per glyph, bit 4 the leftmost column.
__constant__ unsigned char FONT[16][8] = {
    {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},
    {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
    {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},
    {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}, {0x00, 0x04, 0x04, 0x00, 0x04, 0x04, 0x00}, {0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00},
    {0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A}, {0}, {0}, {0},
};

// the glyph coverage rule of PRIM_TEXT, integers only
template <int V>
__device__ __forceinline__ unsigned text_cover(int4 p, int4 m, int px, int py) {
    const int s = p.z, v = py - p.y;
    if (v < 0 || v >= 7 * s) return 0;
    const int row = v / s;
    unsigned mask = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int u = px + j - p.x;
        if (u < 0) continue;
        const int c = u / (6 * s), col = u % (6 * s) / s;
        if (c >= p.w || col >= 5) continue;
        const unsigned code = (unsigned)(c < 8 ? m.z : m.w) >> (4 * (c & 7)) & 15u;
        mask |= (FONT[code][row] >> (4 - col) & 1u) << j;
    }
    return mask;
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

// OV: the overlay's primitive kinds exist (the people-only kernels are compiled without them)
template <int V, bool OV>
__device__ __forceinline__ unsigned cover(int4 p, int4 m, int px, int py, int H) {
    if constexpr (OV) {
        if (m.x == PRIM_FILL) return py >= p.y && py <= p.w ? span_mask<V>(p.x, p.z, px) : 0;
        if (m.x == PRIM_TEXT) return text_cover<V>(p, m, px, py);
    }
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

// what the setup pass left for the raster pass, the frame's size and the grid
struct PaintArgs {
    const int* count;
    const int4* bb;
    const int4* par;
    const int4* meta;
    int B, M, S, H, W, grid, grid_step;
    unsigned grid_colour;        // packed like a primitive's colour
    const int4* ov_bb;           // the overlay's list, binned after the people's (read by the OV kernels only)
    const int4* ov_par;
    const int4* ov_meta;
    int ov_fixed, ov_person;     // slots per image before the people's, and per person
};

constexpr unsigned GRID_RGB = 110u | 110u << 8 | 110u << 16;

// What the people of image b and the grid paint on the pixels (px .. px + V - 1, py) of the tile at (tx0, ty0): bit j of
// `hit` and col[j] (the primitive's packed colour) for the pixels of `inside`.  Every thread of the workgroup calls it:
// there are barriers inside.  OV: the overlay's list follows the people's.
template <int V, bool OV>
__device__ __forceinline__ void paint(const PaintArgs& a, int b, int tx0, int ty0, int px, int py, unsigned inside,
                                      unsigned& hit, unsigned (&col)[V]) {
    __shared__ int4 s_bb[CAP], s_par[CAP], s_meta[CAP];
    __shared__ int s_wave[THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx1 = min(tx0 + 32 * V, a.W) - 1, ty1 = min(ty0 + TILE_H, a.H) - 1;
    hit = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) col[j] = 0;

    // the last primitive of the list's first `cnt` entries that covers each pixel
    auto resolve = [&](int cnt) {
        unsigned todo = inside;
        for (int i = cnt - 1; i >= 0 && todo; --i) {
            const int4 bb = s_bb[i];
            if (py < bb.y || py > bb.w || px + V - 1 < bb.x || px > bb.z) continue;
            const int4 m = s_meta[i];
            const unsigned c = cover<V, OV>(s_par[i], m, px, py, a.H) & todo;
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (c >> j & 1) col[j] = (unsigned)m.y;
            hit |= c;
            todo &= ~c;
        }
    };

    const int people = min(max(a.count[b], 0), a.M);
    const int n_people = people * a.S, n = n_people + (OV ? a.ov_fixed + a.ov_person * people : 0);
    const size_t base = (size_t)b * a.M * a.S, ov_base = OV ? (size_t)b * (a.ov_fixed + a.ov_person * a.M) : 0;
    int cnt = 0;
    // one list in paint order: the people's primitives, then the overlay's; a block of THREADS may span the seam
    for (int i0 = 0; i0 < n; i0 += THREADS) {
        const int i = i0 + t;
        bool ov = false;
        int4 bb = make_int4(0, 0, -1, -1);
        const bool second = OV && i >= n_people;
        const size_t at_g = second ? ov_base + (i - n_people) : base + i;
        if (i < n) {
            bb = (second ? a.ov_bb : a.bb)[at_g];
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
            s_par[at] = (second ? a.ov_par : a.par)[at_g];
            s_meta[at] = (second ? a.ov_meta : a.meta)[at_g];
        }
        cnt += total;
        __syncthreads();
    }
    resolve(cnt);

    if (a.grid) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if ((inside >> j & 1) && ((px + j) % a.grid_step == 0 || py % a.grid_step == 0)) {
                col[j] = a.grid_colour;
                hit |= 1u << j;
            }
        }
    }
}

struct RasterArgs {
    const unsigned char* src;    // [B][H][W][3]
    unsigned char* dst;
    PaintArgs p;
};

template <int V, bool INPLACE, bool OV>
__global__ void __launch_bounds__(THREADS) draw_raster_kernel(RasterArgs ra) {
    const PaintArgs& a = ra.p;
    const int t = threadIdx.x;
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * 32 * V, ty0 = blockIdx.y * TILE_H;
    const int px = tx0 + (t & 31) * V, py = ty0 + (t >> 5);
    unsigned inside = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) inside |= (px + j < a.W && py < a.H) ? 1u << j : 0u;
    unsigned hit;
    unsigned col[V];
    paint<V, OV>(a, b, tx0, ty0, px, py, inside, hit, col);

    const size_t o = (((size_t)b * a.H + py) * a.W + px) * 3;
    if constexpr (INPLACE) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (hit >> j & 1) {
                ra.dst[o + 3 * j] = (unsigned char)col[j];
                ra.dst[o + 3 * j + 1] = (unsigned char)(col[j] >> 8);
                ra.dst[o + 3 * j + 2] = (unsigned char)(col[j] >> 16);
            }
        }
    } else if constexpr (V == 4) {
        if (inside) {                                             // W % 4 == 0: the four pixels are in the frame together
            const unsigned* s4 = reinterpret_cast<const unsigned*>(ra.src + o);
            unsigned q[3] = {s4[0], s4[1], s4[2]};
#pragma unroll
            for (int n8 = 0; n8 < 12; ++n8) {                     // byte n8 of the twelve: channel n8 % 3 of pixel n8 / 3
                if (hit >> (n8 / 3) & 1) {
                    const unsigned v = col[n8 / 3] >> (8 * (n8 % 3)) & 0xffu;
                    q[n8 / 4] = (q[n8 / 4] & ~(0xffu << (8 * (n8 % 4)))) | v << (8 * (n8 % 4));
                }
            }
            unsigned* d4 = reinterpret_cast<unsigned*>(ra.dst + o);
            d4[0] = q[0]; d4[1] = q[1]; d4[2] = q[2];
        }
    } else {
        if (inside) {
            const bool h = hit & 1;
            ra.dst[o] = h ? (unsigned char)col[0] : ra.src[o];
            ra.dst[o + 1] = h ? (unsigned char)(col[0] >> 8) : ra.src[o + 1];
            ra.dst[o + 2] = h ? (unsigned char)(col[0] >> 16) : ra.src[o + 2];
        }
    }
}

// ---- raw video surfaces (ppn_draw_humans_yuv) ------------------------------------------------------------------------
// The same (hit, colour) pairs, the colours converted to Y | U << 8 | V << 16 on the host, stored into NV12, I420 or YUYV
// planes.  A luma sample takes its own pixel's colour; a chroma sample the colour of the first painted pixel of its group
// in row-major order.  A thread's four pixels are two column pairs; in NV12 / I420 the two rows of a 2 x 2 group are lanes
// l and l ^ 32 of one wave (a tile starts on an even row), so one exchange of each pair's pick settles the group and the
// even row's thread stores the sample.  MODE: in place (painted samples only, bytes), out of place as bytes, out of place
// as dwords (halfwords for I420's chroma) when the host found every plane, pitch and stride of both surfaces aligned.
enum { YUV_INPLACE = 0, YUV_BYTES = 1, YUV_WORDS = 2 };

struct YuvPlanes {
    unsigned char* y;
    unsigned char* u;
    unsigned char* v;
    long long frame_stride;
    int pitch, pitch_c;
};

struct YuvRasterArgs {
    YuvPlanes src, dst;
    PaintArgs p;
};

// N bytes at d: val[i] where bit i of `painted` is set, the source byte otherwise; only bytes of `valid` exist
template <int N, int MODE>
__device__ __forceinline__ void store_samples(unsigned char* d, const unsigned char* s, const unsigned (&val)[N],
                                              unsigned painted, unsigned valid) {
    if constexpr (MODE == YUV_INPLACE) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (painted >> i & 1) d[i] = (unsigned char)val[i];
    } else if constexpr (MODE == YUV_BYTES) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (valid >> i & 1) d[i] = (painted >> i & 1) ? (unsigned char)val[i] : s[i];
    } else if (valid) {                                           // width % 4 == 0: all N bytes are in the frame together
        using word = std::conditional_t<N == 2, unsigned short, unsigned>;
        constexpr int B = (int)sizeof(word);
#pragma unroll
        for (int w = 0; w < N / B; ++w) {
            unsigned q = reinterpret_cast<const word*>(s)[w];
#pragma unroll
            for (int i = 0; i < B; ++i)
                if (painted >> (w * B + i) & 1) q = (q & ~(0xffu << (8 * i))) | (val[w * B + i] & 0xffu) << (8 * i);
            reinterpret_cast<word*>(d)[w] = (word)q;
        }
    }
}

template <int FMT, int MODE, bool OV>
__global__ void __launch_bounds__(THREADS) draw_raster_yuv_kernel(YuvRasterArgs ya) {
    constexpr int V = 4;
    const PaintArgs& a = ya.p;
    const int t = threadIdx.x;
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * 32 * V, ty0 = blockIdx.y * TILE_H;
    const int px = tx0 + (t & 31) * V, py = ty0 + (t >> 5);
    unsigned inside = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) inside |= (px + j < a.W && py < a.H) ? 1u << j : 0u;
    unsigned hit;
    unsigned col[V];
    paint<V, OV>(a, b, tx0, ty0, px, py, inside, hit, col);

    // per column pair g: bit 24 set and the colour of the first painted pixel of this row's pair, or 0
    unsigned pick[2];
#pragma unroll
    for (int g = 0; g < 2; ++g)
        pick[g] = (hit >> (2 * g) & 1) ? col[2 * g] | 1u << 24 : (hit >> (2 * g + 1) & 1) ? col[2 * g + 1] | 1u << 24 : 0u;
    const unsigned pairs = (inside & 1) | (inside >> 1 & 2);      // bit g: pair g is in the frame (the width is even)
    const long long so = (long long)b * ya.src.frame_stride, dof = (long long)b * ya.dst.frame_stride;

    if constexpr (FMT == PPN_PIX_YUYV) {
        unsigned val[8], painted = 0, valid = 0;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            val[4 * g] = col[2 * g] & 0xffu;
            val[4 * g + 1] = pick[g] >> 8 & 0xffu;
            val[4 * g + 2] = col[2 * g + 1] & 0xffu;
            val[4 * g + 3] = pick[g] >> 16 & 0xffu;
            painted |= ((hit >> (2 * g) & 1) | (pick[g] >> 24) << 1 | (hit >> (2 * g + 1) & 1) << 2 | (pick[g] >> 24) << 3) << (4 * g);
            valid |= (pairs >> g & 1) ? 0xfu << (4 * g) : 0u;
        }
        const long long row = 2ll * px;
        store_samples<8, MODE>(ya.dst.y + dof + (long long)py * ya.dst.pitch + row,
                               ya.src.y + so + (long long)py * ya.src.pitch + row, val, painted, valid);
    } else {
        unsigned val[4];
#pragma unroll
        for (int j = 0; j < V; ++j) val[j] = col[j] & 0xffu;
        store_samples<4, MODE>(ya.dst.y + dof + (long long)py * ya.dst.pitch + px,
                               ya.src.y + so + (long long)py * ya.src.pitch + px, val, hit, inside);
        unsigned below[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) below[g] = (unsigned)__shfl_xor((int)pick[g], 32);
        if ((t & 32) == 0) {                                      // the even row of the pair stores the group's sample
            unsigned c[2], any = 0;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                c[g] = pick[g] >> 24 ? pick[g] : below[g];
                any |= (c[g] >> 24) << g;
            }
            const long long crow = py >> 1;
            if constexpr (FMT == PPN_PIX_NV12) {
                const unsigned uv[4] = {c[0] >> 8 & 0xffu, c[0] >> 16 & 0xffu, c[1] >> 8 & 0xffu, c[1] >> 16 & 0xffu};
                const unsigned painted = (any & 1 ? 3u : 0u) | (any & 2 ? 12u : 0u);
                const unsigned valid = (pairs & 1 ? 3u : 0u) | (pairs & 2 ? 12u : 0u);
                store_samples<4, MODE>(ya.dst.u + dof + crow * ya.dst.pitch_c + px, ya.src.u + so + crow * ya.src.pitch_c + px,
                                       uv, painted, valid);
            } else {
                const unsigned us[2] = {c[0] >> 8 & 0xffu, c[1] >> 8 & 0xffu}, vs[2] = {c[0] >> 16 & 0xffu, c[1] >> 16 & 0xffu};
                const long long od = dof + crow * ya.dst.pitch_c + (px >> 1), os = so + crow * ya.src.pitch_c + (px >> 1);
                store_samples<2, MODE>(ya.dst.u + od, ya.src.u + os, us, any, pairs);
                store_samples<2, MODE>(ya.dst.v + od, ya.src.v + os, vs, any, pairs);
            }
        }
    }
}

// the forward colour rule's sets (include/ppn.h), index (full_range ? 2 : 0) + matrix: CYR CYG CYB, CUR CUG CUB, CVR CVG CVB, yoff
const int32_t kRgbToYuv[4][10] = {
    {269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897, 16},
    {191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230, 16},
    {313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262, 0},
    {222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074, 0},
};

inline int sat8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// Y | U << 8 | V << 16 of one colour
unsigned rgb_to_yuv(const int32_t* k, int r, int g, int b) {
    const int h = 1 << 19;
    const int y = sat8((k[0] * r + k[1] * g + k[2] * b + h + (k[9] << 20)) >> 20);
    const int u = sat8((k[3] * r + k[4] * g + k[5] * b + h + (128 << 20)) >> 20);
    const int v = sat8((k[6] * r + k[7] * g + k[8] * b + h + (128 << 20)) >> 20);
    return (unsigned)y | (unsigned)u << 8 | (unsigned)v << 16;
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


// what both entries refuse of the people and the workspace; `who` names the entry in the message
int check_call(const char* who, const ppn_draw_cfg* cfg, bool null_pointer, int batch, int height, int width, int max_humans,
               const void* workspace) {
    if (int rc = check_cfg(cfg, who)) return rc;
    if (null_pointer) return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", who);
    if (batch < 1 || height < 1 || width < 1 || max_humans < 1)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry (batch %d, %dx%d, max_humans %d)", who, batch, height, width,
                         max_humans);
    const int S = cfg->K + cfg->E;
    const long long prims = (long long)batch * max_humans * S;
    if (batch > 65535 || height > 32768 || width > 32768 || (long long)max_humans * S > 0x7fffffffLL / 2 ||
        (prims + THREADS - 1) / THREADS > 0x7fffffffLL)
        return ppn::fail(PPN_E_UNSUPPORTED, "%s: batch %d, frame %dx%d or %d people x %d slots beyond the limits", who, batch,
                         height, width, max_humans, S);
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return ppn::fail(PPN_E_INVALID, "%s: workspace must be 16-byte aligned", who);
    return PPN_OK;
}

// The setup launch with the palette as packed colours (RGB, or YUV for a raw surface); *p: what the raster pass needs.
int launch_setup(const ppn_draw_cfg* cfg, const unsigned* colour, unsigned grid_colour, const int32_t* count,
                 const int32_t* kp_cell, const float* bbox, int batch, int height, int width, int max_humans, void* workspace,
                 hipStream_t st, PaintArgs* p, OverlayArgs* ov = nullptr) {
    const int S = cfg->K + cfg->E;
    const long long prims = (long long)batch * max_humans * S;
    int4* ws = static_cast<int4*>(workspace);
    SetupArgs sa{count, kp_cell, bbox, ws, ws + prims, ws + 2 * prims, batch, max_humans, cfg->K, cfg->E, height, width,
                 cfg->visbbox ? 1 : 0, {}};
    for (int i = 0; i < cfg->E; ++i) { sa.t.edge_src[i] = cfg->edge_src[i]; sa.t.edge_dst[i] = cfg->edge_dst[i]; }
    for (int i = 0; i < cfg->K; ++i) {
        sa.t.kp_order[i] = cfg->kp_order[i];
        sa.t.colour[i] = colour[i];
    }
    *p = PaintArgs{count, sa.bb, sa.par, sa.meta, batch, max_humans, S, height, width, cfg->grid ? 1 : 0,
                   cfg->grid ? cfg->grid_step : 1, grid_colour, nullptr, nullptr, nullptr, 0, 0};
    if (ov) {                                                     // the overlay's records lie behind the people's
        const long long slots = (long long)batch * (OV_FIXED + OV_PERSON_SLOTS * (long long)max_humans);
        if ((prims + slots + THREADS - 1) / THREADS > 0x7fffffffLL)
            return ppn::fail(PPN_E_UNSUPPORTED, "ppn_draw_scene: %lld primitives beyond the limits", prims + slots);
        ov->bb = ws + 3 * prims;
        ov->par = ov->bb + slots;
        ov->meta = ov->par + slots;
        draw_scene_setup_kernel<<<(unsigned)((prims + slots + THREADS - 1) / THREADS), THREADS, 0, st>>>(sa, *ov, prims);
        p->ov_bb = ov->bb; p->ov_par = ov->par; p->ov_meta = ov->meta;
        p->ov_fixed = OV_FIXED; p->ov_person = OV_PERSON_SLOTS;
    } else {
        draw_setup_kernel<<<(unsigned)((prims + THREADS - 1) / THREADS), THREADS, 0, st>>>(sa);
    }
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

// what ppn_draw_humans_yuv refuses of one surface
int check_surface(const char* who, const char* name, const ppn_yuv_surface* s) {
    if (!s) return ppn::fail(PPN_E_INVALID, "%s: NULL %s surface", who, name);
    const int fmt = s->format;
    if (fmt != PPN_PIX_NV12 && fmt != PPN_PIX_I420 && fmt != PPN_PIX_YUYV)
        return ppn::fail(PPN_E_INVALID, "%s: %s: unknown format %d", who, name, fmt);
    if (s->matrix != 0 && s->matrix != 1) return ppn::fail(PPN_E_INVALID, "%s: %s: unknown matrix %d", who, name, s->matrix);
    const bool is420 = fmt != PPN_PIX_YUYV;
    if (!s->y || (is420 && !s->u) || (fmt == PPN_PIX_I420 && !s->v)) return ppn::fail(PPN_E_INVALID, "%s: %s: NULL plane", who, name);
    if (s->height < 1 || s->width < 1) return ppn::fail(PPN_E_INVALID, "%s: %s: bad size %dx%d", who, name, s->height, s->width);
    if ((s->width & 1) || (is420 && (s->height & 1)))
        return ppn::fail(PPN_E_INVALID, "%s: %s: odd size %dx%d", who, name, s->height, s->width);
    const int64_t row = is420 ? s->width : 2 * (int64_t)s->width;
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

// every plane, pitch and stride of the surface allows the word stores of YUV_WORDS
bool word_aligned(const ppn_yuv_surface* s) {
    auto off = [](const void* p, int64_t a, int64_t b, uintptr_t n) {
        return reinterpret_cast<uintptr_t>(p) % n || a % (int64_t)n || b % (int64_t)n;
    };
    if (s->width % 4 || off(s->y, s->pitch, s->frame_stride, 4)) return false;
    if (s->format == PPN_PIX_NV12) return !off(s->u, s->pitch_c, s->frame_stride, 4);
    if (s->format == PPN_PIX_I420) return !off(s->u, s->pitch_c, s->frame_stride, 2) && !off(s->v, s->pitch_c, s->frame_stride, 2);
    return true;
}

YuvPlanes planes_of(const ppn_yuv_surface* s) {
    const bool is420 = s->format != PPN_PIX_YUYV;
    return {static_cast<unsigned char*>(s->y), is420 ? static_cast<unsigned char*>(s->u) : nullptr,
            s->format == PPN_PIX_I420 ? static_cast<unsigned char*>(s->v) : nullptr, s->frame_stride, s->pitch,
            is420 ? s->pitch_c : 0};
}

template <int FMT, bool OV>
void launch_yuv(int mode, dim3 grid, hipStream_t st, const YuvRasterArgs& ya) {
    if (mode == YUV_INPLACE) draw_raster_yuv_kernel<FMT, YUV_INPLACE, OV><<<grid, THREADS, 0, st>>>(ya);
    else if (mode == YUV_WORDS) draw_raster_yuv_kernel<FMT, YUV_WORDS, OV><<<grid, THREADS, 0, st>>>(ya);
    else draw_raster_yuv_kernel<FMT, YUV_BYTES, OV><<<grid, THREADS, 0, st>>>(ya);
}

template <bool OV>
void launch_yuv_format(int format, int mode, dim3 grid, hipStream_t st, const YuvRasterArgs& ya) {
    if (format == PPN_PIX_NV12) launch_yuv<PPN_PIX_NV12, OV>(mode, grid, st, ya);
    else if (format == PPN_PIX_I420) launch_yuv<PPN_PIX_I420, OV>(mode, grid, st, ya);
    else launch_yuv<PPN_PIX_YUYV, OV>(mode, grid, st, ya);
}

template <bool OV>
void launch_rgb(bool inplace, bool vec, dim3 grid, hipStream_t st, const RasterArgs& ra) {
    if (inplace) draw_raster_kernel<4, true, OV><<<grid, THREADS, 0, st>>>(ra);
    else if (vec) draw_raster_kernel<4, false, OV><<<grid, THREADS, 0, st>>>(ra);
    else draw_raster_kernel<1, false, OV><<<grid, THREADS, 0, st>>>(ra);
}

// What ppn_draw_scene refuses of the overlay; on success *o holds everything but the workspace pointers, the colours
// packed as RGB, and *parts says whether there is anything to draw (a zone part or an id part).
int check_overlay(const char* who, const ppn_overlay_cfg* oc, const ppn_overlay_in* in, int batch, int max_humans, OverlayArgs* o,
                  bool* parts) {
    if (!oc || !in) return ppn::fail(PPN_E_INVALID, "%s: NULL overlay cfg or inputs", who);
    if (oc->scale < 1 || oc->scale > 4) return ppn::fail(PPN_E_INVALID, "%s: scale %d outside 1..4", who, oc->scale);
    if (oc->frames < 1) return ppn::fail(PPN_E_INVALID, "%s: frames %d < 1", who, oc->frames);
    if (batch >= 1 && batch % oc->frames) return ppn::fail(PPN_E_INVALID, "%s: batch %d is no multiple of frames %d", who, batch, oc->frames);
    if (!(oc->tick >= 0.f) || !(oc->tick <= 3.4028234663852886e38f))
        return ppn::fail(PPN_E_INVALID, "%s: tick must be finite and not negative", who);
    const void* zone[8] = {in->geom.zone_n, in->geom.zone_nv, in->geom.zone_xy, in->geom.line_n, in->geom.line_xy, in->out_zone,
                           in->out_line, in->line_total};
    int given = 0;
    for (const void* q : zone) given += q != nullptr;
    if (given != 0 && given != 8)
        return ppn::fail(PPN_E_INVALID, "%s: NULL pointer in the zone part (all eight of its pointers, or none)", who);
    if (max_humans >= 1 && batch >= 1 && (OV_FIXED + OV_PERSON_SLOTS * (long long)max_humans) * batch > 0x7fffffffLL)
        return ppn::fail(PPN_E_UNSUPPORTED, "%s: batch %d x %d people beyond the limits", who, batch, max_humans);
    *o = OverlayArgs{in->ids, in->geom.zone_n, in->geom.zone_nv, in->geom.zone_xy, in->geom.line_n, in->geom.line_xy, in->out_zone,
                     in->out_line, in->line_total, in->n_frames, nullptr, nullptr, nullptr, oc->frames, oc->scale,
                     oc->plates ? 1 : 0, oc->tick, {}};
    auto pack = [](const uint8_t* c) { return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16; };
    for (int i = 0; i < 16; ++i) {
        o->colour[OV_ZONE + i] = pack(oc->zone_colour[i]);
        o->colour[OV_LINE + i] = pack(oc->line_colour[i]);
        o->colour[OV_ID + i] = pack(oc->id_colour[i]);
    }
    o->colour[OV_ACTIVE] = pack(oc->active);
    o->colour[OV_ALERT] = pack(oc->alert);
    o->colour[OV_TEXT] = pack(oc->text);
    o->colour[OV_PLATE] = pack(oc->plate);
    *parts = given == 8 || in->ids;
    return PPN_OK;
}

// ppn_draw_humans, with the overlay's list when ov is given
int draw_rgb(const char* who, const ppn_draw_cfg* cfg, OverlayArgs* ov, const uint8_t* src, uint8_t* dst, int32_t batch,
             int32_t height, int32_t width, const int32_t* count, const int32_t* kp_cell, const float* bbox, int32_t max_humans,
             void* workspace, void* stream) {
    if (int rc = check_call(who, cfg, !src || !dst || !count || !kp_cell || !bbox || !workspace, batch, height, width, max_humans,
                            workspace))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned colour[PPN_MAX_KP];
    for (int i = 0; i < cfg->K; ++i)
        colour[i] = (unsigned)cfg->palette[i][0] | (unsigned)cfg->palette[i][1] << 8 | (unsigned)cfg->palette[i][2] << 16;
    RasterArgs ra{src, dst, {}};
    if (int rc = launch_setup(cfg, colour, GRID_RGB, count, kp_cell, bbox, batch, height, width, max_humans, workspace, st, &ra.p,
                              ov))
        return rc;
    const bool inplace = src == dst;
    const bool vec = width % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    const int V = inplace || vec ? 4 : 1;
    const dim3 grid((width + 32 * V - 1) / (32 * V), (height + TILE_H - 1) / TILE_H, batch);
    if (ov) launch_rgb<true>(inplace, vec, grid, st, ra);
    else launch_rgb<false>(inplace, vec, grid, st, ra);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

// ppn_draw_humans_yuv, with the overlay's list (its colours converted like the palette's) when ov is given
int draw_yuv(const char* who, const ppn_draw_cfg* cfg, OverlayArgs* ov, const ppn_yuv_surface* src, const ppn_yuv_surface* dst,
             int32_t batch, const int32_t* count, const int32_t* kp_cell, const float* bbox, int32_t max_humans, void* workspace,
             void* stream) {
    if (int rc = check_surface(who, "src", src)) return rc;
    if (int rc = check_surface(who, "dst", dst)) return rc;
    if (src->format != dst->format || src->height != dst->height || src->width != dst->width || src->matrix != dst->matrix ||
        !src->full_range != !dst->full_range)
        return ppn::fail(PPN_E_INVALID, "%s: src and dst differ in format, size, matrix or range", who);
    const YuvPlanes ps = planes_of(src), pd = planes_of(dst);
    const bool all = ps.y == pd.y && ps.u == pd.u && ps.v == pd.v && ps.pitch == pd.pitch && ps.pitch_c == pd.pitch_c &&
                     ps.frame_stride == pd.frame_stride;
    const bool any = ps.y == pd.y || (ps.u && ps.u == pd.u) || (ps.v && ps.v == pd.v);
    if (any && !all)
        return ppn::fail(PPN_E_INVALID, "%s: dst shares a plane with src but not every plane and the geometry (in place means all)",
                         who);
    if (int rc = check_call(who, cfg, !count || !kp_cell || !bbox || !workspace, batch, src->height, src->width, max_humans,
                            workspace))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t* k = kRgbToYuv[(src->full_range ? 2 : 0) + src->matrix];
    unsigned colour[PPN_MAX_KP];
    for (int i = 0; i < cfg->K; ++i) colour[i] = rgb_to_yuv(k, cfg->palette[i][0], cfg->palette[i][1], cfg->palette[i][2]);
    if (ov)
        for (unsigned& c : ov->colour) c = rgb_to_yuv(k, c & 0xffu, c >> 8 & 0xffu, c >> 16 & 0xffu);
    YuvRasterArgs ya{ps, pd, {}};
    if (int rc = launch_setup(cfg, colour, rgb_to_yuv(k, 110, 110, 110), count, kp_cell, bbox, batch, src->height, src->width,
                              max_humans, workspace, st, &ya.p, ov))
        return rc;
    const int mode = all ? YUV_INPLACE : word_aligned(src) && word_aligned(dst) ? YUV_WORDS : YUV_BYTES;
    const dim3 grid((src->width + 127) / 128, (src->height + TILE_H - 1) / TILE_H, batch);
    if (ov) launch_yuv_format<true>(src->format, mode, grid, st, ya);
    else launch_yuv_format<false>(src->format, mode, grid, st, ya);
    PPN_LAUNCH_CHECK();
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
    return draw_rgb("ppn_draw_humans", cfg, nullptr, src, dst, batch, height, width, count, kp_cell, bbox, max_humans, workspace,
                    stream);
}

extern "C" int ppn_rgb_to_yuv(int32_t matrix, int32_t full_range, const uint8_t* rgb, uint8_t* yuv, int64_t n) {
    if (matrix != 0 && matrix != 1) return ppn::fail(PPN_E_INVALID, "ppn_rgb_to_yuv: unknown matrix %d", matrix);
    if (n < 0 || (n > 0 && (!rgb || !yuv))) return ppn::fail(PPN_E_INVALID, "ppn_rgb_to_yuv: NULL pointer or negative count");
    const int32_t* k = kRgbToYuv[(full_range ? 2 : 0) + matrix];
    for (int64_t i = 0; i < n; ++i) {
        const unsigned c = rgb_to_yuv(k, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
        yuv[3 * i] = (uint8_t)c;
        yuv[3 * i + 1] = (uint8_t)(c >> 8);
        yuv[3 * i + 2] = (uint8_t)(c >> 16);
    }
    return PPN_OK;
}

extern "C" int ppn_draw_humans_yuv(const ppn_draw_cfg* cfg, const ppn_yuv_surface* src, const ppn_yuv_surface* dst, int32_t batch,
                                   const int32_t* count, const int32_t* kp_cell, const float* bbox, int32_t max_humans,
                                   void* workspace, void* stream) {
    const char* who = "ppn_draw_humans_yuv";
    if (int rc = check_cfg(cfg, who)) return rc;
    return draw_yuv(who, cfg, nullptr, src, dst, batch, count, kp_cell, bbox, max_humans, workspace, stream);
}

extern "C" size_t ppn_draw_scene_workspace_bytes(const ppn_draw_cfg* cfg, int32_t batch, int32_t max_humans) {
    const size_t people = ppn_draw_workspace_bytes(cfg, batch, max_humans);
    return people ? people + (size_t)batch * (OV_FIXED + OV_PERSON_SLOTS * (size_t)max_humans) * 3 * sizeof(int4) : 0;
}

extern "C" int ppn_draw_scene(const ppn_draw_cfg* cfg, const ppn_overlay_cfg* overlay, const ppn_overlay_in* in, const uint8_t* src,
                              uint8_t* dst, int32_t batch, int32_t height, int32_t width, const int32_t* count,
                              const int32_t* kp_cell, const float* bbox, int32_t max_humans, void* workspace, void* stream) {
    const char* who = "ppn_draw_scene";
    OverlayArgs ov;
    bool parts = false;
    if (int rc = check_cfg(cfg, who)) return rc;
    if (int rc = check_overlay(who, overlay, in, batch, max_humans, &ov, &parts)) return rc;
    return draw_rgb(who, cfg, parts ? &ov : nullptr, src, dst, batch, height, width, count, kp_cell, bbox, max_humans, workspace,
                    stream);
}

extern "C" int ppn_draw_scene_yuv(const ppn_draw_cfg* cfg, const ppn_overlay_cfg* overlay, const ppn_overlay_in* in,
                                  const ppn_yuv_surface* src, const ppn_yuv_surface* dst, int32_t batch, const int32_t* count,
                                  const int32_t* kp_cell, const float* bbox, int32_t max_humans, void* workspace, void* stream) {
    const char* who = "ppn_draw_scene_yuv";
    OverlayArgs ov;
    bool parts = false;
    if (int rc = check_cfg(cfg, who)) return rc;
    if (int rc = check_overlay(who, overlay, in, batch, max_humans, &ov, &parts)) return rc;
    return draw_yuv(who, cfg, parts ? &ov : nullptr, src, dst, batch, count, kp_cell, bbox, max_humans, workspace, stream);
}
