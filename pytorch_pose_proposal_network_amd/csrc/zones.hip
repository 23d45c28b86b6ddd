// Zones and counting lines: occupancy, entries, exits, dwell and directed line crossings of tracked people, kept per stream
// on the device (contract in include/ppn.h, ppn_zone_update; NumPy restatement tests/zones_ref.py).
//
//   zone_update_kernel   one workgroup of four waves per stream; the frames of the stream run in order inside it.  The
//                        stream's geometry is brought into LDS once per call.  Lane i of the first wave keeps slot i's id,
//                        gap, inside mask, 16 dwell counters and last anchor in registers for the whole call; lanes z < 16
//                        of it keep zone z's and line z's totals.  Per frame:
//     anchors  all threads, 16 lanes per person (lane z of the group tests zone z): anchor, validity, the polygon test; the
//              person's mask is its 16-bit field of the wave's ballot; anchor, mask and participating id go to LDS,
//              out_inside to memory; lane z adds up zone z's occupancy from the ballots
//     match    the first wave walks the participants in chunks of 64 and ballots "my slot holds this id", ages the unseen
//              slots and gives the r-th free slot to the r-th unheld participant (clips.hip's match, word for word)
//     events   the first wave, lane = slot: the line tests of the seen slots, entered / exited masks and dwell; per zone and
//              per line one popcll(ballot(..)) in a uniform loop, kept by lane z: no atomics
//     write    after a barrier all threads write out_slot; lanes z < 16 of the first wave out_zone and out_line
//   The count and the first 16 people of the next frame are asked for a frame ahead.
// The file is built with -ffp-contract=off and IEEE division: every f32 step is rounded on its own, as NumPy rounds it.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int NZ = PPN_ZONE_MAX, NV = PPN_ZONE_MAX_VERT, NL = PPN_LINE_MAX;
constexpr int PER_PASS = THREADS / NZ;                 // people per pass of the anchors step
constexpr int PER_WAVE = WAVE / NZ;                    // people per wave and pass
static_assert(PPN_ZONE_SLOTS == WAVE, "one lane per slot");
static_assert(NZ == 16 && NL == 16 && WAVE % NZ == 0, "a person's mask is a 16-bit field of a ballot");
static_assert(NZ * NV * 2 == THREADS, "one vertex coordinate per thread");
static_assert(PPN_MATCH_MAX_PEOPLE % WAVE == 0, "");

struct Args {
    ppn_zone_cfg c;
    ppn_zone_geom g;
    ppn_zone_state st;
    const int* count;            // [B]
    const int* kp_cell;          // [B][M][K]
    const float* bbox;           // [B][M][K][4] ymin, xmin, ymax, xmax
    const int* ids;              // [B][M]
    const float* xy;             // [B][M][K][2] or NULL
    const int* n_frames;         // [S] or NULL
    int* out_slot;               // [B][M]
    unsigned* out_inside;        // [B][M]
    int* out_zone;               // [B][16][4]
    int* out_line;               // [B][16][2]
    int F, M;                    // frames per stream, max_humans
};

__device__ __forceinline__ void wave_sync() {                                     // as track.hip's
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct Person {
    int id, cell;
    float v0, v1, v2, v3;        // the root box, or (x, y) of the smoothed root centre in v0, v1
};

// row p < M of image b: inside the buffers whatever the count says
__device__ __forceinline__ Person load_person(const Args& a, bool use_xy, size_t b, int p) {
    const size_t row = b * a.M + p;
    Person r;
    r.id = a.ids[row];
    r.cell = a.kp_cell[row * a.c.K];
    if (use_xy) {
        r.v0 = a.xy[row * a.c.K * 2], r.v1 = a.xy[row * a.c.K * 2 + 1], r.v2 = r.v3 = 0.f;
    } else {
        const float* box = a.bbox + row * a.c.K * 4;
        r.v0 = box[0], r.v1 = box[1], r.v2 = box[2], r.v3 = box[3];
    }
    return r;
}

__device__ __forceinline__ int sat_inc(int v) { return v < 0x7fffffff ? v + 1 : v; }

__global__ __launch_bounds__(THREADS) void zone_update_kernel(Args a) {
    __shared__ float s_zxy[NZ][NV][2];              // the stream's polygons
    __shared__ int s_znv[NZ];                       // their vertex numbers, clamped, 0: an empty zone
    __shared__ float s_lxy[NL][4];                  // the stream's lines
    __shared__ float s_ax[PPN_MATCH_MAX_PEOPLE];    // per person of the frame: the anchor,
    __shared__ float s_ay[PPN_MATCH_MAX_PEOPLE];
    __shared__ unsigned s_in[PPN_MATCH_MAX_PEOPLE]; // in_now,
    __shared__ int s_part[PPN_MATCH_MAX_PEOPLE];    // the id it takes part with, 0: it does not,
    __shared__ int s_pslot[PPN_MATCH_MAX_PEOPLE];   // its slot, -1: none; all -1 between two frames
    __shared__ int s_occ[WAVES][NZ];                // per wave the listed people in zone z
    __shared__ int s_cand[WAVE];                    // the first 64 birth candidates of the frame, ascending p
    __shared__ int s_cand_id[WAVE];                 // and their ids
    const int M = a.M, F = a.F;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wv = tid / WAVE;
    const bool first = tid < WAVE;                                                // the wave that owns the slots
    int nF = F;
    if (a.n_frames) nF = min(max(a.n_frames[s], 0), F);

    for (int t = nF; t < F; ++t) {                                                // frames that are not processed
        const size_t b = (size_t)s * F + t;
        for (int p = tid; p < M; p += THREADS) a.out_slot[b * M + p] = -1, a.out_inside[b * M + p] = 0u;
        if (tid < NZ * 4) a.out_zone[b * NZ * 4 + tid] = 0;
        if (tid < NL * 2) a.out_line[b * NL * 2 + tid] = 0;
    }
    if (nF == 0) return;                                                          // (uniform) the state stays untouched

    // ---- the stream's geometry, once per call
    const int zone_n = min(max(a.g.zone_n[s], 0), NZ), line_n = min(max(a.g.line_n[s], 0), NL);
    (&s_zxy[0][0][0])[tid] = a.g.zone_xy[(size_t)s * NZ * NV * 2 + tid];
    if (tid < NZ) {
        const int nv = min(max(a.g.zone_nv[s * NZ + tid], 0), NV);
        s_znv[tid] = tid < zone_n && nv >= 3 ? nv : 0;
    }
    if (tid < NL * 4) (&s_lxy[0][0])[tid] = a.g.line_xy[(size_t)s * NL * 4 + tid];
    for (int p = tid; p < M; p += THREADS) s_pslot[p] = -1;

    // ---- the state: slot `lane`, zone `lane` and line `lane`; only the first wave's is used
    const size_t slot = (size_t)s * WAVE + lane;
    int id = 0, gap = 0, flags = 0;
    unsigned inside = 0u;
    float lastx = 0.f, lasty = 0.f;
    int dwell[NZ];
    int zt_in = 0, zt_out = 0, lt_f = 0, lt_b = 0;
#pragma unroll
    for (int z = 0; z < NZ; ++z) dwell[z] = 0;
    if (first) {
        id = a.st.id[slot];
        gap = a.st.gap[slot];
        inside = a.st.inside[slot];
        lastx = a.st.last[slot * 2], lasty = a.st.last[slot * 2 + 1];
#pragma unroll
        for (int z = 0; z < NZ; ++z) dwell[z] = a.st.dwell[slot * NZ + z];
        if (lane < NZ) {
            const size_t w = ((size_t)s * NZ + lane) * 2;
            zt_in = a.st.zone_total[w], zt_out = a.st.zone_total[w + 1];
            lt_f = a.st.line_total[w], lt_b = a.st.line_total[w + 1];
        }
    }

    const bool use_xy = a.xy && a.c.anchor == PPN_ZONE_ANCHOR_CENTER;
    const bool bottom = a.c.anchor == PPN_ZONE_ANCHOR_BOTTOM;
    const int zq = lane % NZ, grp = lane / NZ;                                    // my zone and my person of the wave's four
    const int p_first = wv * PER_WAVE + grp;                                      // my person of the first pass

    // The frames of a stream run one after the other, so a frame should wait for as few memory round trips as it can: its
    // count and its first 16 people (rows < M lie inside the buffers whatever the count says) are asked for a frame ahead.
    int next_count = a.count[(size_t)s * F];
    Person next = {0, -1, 0.f, 0.f, 0.f, 0.f};
    if (p_first < M) next = load_person(a, use_xy, (size_t)s * F, p_first);
    lds_barrier();                                                                // the geometry is in LDS

    for (int t = 0; t < nF; ++t) {
        const size_t b = (size_t)s * F + t;
        const int P = min(max(next_count, 0), M);
        const Person ahead = next;
        if (t + 1 < nF) {
            next_count = a.count[b + 1];
            if (p_first < M) next = load_person(a, use_xy, b + 1, p_first);
        }

        // ---- anchors (step a): 16 lanes per person, lane zq tests zone zq; every lane of a wave runs every ballot
        int occ = 0;                                                              // lane z < 16: the wave's listed people in zone z
        const int nv = s_znv[zq];
        for (int c0 = 0; c0 < P; c0 += PER_PASS) {                                // (uniform)
            const int p = c0 + p_first;
            const bool listed = p < P;
            Person q = ahead;
            if (c0 > 0 && listed) q = load_person(a, use_xy, b, p);
            float ax, ay;
            if (use_xy) {
                ax = q.v0, ay = q.v1;
            } else {
                ax = (q.v1 + q.v3) * 0.5f;
                ay = bottom ? q.v2 : (q.v0 + q.v2) * 0.5f;
            }
            const bool valid = listed && q.cell >= 0 && __builtin_isfinite(ax) && __builtin_isfinite(ay);
            bool in = false;
            for (int i = 0; i < nv; ++i) {
                const int j = i == 0 ? nv - 1 : i - 1;
                const float xi = s_zxy[zq][i][0], yi = s_zxy[zq][i][1], xj = s_zxy[zq][j][0], yj = s_zxy[zq][j][1];
                const float cut = (xj - xi) * (ay - yi) / (yj - yi) + xi;         // NaN or inf on a horizontal edge: masked below
                in ^= ((yi > ay) != (yj > ay)) && ax < cut;
            }
            const unsigned long long bits = __ballot(valid && in);
            const unsigned mask = (unsigned)(bits >> (grp * NZ)) & 0xffffu;
            occ += __popcll((bits >> zq) & 0x0001000100010001ull);
            if (listed && zq == 0) {
                s_ax[p] = ax, s_ay[p] = ay, s_in[p] = mask;
                s_part[p] = valid && q.id > 0 ? q.id : 0;
                a.out_inside[b * M + p] = mask;
            }
        }
        if (lane < NZ) s_occ[wv][lane] = occ;
        for (int p = P + tid; p < M; p += THREADS) a.out_inside[b * M + p] = 0u;
        lds_barrier();

        if (first) {
            // ---- match (step b)
            const bool live = id != 0;
            int my_p = -1;                                                        // the person this slot sees or is born from
            int ncand = 0;                                                        // (uniform) birth candidates so far
            for (int c0 = 0; c0 < P; c0 += WAVE) {
                const int pj = c0 + lane;
                const int pid = pj < P ? s_part[pj] : 0;
                unsigned long long part = __ballot(pid > 0);                      // the chunk's participants
                while (part) {                                                    // (uniform)
                    const int j = __ffsll(part) - 1;
                    part &= part - 1;
                    const int v = __shfl(pid, j);
                    const bool mine = live && id == v;
                    const unsigned long long holders = __ballot(mine);
                    if (mine && my_p < 0) my_p = c0 + j;
                    if (lane == 0) {
                        if (holders) s_pslot[c0 + j] = __ffsll(holders) - 1;
                        else if (ncand < WAVE) {
                            s_cand[ncand] = c0 + j;
                            s_cand_id[ncand] = v;
                        }
                    }
                    ncand += holders ? 0 : 1;
                }
            }

            // ---- seen (step c), unseen (step e), freed (step f)
            const bool seen = my_p >= 0;
            const int sp = seen ? my_p : 0;
            const float p1x = s_ax[sp], p1y = s_ay[sp];                           // read by every lane; used by the seen ones
            const unsigned now = s_in[sp];
            unsigned ent = 0u, exi = 0u;
            int l_f = 0, l_b = 0;                                                 // lane l < 16: the frame's crossings of line l
            for (int l = 0; l < line_n; ++l) {                                    // (uniform)
                const float lax = s_lxy[l][0], lay = s_lxy[l][1], lbx = s_lxy[l][2], lby = s_lxy[l][3];
                const float dx = lbx - lax, dy = lby - lay;
                const bool side0 = dx * (lasty - lay) - dy * (lastx - lax) >= 0.f;
                const bool side1 = dx * (p1y - lay) - dy * (p1x - lax) >= 0.f;
                const float ux = p1x - lastx, uy = p1y - lasty;
                const float e0 = ux * (lay - lasty) - uy * (lax - lastx);
                const float e1 = ux * (lby - lasty) - uy * (lbx - lastx);
                const bool cross = seen && side0 != side1 && ((e0 <= 0.f && e1 >= 0.f) || (e0 >= 0.f && e1 <= 0.f));
                const int nf = __popcll(__ballot(cross && side1)), nb = __popcll(__ballot(cross && !side1));
                if (lane == l) l_f = nf, l_b = nb;
            }
            if (seen) {
                gap = 0;
                ent = now & ~inside, exi = inside & ~now;
#pragma unroll
                for (int z = 0; z < NZ; ++z)
                    if (z < zone_n) dwell[z] = (now >> z & 1u) ? ((inside >> z & 1u) ? sat_inc(dwell[z]) : 1) : 0;
                inside = now, lastx = p1x, lasty = p1y;
            } else if (live) {
                gap += 1;
                if (gap > a.c.max_gap) {
                    exi = inside;
                    id = gap = 0, inside = 0u;
#pragma unroll
                    for (int z = 0; z < NZ; ++z) dwell[z] = 0;
                } else {
#pragma unroll
                    for (int z = 0; z < NZ; ++z)
                        if (z < zone_n && (inside >> z & 1u)) dwell[z] = sat_inc(dwell[z]);
                }
            }

            // ---- births (step d): the r-th free slot takes the r-th candidate
            wave_sync();                                                          // lane 0's s_cand is read by every lane
            const unsigned long long free_mask = __ballot(id == 0);
            const int n_free = __popcll(free_mask);
            const int n_born = min(ncand, n_free);
            if (ncand > n_free) flags |= PPN_ZONE_FLAG_SLOT_OVERFLOW;
            const int rank = __popcll(free_mask & ((1ull << lane) - 1ull));
            if (id == 0 && rank < n_born) {
                const int bp = s_cand[rank];
                id = s_cand_id[rank];
                gap = 0;
                inside = s_in[bp];
                ent |= inside;                                                    // a slot freed just now keeps its exits
                lastx = s_ax[bp], lasty = s_ay[bp];
#pragma unroll
                for (int z = 0; z < NZ; ++z) dwell[z] = (int)(inside >> z & 1u);
                s_pslot[bp] = lane;
            }

            // ---- the frame's counts (step g): lane z keeps zone z's
            int n_ent = 0, n_exi = 0, n_loit = 0;
#pragma unroll
            for (int z = 0; z < NZ; ++z) {
                if (z < zone_n) {                                                 // (uniform)
                    const int ne = __popcll(__ballot(ent >> z & 1u)), nx = __popcll(__ballot(exi >> z & 1u));
                    const int nl = __popcll(__ballot(id != 0 && dwell[z] >= a.c.loiter));
                    if (lane == z) n_ent = ne, n_exi = nx, n_loit = nl;
                }
            }
            if (lane < NZ) {
                int n_occ = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) n_occ += s_occ[w][lane];
                if (lane >= zone_n) n_occ = 0;
                zt_in += n_ent, zt_out += n_exi, lt_f += l_f, lt_b += l_b;
                int* oz = a.out_zone + (b * NZ + lane) * 4;
                oz[0] = n_occ, oz[1] = n_ent, oz[2] = n_exi, oz[3] = n_loit;
                int* ol = a.out_line + (b * NL + lane) * 2;
                ol[0] = l_f, ol[1] = l_b;
            }
        }
        lds_barrier();

        // ---- write out_slot (step g).  The next frame's anchors step writes what the first wave has read before this
        // barrier, and the first wave reads s_pslot again only after the next frame's barrier.
        for (int p = tid; p < M; p += THREADS) {
            a.out_slot[b * M + p] = s_pslot[p];
            s_pslot[p] = -1;
        }
    }

    if (first) {
        a.st.id[slot] = id;
        a.st.gap[slot] = gap;
        a.st.inside[slot] = inside;
        a.st.last[slot * 2] = lastx, a.st.last[slot * 2 + 1] = lasty;
#pragma unroll
        for (int z = 0; z < NZ; ++z) a.st.dwell[slot * NZ + z] = dwell[z];
        if (lane < NZ) {
            const size_t w = ((size_t)s * NZ + lane) * 2;
            a.st.zone_total[w] = zt_in, a.st.zone_total[w + 1] = zt_out;
            a.st.line_total[w] = lt_f, a.st.line_total[w + 1] = lt_b;
        }
        if (lane == 0 && flags) a.st.flags[s] |= flags;                           // this workgroup owns the word: no atomic
    }
}

}  // namespace

extern "C" int ppn_zone_update(const ppn_zone_cfg* cfg, const ppn_zone_geom* geom, const ppn_zone_state* st,
                               const int32_t* count, const int32_t* kp_cell, const float* bbox, const int32_t* ids,
                               const float* xy, int32_t streams, int32_t frames, int32_t max_humans, const int32_t* n_frames,
                               int32_t* out_slot, uint32_t* out_inside, int32_t* out_zone, int32_t* out_line, void* stream) {
    const char* fn = "ppn_zone_update";
    if (!cfg || !geom || !st) return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", fn);
    if (!geom->zone_n || !geom->zone_nv || !geom->zone_xy || !geom->line_n || !geom->line_xy)
        return ppn::fail(PPN_E_INVALID, "%s: NULL geometry table", fn);
    if (!st->id || !st->gap || !st->inside || !st->dwell || !st->last || !st->zone_total || !st->line_total || !st->flags)
        return ppn::fail(PPN_E_INVALID, "%s: NULL state pointer", fn);
    if (cfg->K < 1 || cfg->K > PPN_MAX_KP) return ppn::fail(PPN_E_INVALID, "%s: K %d outside 1..%d", fn, cfg->K, PPN_MAX_KP);
    if (cfg->max_gap < 0) return ppn::fail(PPN_E_INVALID, "%s: max_gap %d must be >= 0", fn, cfg->max_gap);
    if (cfg->anchor != PPN_ZONE_ANCHOR_CENTER && cfg->anchor != PPN_ZONE_ANCHOR_BOTTOM)
        return ppn::fail(PPN_E_INVALID, "%s: unknown anchor %d", fn, cfg->anchor);
    if (cfg->loiter < 1) return ppn::fail(PPN_E_INVALID, "%s: loiter %d must be >= 1", fn, cfg->loiter);
    if (!count || !kp_cell || !bbox || !ids || !out_slot || !out_inside || !out_zone || !out_line)
        return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", fn);
    if (streams < 1 || frames < 1 || max_humans < 1)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry (%d streams, %d frames, max_humans %d)", fn, streams, frames,
                         max_humans);
    if (max_humans > PPN_MATCH_MAX_PEOPLE)
        return ppn::fail(PPN_E_UNSUPPORTED, "%s: max_humans %d beyond the limit %d", fn, max_humans, PPN_MATCH_MAX_PEOPLE);
    Args a{*cfg, *geom, *st, count, kp_cell, bbox, ids, xy, n_frames, out_slot, out_inside, out_zone, out_line, frames,
           max_humans};
    zone_update_kernel<<<(unsigned)streams, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
