// Per-track skeleton clips: the last T frames of every tracked person's keypoints, kept on the device as a ring per track
// id and handed out as one [3, T, K] tensor per person (contract in include/ppn.h, ppn_clip_push / ppn_clip_gather; NumPy
// restatement tests/clips_ref.py).
//
//   clip_push_kernel       one workgroup of four waves per stream; the frames of the stream run in order inside it.  Lane i of
//                          the first wave keeps slot i's id, gap and len in registers for the whole call.  Per frame:
//     match   the first wave walks the frame's ids in chunks of 64 (lane j holds person c * 64 + j) and, per participant in
//             ascending p, ballots "my slot holds this id": the slot learns its person, the person its slot, and a
//             participant nobody holds is listed as a birth candidate
//     age     lane-parallel: seen slots reset their gap, the others age and may be freed; the r-th free slot takes the r-th
//             candidate (the same pairs as the sequential rule).  No global load so far but the ids past the first 64
//     write   after a barrier all threads write out_row, and every wave, for 16 slots of its own that were live or are
//             born, the 3K floats of ring row r (two per lane), the row's presence mask (a ballot over the lanes that hold
//             plane x) and the ref box: all loads of the frame are issued before its first store
//   clip_gather_kernel<V>  one workgroup per (stream, slot): the ring rows in chronological order into [3][T][K], V floats
//                          per thread and access (runs of K floats are contiguous on both sides), zeros for the left padding
//                          and for free slots, the root-box normalisation on the way
// The file is built with -ffp-contract=off and IEEE division: every f32 step is rounded on its own, as NumPy rounds it.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int PER_WAVE = PPN_CLIP_SLOTS / WAVES;       // slots whose rows one wave writes
static_assert(3 * PPN_MAX_KP <= 2 * WAVE, "a ring row is at most two elements per lane");
static_assert(PPN_CLIP_SLOTS == WAVE, "one lane per clip");
static_assert(PPN_MAX_KP <= 32, "the presence mask is one 32-bit word");
static_assert(PPN_MATCH_MAX_PEOPLE % WAVE == 0, "");

struct PushArgs {
    ppn_clip_cfg c;
    ppn_clip_state st;
    const int* count;            // [B]
    const int* kp_cell;          // [B][M][K]
    const float* bbox;           // [B][M][K][4] ymin, xmin, ymax, xmax
    const float* score;          // [B][M][K]
    const int* ids;              // [B][M]
    const float* xy;             // [B][M][K][2] or NULL
    const int* n_frames;         // [S] or NULL
    int* out_row;                // [B][M]
    int F, M;                    // frames per stream, max_humans
};

__device__ __forceinline__ void wave_sync() {                                     // as track.hip's
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(THREADS) void clip_push_kernel(PushArgs a) {
    __shared__ int s_pslot[PPN_MATCH_MAX_PEOPLE];   // the person's slot, -1: none; all -1 between two frames
    __shared__ int s_cand[WAVE];                    // the first 64 birth candidates of the frame, ascending p
    __shared__ int s_cand_id[WAVE];                 // and their ids
    __shared__ int s_src[WAVE];                     // per slot the person whose row it gets, -1: a zero row, -2: no row
    const int K = a.c.K, L = a.c.length, M = a.M, F = a.F;
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE;
    const bool first = tid < WAVE;                                                // the wave that owns the slots
    int nF = F;
    if (a.n_frames) nF = min(max(a.n_frames[s], 0), F);

    for (int t = nF; t < F; ++t) {                                                // frames that are not processed
        const size_t b = (size_t)s * F + t;
        for (int p = tid; p < M; p += THREADS) a.out_row[b * M + p] = -1;
    }
    if (nF == 0) return;                                                          // (uniform) the state stays untouched

    const size_t slot = (size_t)s * WAVE + lane;                                  // slot `lane`; only the first wave's is used
    int id = 0, gap = 0, len = 0, flags = 0;
    if (first) {
        id = a.st.id[slot];
        gap = a.st.gap[slot];
        len = a.st.len[slot];
    }
    int r = a.st.pos[s];
    r = min(max(r, 0), L - 1);                                                    // 0..L-1 by contract; never leave the ring
    for (int p = tid; p < M; p += THREADS) s_pslot[p] = -1;

    // the two elements e = lane, lane + 64 of a ring row (3K <= 96) that this thread writes for every slot of its wave, and
    // where their values come from: score[k], xy[k][plane], or the two box edges whose mean is the centre
    const int K3 = 3 * K, wv = tid / WAVE;
    bool ok[2], avg[2];
    int ek[2], mul[2], off1[2], off2[2];
    const float *base1[2], *base2[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = lane + q * WAVE;
        ok[q] = e < K3;
        const int ec = min(e, K3 - 1), plane = ec / K, k = ec - plane * K;
        ek[q] = k;
        avg[q] = plane < 2 && !a.xy;
        if (plane == 2) {
            base1[q] = base2[q] = a.score, mul[q] = 1, off1[q] = off2[q] = k;
        } else if (a.xy) {
            base1[q] = base2[q] = a.xy, mul[q] = 2, off1[q] = off2[q] = k * 2 + plane;
        } else {
            base1[q] = base2[q] = a.bbox, mul[q] = 4, off1[q] = k * 4 + 1 - plane, off2[q] = k * 4 + 3 - plane;
        }
    }

    // The frames of a stream run one after the other, so a frame should wait for as few memory round trips as it can: its
    // count and its first 64 ids (rows < M lie inside the buffer whatever the count says) are asked for a frame ahead.
    int next_count = a.count[(size_t)s * F];
    int next_ids = first && lane < M ? a.ids[(size_t)s * F * M + lane] : 0;
    for (int t = 0; t < nF; ++t) {
        const size_t b = (size_t)s * F + t;
        const int P = min(max(next_count, 0), M);
        const int ids0 = next_ids;
        if (t + 1 < nF) {
            next_count = a.count[b + 1];
            if (first && lane < M) next_ids = a.ids[(b + 1) * M + lane];
        }
        lds_barrier();                                                            // the last frame's readers are done

        if (first) {
            // ---- match (steps a and b)
            const bool live = id != 0;
            int my_p = -1;                                                        // the person this slot sees or is born from
            int ncand = 0;                                                        // (uniform) birth candidates so far
            for (int c0 = 0; c0 < P; c0 += WAVE) {
                const int pj = c0 + lane;
                const int pid = pj < P ? (c0 == 0 ? ids0 : a.ids[b * M + pj]) : 0;
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

            // ---- seen (step b), unseen (step c)
            int src = -2;
            if (my_p >= 0) {
                gap = 0;
                len = min(len + 1, L);
                src = my_p;
            } else if (live) {
                src = -1;
                gap += 1;
                len = min(len + 1, L);
                if (gap > a.c.max_gap) id = gap = len = 0;
            }

            // ---- births (step d): the r-th free slot takes the r-th candidate
            wave_sync();                                                          // lane 0's s_cand is read by every lane
            const unsigned long long free_mask = __ballot(id == 0);
            const int n_free = __popcll(free_mask);
            const int n_born = min(ncand, n_free);
            if (ncand > n_free) flags |= PPN_CLIP_FLAG_SLOT_OVERFLOW;
            const int rank = __popcll(free_mask & ((1ull << lane) - 1ull));
            if (id == 0 && rank < n_born) {
                my_p = s_cand[rank];
                id = s_cand_id[rank];
                gap = 0;
                len = 1;
                src = my_p;
                s_pslot[my_p] = lane;
            }
            s_src[lane] = src;
        }
        lds_barrier();

        // ---- write (step e): out_row of every row; ring row r, its mask and ref of every slot that was live or was born.
        // A thread meets the same slots, the same two elements of a row and the same p in every frame, so its stores to
        // one address stay in program order.  First every load of the frame (value and cell side by side: a listed
        // person's rows lie inside the buffers whatever they hold; the slots without a person are skipped wave-uniformly),
        // then the stores: one memory round trip per frame instead of one per slot.
        for (int p = tid; p < M; p += THREADS) {
            a.out_row[b * M + p] = s_pslot[p];
            s_pslot[p] = -1;
        }
        int src[PER_WAVE], cell[PER_WAVE][2];
        float va[PER_WAVE][2], vb[PER_WAVE][2], rootv[PER_WAVE];
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            src[i] = s_src[i * WAVES + wv];                                       // (uniform)
            rootv[i] = 0.f;
#pragma unroll
            for (int q = 0; q < 2; ++q) cell[i][q] = -1, va[i][q] = vb[i][q] = 0.f;
            if (src[i] < 0) continue;                                             // (uniform) nothing to load
            const size_t prow = (b * M + src[i]) * K;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                cell[i][q] = a.kp_cell[prow + ek[q]];
                va[i][q] = base1[q][prow * mul[q] + off1[q]];
                vb[i][q] = base2[q][prow * mul[q] + off2[q]];
            }
            rootv[i] = a.bbox[prow * 4 + (lane & 3)];
        }
#pragma unroll
        for (int i = 0; i < PER_WAVE; ++i) {
            if (src[i] == -2) continue;                                           // (uniform) a free slot: no row
            const size_t sl = (size_t)s * WAVE + i * WAVES + wv;
            const bool person = src[i] >= 0;
            const unsigned long long present = __ballot(person && lane < K && cell[i][0] >= 0);   // lane k < K: plane x, keypoint k
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const float v = avg[q] ? (va[i][q] + vb[i][q]) * 0.5f : va[i][q];
                if (ok[q]) a.st.ring[(sl * L + r) * K3 + lane + q * WAVE] = person && cell[i][q] >= 0 ? v : 0.f;
            }
            if (lane == 0) a.st.mask[sl * L + r] = (unsigned)present;
            if (person && lane < 4) a.st.ref[sl * 4 + lane] = rootv[i];
        }
        r = r + 1 == L ? 0 : r + 1;
    }

    if (first) {
        a.st.id[slot] = id;
        a.st.gap[slot] = gap;
        a.st.len[slot] = len;
        if (lane == 0) {
            a.st.pos[s] = r;
            if (flags) a.st.flags[s] |= flags;                                    // this workgroup owns the word: no atomic
        }
    }
}

struct GatherArgs {
    ppn_clip_cfg c;
    ppn_clip_state st;
    float* out;                  // [S][64][3][T][K]
    int* out_id;                 // [S][64]
    int* out_len;                // [S][64]
};

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<2> { typedef float2 type; };
template <> struct Vec<4> { typedef float4 type; };

// V floats of one keypoint run: K % V == 0, so a vector never straddles two runs
template <int V>
__global__ __launch_bounds__(THREADS) void clip_gather_kernel(GatherArgs a) {
    typedef typename Vec<V>::type vec;
    const int K = a.c.K, L = a.c.length, KV = K / V;
    const size_t slot = blockIdx.x;                                               // s * 64 + i
    const int s = (int)(slot / WAVE);
    const int id = a.st.id[slot], len = min(max(a.st.len[slot], 0), L);
    const int pos = min(max(a.st.pos[s], 0), L - 1);
    if (threadIdx.x == 0) {
        a.out_id[slot] = id;
        a.out_len[slot] = a.st.len[slot];
    }
    const int first_valid = id != 0 ? L - len : L;                                // time steps before it are padding
    float cx = 0.f, cy = 0.f, sc = 1.f;
    const bool norm = a.c.norm == PPN_CLIP_NORM_ROOT;
    if (norm) {
        const float r0 = a.st.ref[slot * 4], r1 = a.st.ref[slot * 4 + 1], r2 = a.st.ref[slot * 4 + 2], r3 = a.st.ref[slot * 4 + 3];
        cx = (r1 + r3) * 0.5f;
        cy = (r0 + r2) * 0.5f;
        const float h = r2 - r0, w = r3 - r1;
        sc = h > w ? h : w;
        if (!(sc > 0.f)) sc = 1.0f;
    }
    const float* ring = a.st.ring + slot * L * 3 * K;
    const unsigned* mask = a.st.mask + slot * L;
    float* out = a.out + slot * 3 * L * K;
    const int per_plane = L * KV, total = 3 * per_plane;
    for (int u = threadIdx.x; u < total; u += THREADS) {
        const int plane = u / per_plane, rest = u - plane * per_plane;
        const int j = rest / KV, k0 = (rest - j * KV) * V;
        alignas(16) float v[V];
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = 0.f;
        if (j >= first_valid) {
            int row = pos + j;
            row = row >= L ? row - L : row;
            *reinterpret_cast<vec*>(v) = *reinterpret_cast<const vec*>(ring + ((size_t)row * 3 + plane) * K + k0);
            if (norm && plane < 2) {
                const unsigned m = mask[row] >> k0;
                const float c = plane == 0 ? cx : cy;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float d = v[i] - c;
                    v[i] = (m >> i & 1u) ? d / sc : 0.f;
                }
            }
        }
        *reinterpret_cast<vec*>(out + ((size_t)plane * L + j) * K + k0) = *reinterpret_cast<vec*>(v);
    }
}

int check_common(const char* fn, const ppn_clip_cfg* cfg, const ppn_clip_state* st) {
    if (!cfg || !st) return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", fn);
    if (!st->id || !st->gap || !st->len || !st->ref || !st->mask || !st->ring || !st->pos || !st->flags)
        return ppn::fail(PPN_E_INVALID, "%s: NULL state pointer", fn);
    if (cfg->K < 1 || cfg->K > PPN_MAX_KP) return ppn::fail(PPN_E_INVALID, "%s: K %d outside 1..%d", fn, cfg->K, PPN_MAX_KP);
    if (cfg->length < 1 || cfg->length > PPN_CLIP_MAX_LEN)
        return ppn::fail(PPN_E_INVALID, "%s: length %d outside 1..%d", fn, cfg->length, PPN_CLIP_MAX_LEN);
    if (cfg->max_gap < 0) return ppn::fail(PPN_E_INVALID, "%s: max_gap %d must be >= 0", fn, cfg->max_gap);
    if (cfg->norm != PPN_CLIP_NORM_NONE && cfg->norm != PPN_CLIP_NORM_ROOT)
        return ppn::fail(PPN_E_INVALID, "%s: unknown norm %d", fn, cfg->norm);
    return PPN_OK;
}

}  // namespace

extern "C" int ppn_clip_push(const ppn_clip_cfg* cfg, const ppn_clip_state* st, const int32_t* count, const int32_t* kp_cell,
                             const float* bbox, const float* score, const int32_t* ids, const float* xy, int32_t streams,
                             int32_t frames, int32_t max_humans, const int32_t* n_frames, int32_t* out_row, void* stream) {
    if (const int rc = check_common("ppn_clip_push", cfg, st)) return rc;
    if (!count || !kp_cell || !bbox || !score || !ids || !out_row)
        return ppn::fail(PPN_E_INVALID, "ppn_clip_push: NULL pointer");
    if (streams < 1 || frames < 1 || max_humans < 1)
        return ppn::fail(PPN_E_INVALID, "ppn_clip_push: bad geometry (%d streams, %d frames, max_humans %d)", streams, frames,
                         max_humans);
    if (max_humans > PPN_MATCH_MAX_PEOPLE)
        return ppn::fail(PPN_E_UNSUPPORTED, "ppn_clip_push: max_humans %d beyond the limit %d", max_humans,
                         PPN_MATCH_MAX_PEOPLE);
    PushArgs a{*cfg, *st, count, kp_cell, bbox, score, ids, xy, n_frames, out_row, frames, max_humans};
    clip_push_kernel<<<(unsigned)streams, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_clip_gather(const ppn_clip_cfg* cfg, const ppn_clip_state* st, int32_t streams, float* out, int32_t* out_id,
                               int32_t* out_len, void* stream) {
    if (const int rc = check_common("ppn_clip_gather", cfg, st)) return rc;
    if (!out || !out_id || !out_len) return ppn::fail(PPN_E_INVALID, "ppn_clip_gather: NULL pointer");
    if (streams < 1) return ppn::fail(PPN_E_INVALID, "ppn_clip_gather: %d streams", streams);
    GatherArgs a{*cfg, *st, out, out_id, out_len};
    const unsigned grid = (unsigned)streams * PPN_CLIP_SLOTS;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    // the widest vector that the keypoint runs and both base addresses allow
    const uintptr_t both = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(st->ring);
    if (cfg->K % 4 == 0 && both % 16 == 0) clip_gather_kernel<4><<<grid, THREADS, 0, hs>>>(a);
    else if (cfg->K % 2 == 0 && both % 8 == 0) clip_gather_kernel<2><<<grid, THREADS, 0, hs>>>(a);
    else clip_gather_kernel<1><<<grid, THREADS, 0, hs>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
