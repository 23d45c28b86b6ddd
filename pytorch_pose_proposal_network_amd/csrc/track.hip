// Tracking people across the frames of a video: ids that follow a human and keypoint centres smoothed over time (contract
// in include/ppn.h, ppn_track_update; NumPy restatement tests/track_ref.py).
//
//   track_kernel<KMAX>   one workgroup of four waves per stream; the frames of the stream run in order inside it.  Lane i of
//                        the first wave keeps slot i's state in registers for the whole call: id, miss, hits, mask, root box
//                        and the 2K centres (static indices only: KMAX is 4, 18 or 32, nothing goes to scratch).  Per frame:
//     stage   all threads put the frame's D <= 256 people into LDS: centres, presence mask, root box, root score
//     match   the first wave walks p = 0 .. D-1.  Every lane reads person p from LDS (one address: a broadcast), computes
//             its slot's iou and n_close; the slot is elected by ballots over the bits of (n_close, iou bits) from the top
//             down and a find-first-set.  Nothing but integer comparisons: the order of the rules is the order of the bits.
//     update  lane-parallel: the taken lanes read their person, the others age, the free lanes take the birth candidates
//             the walk listed (the r-th free slot takes the r-th candidate: the same pairs as the sequential rule)
//     write   the first wave writes the tracked rows of out_xy from its registers; after a barrier all threads write out_id
//             and out_hits for every row and the raw centres of the untracked rows
// The file is built with -ffp-contract=off and IEEE division: every f32 step is rounded on its own, as NumPy rounds it.
#include "common.h"

#include <cmath>

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
static_assert(PPN_TRACK_SLOTS == WAVE, "one lane per track");
static_assert(PPN_MAX_KP <= 32, "the presence mask is one 32-bit word");
static_assert(PPN_TRACK_MAX_DET % WAVE == 0, "");

struct TrackArgs {
    ppn_track_cfg c;
    ppn_track_state st;
    const int* count;            // [B]
    const int* kp_cell;          // [B][M][K]
    const float* bbox;           // [B][M][K][4] ymin, xmin, ymax, xmax
    const float* score;          // [B][M][K]
    const int* n_frames;         // [S] or NULL
    int* out_id;                 // [B][M]
    int* out_hits;               // [B][M]
    float* out_xy;               // [B][M][K][2] or NULL
    int* out_live;               // [B]
    int T, M, dcap;              // frames per stream, max_humans, min(M, PPN_TRACK_MAX_DET): the LDS rows
};

// Orders the LDS traffic of one wave: the hardware executes a wave's LDS instructions in program order, this keeps the
// compiler from moving one lane's read above another lane's write.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float box_area(const float4& b) { return (b.z - b.x) * (b.w - b.y); }

// decode.hip's iou_ge without the comparison; a value that is not > 0 (NaN included) is 0
__device__ __forceinline__ float iou_of(const float4& bi, float ai, const float4& bj, float aj) {
    const float tl0 = fmaxf(bi.x, bj.x), tl1 = fmaxf(bi.y, bj.y);
    const float br0 = fminf(bi.z, bj.z), br1 = fminf(bi.w, bj.w);
    const float inter = ((br0 - tl0) * (br1 - tl1)) * ((tl0 < br0 && tl1 < br1) ? 1.0f : 0.0f);
    const float iou = inter / ((ai + aj) - inter);
    return iou > 0.0f ? iou : 0.0f;
}

template <int KMAX>
__global__ __launch_bounds__(THREADS) void track_kernel(TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cand[WAVE];         // the first 64 birth candidates of the frame, ascending p
    __shared__ int s_slot_id[WAVE];      // the slots after the frame, for the output pass
    __shared__ int s_slot_hits[WAVE];
    const int K = a.c.K, M = a.M, T = a.T, dcap = a.dcap;
    float4* s_box = reinterpret_cast<float4*>(smem);                              // [dcap] root box
    float2* s_c = reinterpret_cast<float2*>(s_box + dcap);                        // [dcap][K] centres, (0, 0) when absent
    float* s_score = reinterpret_cast<float*>(s_c + (size_t)dcap * K);            // [dcap] root score
    unsigned* s_mask = reinterpret_cast<unsigned*>(s_score + dcap);               // [dcap] presence bits
    int* s_pslot = reinterpret_cast<int*>(s_mask + dcap);                         // [dcap] the person's slot, -1: none

    const int s = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE;
    const bool first = tid < WAVE;                                                // the wave that owns the slots
    int nT = T;
    if (a.n_frames) nT = min(max(a.n_frames[s], 0), T);

    for (int t = nT; t < T; ++t) {                                                // frames that are not processed
        const size_t b = (size_t)s * T + t;
        for (int p = tid; p < M; p += THREADS) {
            a.out_id[b * M + p] = -1;
            a.out_hits[b * M + p] = 0;
        }
        if (tid == 0) a.out_live[b] = -1;
    }
    if (nT == 0) return;                                                          // (uniform) the state stays untouched

    // slot `lane` of this stream; only the first wave's copy is used
    const size_t slot = (size_t)s * WAVE + lane;
    int id = 0, miss = 0, hits = 0, last_id = 0, flags = 0;
    unsigned mask = 0;
    float4 root = make_float4(0.f, 0.f, 0.f, 0.f);
    float tx[KMAX], ty[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) tx[k] = ty[k] = 0.f;
    if (first) {
        id = a.st.id[slot];
        miss = a.st.miss[slot];
        hits = a.st.hits[slot];
        mask = a.st.mask[slot];
        root = make_float4(a.st.root[slot * 4], a.st.root[slot * 4 + 1], a.st.root[slot * 4 + 2], a.st.root[slot * 4 + 3]);
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                tx[k] = a.st.xy[(slot * K + k) * 2];
                ty[k] = a.st.xy[(slot * K + k) * 2 + 1];
            }
        last_id = a.st.last_id[s];
    }
    const float gate2 = a.c.kp_gate * a.c.kp_gate;

    int next_count = a.count[(size_t)s * T];
    for (int t = 0; t < nT; ++t) {
        const size_t b = (size_t)s * T + t;
        const int P = min(max(next_count, 0), M);
        const int D = min(P, PPN_TRACK_MAX_DET);                                  // <= dcap
        if (P > D) flags |= PPN_TRACK_FLAG_DET_OVERFLOW;
        const size_t row0 = b * M * K;                                            // first keypoint row of the image

        // ---- stage.  The frames of a stream run one after the other: the box is loaded beside its cell, not behind it
        // (rows p < P lie inside the buffers whatever they hold), a person's K cells are K loads in flight, and the next
        // frame's count is asked for a frame ahead, so that a frame waits for as few memory round trips as it can.
        for (int i = tid; i < D * K; i += THREADS) {
            const int cell = a.kp_cell[row0 + i];
            const float4 bb = reinterpret_cast<const float4*>(a.bbox)[row0 + i];
            s_c[i] = cell >= 0 ? make_float2((bb.y + bb.w) * 0.5f, (bb.x + bb.z) * 0.5f) : make_float2(0.f, 0.f);
        }
        for (int p = tid; p < D; p += THREADS) {
            int cell[KMAX];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) cell[k] = k < K ? a.kp_cell[row0 + (size_t)p * K + k] : -1;
            s_box[p] = reinterpret_cast<const float4*>(a.bbox)[row0 + (size_t)p * K];
            s_score[p] = a.score[row0 + (size_t)p * K];
            unsigned m = 0;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) m |= (cell[k] >= 0 ? 1u : 0u) << k;
            s_mask[p] = m;
        }
        if (t + 1 < nT) next_count = a.count[b + 1];
        lds_barrier();                                                            // LDS only: no global value is shared

        if (first) {
            // ---- match (steps 1 and 2)
            const bool live = id != 0;
            const float ai = box_area(root);
            const float r2 = gate2 * ai;
            bool taken = false;
            int my_p = -1;                                                        // the person this slot takes or is born from
            int ncand = 0;                                                        // (uniform) birth candidates so far
            for (int p = 0; p < D; ++p) {
                const unsigned pm = s_mask[p];
                int won = -1;
                if ((pm & 1u) && __ballot(live && !taken) != 0ull) {              // (uniform)
                    const float4 pb = s_box[p];
                    const float iou = iou_of(root, ai, pb, box_area(pb));
                    const unsigned both = pm & mask;
                    int n_close = 0;
#pragma unroll
                    for (int k = 1; k < KMAX; ++k)
                        if (k < K) {
                            const float2 c = s_c[p * K + k];
                            const float dx = c.x - tx[k], dy = c.y - ty[k];
                            const float xx = dx * dx, yy = dy * dy;
                            n_close += ((both >> k & 1u) && xx + yy <= r2) ? 1 : 0;
                        }
                    const bool eligible = live && !taken && (iou >= a.c.iou_thr || n_close >= a.c.min_close);
                    // The election: the largest n_close, then the largest iou (>= +0: its bits order as it does), then the
                    // lowest slot.  A maximum over lanes by ballots, no cross-lane traffic: from the top bit down, wherever
                    // some candidate has the bit, only those stay candidates.  The iou is walked only when several remain.
                    bool c = eligible;
                    unsigned long long m = __ballot(c);
                    if (m) {                                                      // (uniform, as every test of a ballot)
#pragma unroll
                        for (int bit = 4; bit >= 0; --bit) {
                            const bool has = c && (n_close >> bit & 1);
                            if (__ballot(has)) c = has;
                        }
                        m = __ballot(c);
                        if (m & (m - 1)) {
                            const unsigned ib = __float_as_uint(iou);
#pragma unroll
                            for (int bit = 31; bit >= 0; --bit) {
                                const bool has = c && (ib >> bit & 1u);
                                if (__ballot(has)) c = has;
                            }
                            m = __ballot(c);
                        }
                        won = __ffsll(m) - 1;
                    }
                }
                if (lane == won) {
                    taken = true;
                    my_p = p;
                }
                const bool cand = won < 0 && (pm & 1u) && s_score[p] >= a.c.birth_thr;     // (uniform)
                if (lane == 0) {
                    s_pslot[p] = won;
                    if (cand && ncand < WAVE) s_cand[ncand] = p;
                }
                ncand += cand ? 1 : 0;
            }

            // ---- update a taken slot (step 3), age the others (step 4)
            if (taken) {
                const unsigned pm = s_mask[my_p];
                root = s_box[my_p];
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K && (pm >> k & 1u)) {
                        const float2 c = s_c[my_p * K + k];
                        if ((mask >> k & 1u) && a.c.alpha != 1.0f) {
                            const float ddx = c.x - tx[k], ddy = c.y - ty[k];
                            const float sx = a.c.alpha * ddx, sy = a.c.alpha * ddy;
                            tx[k] = tx[k] + sx;
                            ty[k] = ty[k] + sy;
                        } else {
                            tx[k] = c.x;
                            ty[k] = c.y;
                        }
                    }
                mask = pm;
                miss = 0;
                hits += 1;
            } else if (live) {
                miss += 1;
                if (miss > a.c.max_age) {
                    id = miss = hits = 0;
                    mask = 0u;
                }
            }

            // ---- births (step 5): the r-th free slot takes the r-th candidate
            wave_sync();                                                          // lane 0's s_cand is read by every lane
            const unsigned long long free_mask = __ballot(id == 0);
            const int n_free = __popcll(free_mask);
            const int n_born = min(ncand, n_free);
            if (ncand > n_free) flags |= PPN_TRACK_FLAG_SLOT_OVERFLOW;
            const int rank = __popcll(free_mask & ((1ull << lane) - 1ull));
            if (id == 0 && rank < n_born) {
                my_p = s_cand[rank];
                const unsigned pm = s_mask[my_p];
                root = s_box[my_p];
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K && (pm >> k & 1u)) {
                        const float2 c = s_c[my_p * K + k];
                        tx[k] = c.x;
                        ty[k] = c.y;
                    }
                mask = pm;
                id = last_id + rank + 1;
                hits = 1;
                miss = 0;
                s_pslot[my_p] = lane;
            }
            last_id += n_born;

            // ---- the tracked rows of out_xy, and the slots for the output pass
            if (a.out_xy && my_p >= 0) {
                float2* o = reinterpret_cast<float2*>(a.out_xy) + (b * M + my_p) * K;
#pragma unroll
                for (int k = 0; k < KMAX; ++k)
                    if (k < K) o[k] = (mask >> k & 1u) ? make_float2(tx[k], ty[k]) : make_float2(0.f, 0.f);
            }
            s_slot_id[lane] = id;
            s_slot_hits[lane] = hits;
            const int n_live = __popcll(__ballot(id != 0));
            if (lane == 0) a.out_live[b] = n_live;
        }
        lds_barrier();

        // ---- write (step 6): ids and hits of every row, raw centres of the untracked rows
        for (int p = tid; p < M; p += THREADS) {
            const int sl = p < D ? s_pslot[p] : -1;
            a.out_id[b * M + p] = sl >= 0 ? s_slot_id[sl] : -1;
            a.out_hits[b * M + p] = sl >= 0 ? s_slot_hits[sl] : 0;
        }
        if (a.out_xy) {
            for (int i = tid; i < P * K; i += THREADS) {
                const int p = i / K;
                if (p < D && s_pslot[p] >= 0) continue;
                const int cell = a.kp_cell[row0 + i];
                const float4 bb = reinterpret_cast<const float4*>(a.bbox)[row0 + i];
                reinterpret_cast<float2*>(a.out_xy)[row0 + i] =
                    cell >= 0 ? make_float2((bb.y + bb.w) * 0.5f, (bb.x + bb.z) * 0.5f) : make_float2(0.f, 0.f);
            }
        }
        // the next frame's stage writes none of s_pslot / s_slot_*: the first wave rewrites them behind the stage's barrier
    }

    if (first) {
        a.st.id[slot] = id;
        a.st.miss[slot] = miss;
        a.st.hits[slot] = hits;
        a.st.mask[slot] = mask;
        a.st.root[slot * 4] = root.x;
        a.st.root[slot * 4 + 1] = root.y;
        a.st.root[slot * 4 + 2] = root.z;
        a.st.root[slot * 4 + 3] = root.w;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                a.st.xy[(slot * K + k) * 2] = tx[k];
                a.st.xy[(slot * K + k) * 2 + 1] = ty[k];
            }
        if (lane == 0) {
            a.st.last_id[s] = last_id;
            if (flags) a.st.flags[s] |= flags;                                    // this workgroup owns the word: no atomic
        }
    }
}

template <int KMAX>
int launch(const TrackArgs& a, int streams, size_t lds, hipStream_t stream) {
    static int lds_set = 64 * 1024;                                               // the limit a kernel has without asking
    PPN_LDS_ONCE(lds_set, reinterpret_cast<const void*>(track_kernel<KMAX>), hipFuncAttributeMaxDynamicSharedMemorySize,
                 (int)lds);
    track_kernel<KMAX><<<(unsigned)streams, THREADS, lds, stream>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

}  // namespace

extern "C" int ppn_track_update(const ppn_track_cfg* cfg, const ppn_track_state* st, const int32_t* count,
                                const int32_t* kp_cell, const float* bbox, const float* score, int32_t streams,
                                int32_t frames, int32_t max_humans, const int32_t* n_frames, int32_t* out_id,
                                int32_t* out_hits, float* out_xy, int32_t* out_live, void* stream) {
    if (!cfg || !st || !count || !kp_cell || !bbox || !score || !out_id || !out_hits || !out_live)
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: NULL pointer");
    if (!st->id || !st->miss || !st->hits || !st->mask || !st->root || !st->xy || !st->last_id || !st->flags)
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: NULL state pointer");
    if (cfg->K < 1 || cfg->K > PPN_MAX_KP)
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: K %d outside 1..%d", cfg->K, PPN_MAX_KP);
    if (cfg->min_close < 1 || cfg->max_age < 0)
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: min_close %d must be >= 1 and max_age %d >= 0", cfg->min_close,
                         cfg->max_age);
    if (!std::isfinite(cfg->iou_thr) || !std::isfinite(cfg->kp_gate) || !std::isfinite(cfg->birth_thr) ||
        !std::isfinite(cfg->alpha))
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: a cfg value is not finite");
    if (cfg->iou_thr < 0.f || cfg->iou_thr > 1.f || cfg->kp_gate < 0.f || !(cfg->alpha > 0.f) || cfg->alpha > 1.f)
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: iou_thr %g must be in [0, 1], kp_gate %g >= 0, alpha %g in (0, 1]",
                         cfg->iou_thr, cfg->kp_gate, cfg->alpha);
    if (streams < 1 || frames < 1 || max_humans < 1)
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: bad geometry (%d streams, %d frames, max_humans %d)", streams,
                         frames, max_humans);
    if (reinterpret_cast<uintptr_t>(bbox) % 16)
        return ppn::fail(PPN_E_INVALID, "ppn_track_update: bbox must be 16-byte aligned");
    if (max_humans > PPN_MATCH_MAX_PEOPLE)
        return ppn::fail(PPN_E_UNSUPPORTED, "ppn_track_update: max_humans %d beyond the limit %d", max_humans,
                         PPN_MATCH_MAX_PEOPLE);
    TrackArgs a{*cfg, *st, count, kp_cell, bbox, score, n_frames, out_id, out_hits, out_xy, out_live, frames, max_humans,
                max_humans < PPN_TRACK_MAX_DET ? max_humans : PPN_TRACK_MAX_DET};
    // per LDS row: root box 16, K centres 8K, score 4, mask 4, slot 4 -- 43 KB for 256 people of 18 keypoints
    const size_t lds = (size_t)a.dcap * (16 + 8 * (size_t)cfg->K + 12);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (cfg->K <= 4) return launch<4>(a, streams, lds, hs);
    if (cfg->K <= 18) return launch<18>(a, streams, lds, hs);
    return launch<32>(a, streams, lds, hs);
}
