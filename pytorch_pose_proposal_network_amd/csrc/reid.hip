// Re-identification by appearance: an integer colour descriptor per person, read from the raw frame, and a gallery per
// stream that hands out persistent ids (contract in include/ppn.h, ppn_people_descr / ppn_reid_update; NumPy restatement
// tests/reid_ref.py).  No float arithmetic anywhere in this file, no global atomics, plain vector stores.
//
//   people_descr_kernel   one workgroup of four waves per (frame, slot).  The slot is judged first, from two uniform loads
//                         (status and the rectangle): an empty or bad slot writes its zeros and leaves without a read of the
//                         surface.  A wave takes two sample rows per pass, lanes 0..31 the 32 columns of the one and lanes
//                         32..63 of the other, so the luma bytes of a sample row come from one row of the plane; the four
//                         waves take 8 rows per pass and 12 passes make the 96 rows, 4 passes per band, so the band is a
//                         constant of the unrolled pass.  A bin's count is popcll(ballot(bin == q)), kept by lane
//                         channel * 8 + q: no atomics, not even in LDS.  The waves' 72 counts are added through LDS.
//   reid_update_kernel    one wave per stream, lane i owns entries i and i + 64: pid, tid, lost and n in registers for the
//                         whole call, the 128 descriptors transposed in LDS ([count][entry]: two lanes per dword, no bank
//                         conflict).  Per frame: the people's ids go to LDS; every lane walks them for its two tids (bound);
//                         the newcomers with a descriptor are taken one by one, every lane scores its two entries and one
//                         64-bit max over the wave picks the winner -- (similarity, -lost, -index) packed into the key;
//                         ageing; births by rank (the r-th newcomer takes the r-th free entry); outputs.
#include "common.h"

namespace {

constexpr int ROWS = PPN_DESCR_ROWS, COLS = PPN_DESCR_COLS, LEN = PPN_DESCR_LEN, BINS = PPN_DESCR_BINS;
constexpr int DESCR_THREADS = 256, WAVE = 64, DESCR_WAVES = DESCR_THREADS / WAVE;
constexpr int ROWS_PER_PASS = DESCR_WAVES * (WAVE / COLS);          // 8
constexpr int PASSES = ROWS / ROWS_PER_PASS;                        // 12
constexpr int PASSES_PER_BAND = PASSES / PPN_DESCR_BANDS;           // 4
static_assert(COLS == 32 && WAVE % COLS == 0 && ROWS % ROWS_PER_PASS == 0 && PASSES % PPN_DESCR_BANDS == 0, "");
static_assert(LEN == PPN_DESCR_BANDS * 3 * BINS && 3 * BINS <= WAVE && LEN <= DESCR_THREADS, "");

struct DescrArgs {
    const unsigned char *y, *u, *v;
    int64_t frame_stride;
    int pitch, pitch_c, height, width;
    const int* roi;              // [F][R][4]
    const int* status;           // [F][R]
    unsigned short* descr;       // [F][R][72]
    int* valid;                  // [F][R]
    int R;
};

__device__ __forceinline__ int bin_luma(int c) { return c >> 5; }
__device__ __forceinline__ int bin_chroma(int c) { return (min(max(c, 64), 191) - 64) >> 4; }

template <int FMT>
__global__ __launch_bounds__(DESCR_THREADS) void people_descr_kernel(DescrArgs a) {
    __shared__ int s_h[DESCR_WAVES][LEN];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wv = tid / WAVE;
    const int* q = a.roi + (size_t)img * 4;
    const int y0 = q[0], x0 = q[1], h = q[2], w = q[3];
    bool good = a.status[img] == PPN_ROI_OK && y0 >= 0 && x0 >= 0 && h >= 1 && w >= 1 && h <= a.height && w <= a.width &&
                y0 <= a.height - h && x0 <= a.width - w;
    if (FMT != PPN_PIX_BGR24) good = good && !((x0 | w) & 1);
    if (FMT == PPN_PIX_NV12 || FMT == PPN_PIX_I420) good = good && !((y0 | h) & 1);
    unsigned short* out = a.descr + (size_t)img * LEN;
    if (!good) {                                                    // uniform: the whole workgroup leaves without a read
        if (tid < LEN) out[tid] = 0;
        if (tid == 0) a.valid[img] = 0;
        return;
    }
    const size_t f = (size_t)(img / a.R);
    const unsigned char* py = a.y + f * (size_t)a.frame_stride;
    const unsigned char* pu = FMT == PPN_PIX_NV12 || FMT == PPN_PIX_I420 ? a.u + f * (size_t)a.frame_stride : nullptr;
    const unsigned char* pv = FMT == PPN_PIX_I420 ? a.v + f * (size_t)a.frame_stride : nullptr;
    const int j = lane % COLS, sub = wv * (WAVE / COLS) + lane / COLS;
    const int x = x0 + ((2 * j + 1) * w) / (2 * COLS);             // inside the rectangle: (63 * w) / 64 < w

    int c0[PASSES], c1[PASSES], c2[PASSES];                         // all loads first, then the counting
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int i = ps * ROWS_PER_PASS + sub;
        const int y = y0 + ((2 * i + 1) * h) / (2 * ROWS);         // (191 * h) / 192 < h
        if (FMT == PPN_PIX_BGR24) {
            const unsigned char* p = py + (size_t)y * a.pitch + 3 * x;
            c1[ps] = p[0], c0[ps] = p[1], c2[ps] = p[2];            // (G, B, R)
        } else if (FMT == PPN_PIX_YUYV) {
            const unsigned char* row = py + (size_t)y * a.pitch;
            c0[ps] = row[2 * x], c1[ps] = row[4 * (x >> 1) + 1], c2[ps] = row[4 * (x >> 1) + 3];
        } else if (FMT == PPN_PIX_NV12) {
            const unsigned char* c = pu + (size_t)(y >> 1) * a.pitch_c + 2 * (x >> 1);
            c0[ps] = py[(size_t)y * a.pitch + x], c1[ps] = c[0], c2[ps] = c[1];
        } else {
            const size_t c = (size_t)(y >> 1) * a.pitch_c + (x >> 1);
            c0[ps] = py[(size_t)y * a.pitch + x], c1[ps] = pu[c], c2[ps] = pv[c];
        }
    }

    int acc[PPN_DESCR_BANDS] = {0, 0, 0};                           // lane ch * 8 + q < 24: the wave's count of that bin
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
        const int b0 = bin_luma(c0[ps]);
        const int b1 = FMT == PPN_PIX_BGR24 ? bin_luma(c1[ps]) : bin_chroma(c1[ps]);
        const int b2 = FMT == PPN_PIX_BGR24 ? bin_luma(c2[ps]) : bin_chroma(c2[ps]);
        int add = 0;
#pragma unroll
        for (int qb = 0; qb < BINS; ++qb) {
            const int n0 = __popcll(__ballot(b0 == qb)), n1 = __popcll(__ballot(b1 == qb)), n2 = __popcll(__ballot(b2 == qb));
            add = lane == qb ? n0 : lane == BINS + qb ? n1 : lane == 2 * BINS + qb ? n2 : add;
        }
        acc[ps / PASSES_PER_BAND] += add;
    }
    if (lane < 3 * BINS) {
#pragma unroll
        for (int bd = 0; bd < PPN_DESCR_BANDS; ++bd) s_h[wv][bd * 3 * BINS + lane] = acc[bd];
    }
    __syncthreads();
    if (tid < LEN) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < DESCR_WAVES; ++k) sum += s_h[k][tid];
        out[tid] = (unsigned short)sum;
    }
    if (tid == 0) a.valid[img] = 1;
}

// what ppn_redact_yuv refuses of one surface (redact.hip's check_surface, which is local to that file)
int check_surface(const char* who, const ppn_yuv_surface* s) {
    if (!s) return ppn::fail(PPN_E_INVALID, "%s: NULL surface", who);
    const int fmt = s->format;
    if (fmt != PPN_PIX_NV12 && fmt != PPN_PIX_I420 && fmt != PPN_PIX_YUYV && fmt != PPN_PIX_BGR24)
        return ppn::fail(PPN_E_INVALID, "%s: unknown format %d", who, fmt);
    const bool bgr = fmt == PPN_PIX_BGR24, is420 = fmt == PPN_PIX_NV12 || fmt == PPN_PIX_I420;
    if (!bgr && s->matrix != 0 && s->matrix != 1) return ppn::fail(PPN_E_INVALID, "%s: unknown matrix %d", who, s->matrix);
    if (!s->y || (is420 && !s->u) || (fmt == PPN_PIX_I420 && !s->v)) return ppn::fail(PPN_E_INVALID, "%s: NULL plane", who);
    if (s->height < 1 || s->width < 1 || s->height > 16384 || s->width > 16384)
        return ppn::fail(PPN_E_INVALID, "%s: bad size %dx%d (1..16384)", who, s->height, s->width);
    if (!bgr && ((s->width & 1) || (is420 && (s->height & 1))))
        return ppn::fail(PPN_E_INVALID, "%s: odd size %dx%d", who, s->height, s->width);
    const int64_t row = bgr ? 3 * (int64_t)s->width : is420 ? s->width : 2 * (int64_t)s->width;
    const int64_t row_c = fmt == PPN_PIX_NV12 ? s->width : s->width / 2;
    if (s->pitch < row || (is420 && s->pitch_c < row_c))
        return ppn::fail(PPN_E_INVALID, "%s: pitch %d / %d below the row's %lld / %lld bytes", who, s->pitch, s->pitch_c,
                         (long long)row, (long long)row_c);
    const int64_t plane = (int64_t)(s->height - 1) * s->pitch + row;
    const int64_t plane_c = is420 ? (int64_t)(s->height / 2 - 1) * s->pitch_c + row_c : 0;
    if (s->frame_stride < plane || s->frame_stride < plane_c)
        return ppn::fail(PPN_E_INVALID, "%s: frame_stride %lld smaller than a plane (%lld bytes)", who,
                         (long long)s->frame_stride, (long long)(plane > plane_c ? plane : plane_c));
    return PPN_OK;
}

// ---- the gallery ----------------------------------------------------------------------------------------------------------
constexpr int SLOTS = PPN_REID_SLOTS, PER_LANE = SLOTS / WAVE;
static_assert(PER_LANE == 2, "lane i owns entries i and i + 64");

struct ReidArgs {
    ppn_reid_cfg c;
    ppn_reid_state st;
    const int* count;               // [B]
    const int* ids;                 // [B][M]
    const unsigned short* descr;    // [B][R][72]
    const int* valid;               // [B][R]
    const int* n_frames;            // [S] or NULL
    int* out_pid;                   // [B][M]
    int* out_sim;                   // [B][M]
    int* out_live;                  // [B]
    int F, M;
};

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// One entry's descriptor takes the person's in: the first one as it is, a later one blended (rule 1).
__device__ __forceinline__ void take_descr(unsigned short (*g)[SLOTS], int e, const unsigned short* d, int& n, int shift) {
    const int keep = (1 << shift) - 1, half = (1 << shift) >> 1;
    for (int k = 0; k < LEN; ++k) {
        const int nw = d[k];
        g[k][e] = (unsigned short)(n == 0 ? nw : (g[k][e] * keep + nw + half) >> shift);
    }
    n = min(n + 1, 65535);
}

__global__ __launch_bounds__(WAVE) void reid_update_kernel(ReidArgs a) {
    __shared__ unsigned short s_g[LEN][SLOTS];          // the stream's descriptors, [count][entry]
    __shared__ unsigned short s_d[LEN];                 // the newcomer's descriptor
    __shared__ int s_part[PPN_MATCH_MAX_PEOPLE];        // per person of the frame: the id it takes part with, 0: it does not,
    __shared__ int s_held[PPN_MATCH_MAX_PEOPLE];        // whether a live entry holds that id,
    __shared__ int s_opid[PPN_MATCH_MAX_PEOPLE];        // out_pid
    __shared__ int s_osim[PPN_MATCH_MAX_PEOPLE];        // and out_sim
    __shared__ int s_born_p[SLOTS], s_born_id[SLOTS];   // the first 128 newcomers of the births step, ascending p
    const int M = a.M, F = a.F, R = a.c.max_rois;
    const int s = blockIdx.x, lane = threadIdx.x;
    int nF = F;
    if (a.n_frames) nF = __builtin_amdgcn_readfirstlane(min(max(a.n_frames[s], 0), F));

    for (int t = nF; t < F; ++t) {                                  // frames that are not processed
        const size_t b = (size_t)s * F + t;
        for (int p = lane; p < M; p += WAVE) a.out_pid[b * M + p] = -1, a.out_sim[b * M + p] = -1;
        if (lane == 0) a.out_live[b] = -1;
    }
    if (nF == 0) return;                                            // (uniform) the state stays untouched

    int pid[PER_LANE], tid[PER_LANE], lost[PER_LANE], n[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        const size_t e = (size_t)s * SLOTS + k * WAVE + lane;
        pid[k] = a.st.pid[e], tid[k] = a.st.tid[e], lost[k] = a.st.lost[e], n[k] = a.st.n[e];
    }
    const unsigned short* g_in = a.st.descr + (size_t)s * SLOTS * LEN;
    for (int i = lane; i < SLOTS * LEN; i += WAVE) s_g[i % LEN][i / LEN] = g_in[i];
    int last_pid = a.st.last_pid[s], flags = 0;
    __syncthreads();

    for (int t = 0; t < nF; ++t) {
        const size_t b = (size_t)s * F + t;
        const int P = __builtin_amdgcn_readfirstlane(min(max(a.count[b], 0), M));
        const int PD = min(P, R);                                   // people that can have a descriptor
        const unsigned short* dsc = a.descr + b * (size_t)R * LEN;
        for (int p = lane; p < P; p += WAVE) {
            const int id = a.ids[b * M + p];
            s_part[p] = id > 0 ? id : 0;
            s_held[p] = 0, s_opid[p] = -1, s_osim[p] = -1;
        }
        __syncthreads();

        // ---- bound (step 1): every lane walks the participants for its two tids
        bool touched[PER_LANE];
        int my_p[PER_LANE];
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) touched[k] = false, my_p[k] = -1;
        for (int p = 0; p < P; ++p) {                               // (uniform) a broadcast read per person
            const int v = s_part[p];
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                if (v > 0 && pid[k] != 0 && tid[k] == v) {
                    s_held[p] = 1;
                    if (my_p[k] < 0) my_p[k] = p;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            if (my_p[k] >= 0) {
                touched[k] = true, lost[k] = 0;
                s_opid[my_p[k]] = pid[k];
                if (my_p[k] < PD && a.valid[b * R + my_p[k]] != 0)
                    take_descr(s_g, k * WAVE + lane, dsc + (size_t)my_p[k] * LEN, n[k], a.c.shift);
            }
        }
        __syncthreads();

        // ---- relink (step 2): the unheld participants with a descriptor, one by one
        for (int p = 0; p < PD; ++p) {                              // (uniform)
            const int id = __builtin_amdgcn_readfirstlane(s_part[p]);
            if (__builtin_amdgcn_readfirstlane((int)(id == 0 || s_held[p] || a.valid[b * R + p] == 0))) continue;
            for (int k = lane; k < LEN; k += WAVE) s_d[k] = dsc[(size_t)p * LEN + k];
            __syncthreads();
            bool cand[PER_LANE];
            int sim[PER_LANE];
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                cand[k] = pid[k] != 0 && !touched[k] && n[k] > 0 && lost[k] >= a.c.min_lost && lost[k] <= a.c.memory;
                sim[k] = 0;
            }
            for (int c = 0; c < LEN; ++c) {
                const int d = s_d[c];
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) sim[k] += min((int)s_g[c][k * WAVE + lane], d);
            }
            unsigned long long key = 0;                             // larger wins: similarity, then small lost, then low index
#pragma unroll
            for (int k = 0; k < PER_LANE; ++k) {
                const unsigned long long mine = 1ull << 62 | (unsigned long long)sim[k] << 40 |
                                                (unsigned long long)(0x7fffffff - lost[k]) << 8 |
                                                (unsigned long long)(255 - (k * WAVE + lane));
                if (cand[k] && mine > key) key = mine;
            }
            key = wave_max(key);
            const int best = 255 - (int)(key & 255u), best_sim = (int)(key >> 40 & 0x3fffu);
            if (key != 0 && best_sim >= a.c.thr) {                  // (uniform)
#pragma unroll
                for (int k = 0; k < PER_LANE; ++k) {
                    if (best == k * WAVE + lane) {
                        touched[k] = true, tid[k] = id, lost[k] = 0;
                        take_descr(s_g, best, s_d, n[k], a.c.shift);
                        s_opid[p] = pid[k], s_osim[p] = best_sim;
                    }
                }
            }
            __syncthreads();                                        // s_d is rewritten; s_opid is read in the births step
        }

        // ---- age (step 3)
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            if (pid[k] != 0 && !touched[k]) {
                if (lost[k] >= a.c.memory) pid[k] = tid[k] = lost[k] = n[k] = 0;
                else lost[k] += 1;
            }
        }

        // ---- births (step 4): the r-th newcomer takes the r-th free entry
        int n_new = 0;                                              // (uniform)
        for (int c0 = 0; c0 < P; c0 += WAVE) {
            const int p = c0 + lane;
            const bool fresh = p < P && s_part[p] > 0 && !s_held[p] && s_opid[p] < 0;
            const unsigned long long m = __ballot(fresh);
            const int r = n_new + __popcll(m & ((1ull << lane) - 1ull));
            if (fresh && r < SLOTS) s_born_p[r] = p, s_born_id[r] = s_part[p];
            n_new += __popcll(m);
        }
        __syncthreads();
        const unsigned long long free0 = __ballot(pid[0] == 0), free1 = __ballot(pid[1] == 0);
        const int n_free = __popcll(free0) + __popcll(free1);
        const int n_born = min(n_new, n_free);
        if (n_new > n_free) flags |= PPN_REID_FLAG_SLOT_OVERFLOW;
        const unsigned long long below = (1ull << lane) - 1ull;
        const int rank[PER_LANE] = {(int)__popcll(free0 & below), (int)(__popcll(free0) + __popcll(free1 & below))};
#pragma unroll
        for (int k = 0; k < PER_LANE; ++k) {
            if (pid[k] == 0 && rank[k] < n_born) {
                const int p = s_born_p[rank[k]];
                pid[k] = last_pid + rank[k] + 1, tid[k] = s_born_id[rank[k]], lost[k] = 0, n[k] = 0;
                if (p < PD && a.valid[b * R + p] != 0) take_descr(s_g, k * WAVE + lane, dsc + (size_t)p * LEN, n[k], a.c.shift);
                s_opid[p] = pid[k];
            }
        }
        last_pid += n_born;
        const int live = __popcll(__ballot(pid[0] != 0)) + __popcll(__ballot(pid[1] != 0));
        __syncthreads();

        // ---- outputs (step 5)
        for (int p = lane; p < M; p += WAVE) {
            a.out_pid[b * M + p] = p < P ? s_opid[p] : -1;
            a.out_sim[b * M + p] = p < P ? s_osim[p] : -1;
        }
        if (lane == 0) a.out_live[b] = live;
        __syncthreads();                                            // the next frame rewrites the people's arrays
    }

#pragma unroll
    for (int k = 0; k < PER_LANE; ++k) {
        const size_t e = (size_t)s * SLOTS + k * WAVE + lane;
        a.st.pid[e] = pid[k], a.st.tid[e] = tid[k], a.st.lost[e] = lost[k], a.st.n[e] = n[k];
    }
    unsigned short* g_out = a.st.descr + (size_t)s * SLOTS * LEN;
    for (int i = lane; i < SLOTS * LEN; i += WAVE) g_out[i] = s_g[i % LEN][i / LEN];
    if (lane == 0) {
        a.st.last_pid[s] = last_pid;
        if (flags) a.st.flags[s] |= flags;                          // this workgroup owns the word: no atomic
    }
}

}  // namespace

extern "C" int ppn_people_descr(const ppn_yuv_surface* src, int32_t frames, const int32_t* roi, const int32_t* status,
                                int32_t max_rois, uint16_t* descr, int32_t* valid, void* stream) {
    static const char who[] = "ppn_people_descr";
    if (int rc = check_surface(who, src)) return rc;
    if (!roi || !status || !descr || !valid) return ppn::fail(PPN_E_INVALID, "%s: NULL roi, status, descr or valid", who);
    if (max_rois < 1 || frames < 1 || (int64_t)frames * max_rois > 65535)
        return ppn::fail(PPN_E_INVALID, "%s: %d frames x %d rois: at least one each, at most 65535 slots", who, frames, max_rois);
    const bool is420 = src->format == PPN_PIX_NV12 || src->format == PPN_PIX_I420;
    DescrArgs a{static_cast<const unsigned char*>(src->y), is420 ? static_cast<const unsigned char*>(src->u) : nullptr,
                src->format == PPN_PIX_I420 ? static_cast<const unsigned char*>(src->v) : nullptr, src->frame_stride,
                src->pitch, is420 ? src->pitch_c : 0, src->height, src->width, roi, status, descr, valid, max_rois};
    const unsigned grid = (unsigned)(frames * max_rois);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (src->format == PPN_PIX_NV12) people_descr_kernel<PPN_PIX_NV12><<<grid, DESCR_THREADS, 0, st>>>(a);
    else if (src->format == PPN_PIX_I420) people_descr_kernel<PPN_PIX_I420><<<grid, DESCR_THREADS, 0, st>>>(a);
    else if (src->format == PPN_PIX_YUYV) people_descr_kernel<PPN_PIX_YUYV><<<grid, DESCR_THREADS, 0, st>>>(a);
    else people_descr_kernel<PPN_PIX_BGR24><<<grid, DESCR_THREADS, 0, st>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_reid_update(const ppn_reid_cfg* cfg, const ppn_reid_state* st, const int32_t* count, const int32_t* ids,
                               const uint16_t* descr, const int32_t* valid, int32_t streams, int32_t frames,
                               int32_t max_humans, const int32_t* n_frames, int32_t* out_pid, int32_t* out_sim,
                               int32_t* out_live, void* stream) {
    const char* fn = "ppn_reid_update";
    if (!cfg || !st) return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", fn);
    if (!st->pid || !st->tid || !st->lost || !st->n || !st->descr || !st->last_pid || !st->flags)
        return ppn::fail(PPN_E_INVALID, "%s: NULL state pointer", fn);
    if (cfg->thr < 0 || cfg->thr > PPN_REID_SIM_MAX)
        return ppn::fail(PPN_E_INVALID, "%s: thr %d outside 0..%d", fn, cfg->thr, PPN_REID_SIM_MAX);
    if (cfg->min_lost < 1) return ppn::fail(PPN_E_INVALID, "%s: min_lost %d must be >= 1", fn, cfg->min_lost);
    if (cfg->memory < 0) return ppn::fail(PPN_E_INVALID, "%s: memory %d must be >= 0", fn, cfg->memory);
    if (cfg->shift < 0 || cfg->shift > 4) return ppn::fail(PPN_E_INVALID, "%s: shift %d outside 0..4", fn, cfg->shift);
    if (cfg->max_rois < 1) return ppn::fail(PPN_E_INVALID, "%s: max_rois %d must be >= 1", fn, cfg->max_rois);
    if (!count || !ids || !descr || !valid || !out_pid || !out_sim || !out_live)
        return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", fn);
    if (streams < 1 || frames < 1 || max_humans < 1)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry (%d streams, %d frames, max_humans %d)", fn, streams, frames,
                         max_humans);
    if (max_humans > PPN_MATCH_MAX_PEOPLE)
        return ppn::fail(PPN_E_UNSUPPORTED, "%s: max_humans %d beyond the limit %d", fn, max_humans, PPN_MATCH_MAX_PEOPLE);
    ReidArgs a{*cfg, *st, count, ids, descr, valid, n_frames, out_pid, out_sim, out_live, frames, max_humans};
    reid_update_kernel<<<(unsigned)streams, WAVE, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
