// Joining the people of overlapping windows of one frame (contract in include/ppn.h, ppn_merge_windows; NumPy restatement
// tests/windows_ref.py): map every person of the F * n window images to frame pixels, drop the duplicates the overlaps
// produce and let a kept person take the better keypoints of its duplicates.
//
//   merge_kernel   one workgroup of four waves per frame, everything of the frame in 60 KB of LDS:
//     collect  an ordered compaction over (window, person): ballots and popcounts give every candidate its (i, p) rank;
//              the first 512 leave a 64-bit key (order-preserving score bits, then the inverted rank) and their id
//     sort     a counting sort: candidate c's place is the number of larger keys (the keys differ, 512 broadcast LDS reads
//              per candidate); its root box is loaded, mapped and stored at that place with area, id and window
//     pairs    the bit matrix [512][8 words]: bit j of row i (j < i) = other window && iou >= merge_thr, one 64-bit word
//              per work item, consecutive lanes on consecutive rows of one word (box j is an LDS broadcast)
//     walk     decode.hip's greedy_resolve: the first wave, 64 candidates at a time, the chunk's own 64 x 64 block on
//              scalar registers; a kept candidate never has a kept partner, a duplicate suppresses nobody
//     keepers  per duplicate the first kept partner: the lowest set bit of row & kept bits
//     members  per kept person the bit row of its members (itself and its duplicates), written over its pair row
//     fuse     one work item per (output person, keypoint) walks the member bits in order and keeps the strictly larger
//              score; the winner's box is mapped and stored
// Integer and bitwise reductions only, no atomics, plain vector stores.  The file is built with -ffp-contract=off and IEEE
// division: y * sy + y0 stays a multiply and an add, the IoU is track.hip's operation for operation.
#include "common.h"
#include "windows.h"

#include <cmath>

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int CAP = PPN_MERGE_MAX_CAND;
constexpr int WORDS = CAP / WAVE;            // 64-bit words of a bit row
constexpr int STRIDE = WORDS + 1;            // row stride in words: 72 bytes, consecutive rows on different banks
static_assert(CAP % WAVE == 0 && WORDS <= WAVE, "lane w of the walking wave keeps the kept bits of chunk w");

struct MergeArgs {
    ppn_merge_cfg c;
    ppn_window_layout lay;
    const int* count;            // [F * n]
    const int* kp_cell;          // [F * n][M][K]
    const float* bbox;           // [F * n][M][K][4] ymin, xmin, ymax, xmax in network pixels of the image
    const float* score;          // [F * n][M][K]
    int* out_count;              // [F]
    int* out_src;                // [F][max_out][K]
    float* out_bbox;             // [F][max_out][K][4] frame pixels
    float* out_score;            // [F][max_out][K]
    int* out_flags;              // [F]
};

__device__ __forceinline__ float box_area(const float4& b) { return (b.z - b.x) * (b.w - b.y); }

// track.hip's iou_of: a value that is not > 0 (NaN included) is 0
__device__ __forceinline__ float iou_of(const float4& bi, float ai, const float4& bj, float aj) {
    const float tl0 = fmaxf(bi.x, bj.x), tl1 = fmaxf(bi.y, bj.y);
    const float br0 = fminf(bi.z, bj.z), br1 = fminf(bi.w, bj.w);
    const float inter = ((br0 - tl0) * (br1 - tl1)) * ((tl0 < br0 && tl1 < br1) ? 1.0f : 0.0f);
    const float iou = inter / ((ai + aj) - inter);
    return iou > 0.0f ? iou : 0.0f;
}

// Window i's map from network pixels of its image to frame pixels: Y = y * sy + y0, X = x * sx + x0.
struct WinMap {
    float sy, sx, y0, x0;
};

__device__ __forceinline__ WinMap win_map(const ppn_window& w, int inH, int inW) {
    return {(float)w.h / (float)inH, (float)w.w / (float)inW, (float)w.y0, (float)w.x0};
}

__device__ __forceinline__ float4 map_box(const float4& b, const WinMap& m) {
    const float y0 = b.x * m.sy, x0 = b.y * m.sx, y1 = b.z * m.sy, x1 = b.w * m.sx;
    return make_float4(y0 + m.y0, x0 + m.x0, y1 + m.y0, x1 + m.x0);
}

// Unsigned bits that order as the f32 values do (no NaN reaches this; -0.0 and +0.0 are one value).
__device__ __forceinline__ unsigned score_bits(float s) {
    const unsigned u = s == 0.0f ? 0u : __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(THREADS) void merge_kernel(MergeArgs a) {
    __shared__ unsigned long long s_key[CAP];              // collect order: score bits << 32 | ~rank
    __shared__ int s_usrc[CAP];                            // collect order: i * M + p
    __shared__ __attribute__((aligned(16))) float4 s_box[CAP];   // from here on in walk order: mapped root box
    __shared__ float s_area[CAP];
    __shared__ int s_src[CAP];                             // i * M + p
    __shared__ int s_win[CAP];                             // i
    __shared__ unsigned long long s_mask[CAP * STRIDE];    // pair bits; rows of kept candidates later hold member bits
    __shared__ int s_keeper[CAP];                          // the kept candidate this one belongs to (itself when kept)
    __shared__ int s_sel[CAP];                             // the kept candidates, in order
    __shared__ unsigned long long s_keepw[WORDS];          // kept bits
    __shared__ int s_wcnt[THREADS / WAVE];
    __shared__ int s_nsel;

    const int f = blockIdx.x, t = threadIdx.x, lane = t % WAVE, wid = t / WAVE;
    const int n = a.lay.n, M = a.c.max_humans, K = a.c.K;

    // ---- collect (rule 1).  `total` is uniform; the walk over the windows stops once the overflow is known.
    int total = 0;
    for (int i = 0; i < n && total <= CAP; ++i) {
        const size_t img = (size_t)f * n + i;
        const int P = min(max(a.count[img], 0), M);
        for (int base = 0; base < P && total <= CAP; base += THREADS) {
            const int p = base + t;
            bool ok = false;
            float sc = 0.f;
            if (p < P) {
                const size_t r = (img * M + p) * K;
                sc = a.score[r];
                ok = a.kp_cell[r] >= 0 && sc == sc;
            }
            const unsigned long long m = __ballot(ok);
            if (lane == 0) s_wcnt[wid] = __popcll(m);
            __syncthreads();
            int pos = total + __popcll(m & ((1ull << lane) - 1ull));
            for (int w = 0; w < THREADS / WAVE; ++w) {
                const int c = s_wcnt[w];
                if (w < wid) pos += c;
                total += c;
            }
            if (ok && pos < CAP) {
                s_key[pos] = (unsigned long long)score_bits(sc) << 32 | (0xFFFFFFFFu - (unsigned)pos);
                s_usrc[pos] = i * M + p;
            }
            __syncthreads();                                                      // s_wcnt is rewritten by the next chunk
        }
    }
    const int nc = min(total, CAP);
    int flags = total > CAP ? PPN_MERGE_FLAG_CAND_OVERFLOW : 0;

    // ---- sort (rule 3) and stage (rule 2): the place of a candidate is the number of larger keys
    for (int c = t; c < nc; c += THREADS) {
        const unsigned long long key = s_key[c];
        int rank = 0;
        for (int j = 0; j < nc; ++j) rank += s_key[j] > key ? 1 : 0;
        const int src = s_usrc[c];
        const int i = src / M, p = src - i * M;
        const WinMap wm = win_map(a.lay.win[i], a.c.inH, a.c.inW);
        const float4 b = map_box(reinterpret_cast<const float4*>(a.bbox)[(((size_t)f * n + i) * M + p) * K], wm);
        s_box[rank] = b;
        s_area[rank] = box_area(b);
        s_src[rank] = src;
        s_win[rank] = i;
    }
    __syncthreads();

    // ---- pairs (rule 4): row i, word w holds the partners j in [64 w, min(64 w + 64, i))
    const int nw = (nc + WAVE - 1) / WAVE;
    for (int q = t; q < nc * nw; q += THREADS) {
        const int w = q / nc, i = q - w * nc;
        const int j0 = w * WAVE, j1 = min(j0 + WAVE, i);
        unsigned long long bits = 0ull;
        if (j0 < j1) {
            const float4 bi = s_box[i];
            const float ai = s_area[i];
            const int wi = s_win[i];
#pragma unroll 4
            for (int j = j0; j < j1; ++j) {
                const bool dup = s_win[j] != wi && iou_of(s_box[j], s_area[j], bi, ai) >= a.c.merge_thr;
                bits |= dup ? 1ull << (j - j0) : 0ull;
            }
        }
        s_mask[i * STRIDE + w] = bits;
    }
    __syncthreads();

    // ---- walk: the first wave, 64 candidates (one per lane) at a time.  A lane drops out if a kept candidate of an
    // earlier chunk is its partner; inside the chunk the dependence is sequential and runs on scalar registers.
    if (t < WAVE) {
        unsigned long long keep_w = 0ull;                                         // lane w: kept bits of chunk w
        int nsel = 0;
        for (int cidx = 0; cidx < nw; ++cidx) {
            const int i = cidx * WAVE + t;
            const bool valid = i < nc;
            bool alive = valid;
            const unsigned long long* rowp = s_mask + (valid ? i : 0) * STRIDE;
            const unsigned long long intra = valid ? rowp[cidx] : 0ull;
            for (int w = 0; w < cidx; ++w) {
                const unsigned long long kw = __shfl(keep_w, w);                  // executed by all 64 lanes
                if (valid && (rowp[w] & kw)) alive = false;
            }
            const unsigned long long cand = __ballot(alive);
            unsigned long long keepc = 0ull;
            const unsigned lo = (unsigned)intra, hi = (unsigned)(intra >> 32);
            for (int bpos = 0; bpos < WAVE; ++bpos) {
                if ((cand >> bpos) & 1ull) {
                    const unsigned long long row = ((unsigned long long)__builtin_amdgcn_readlane(hi, bpos) << 32) |
                                                   (unsigned)__builtin_amdgcn_readlane(lo, bpos);
                    if ((row & keepc) == 0ull) keepc |= 1ull << bpos;
                }
            }
            if ((keepc >> t) & 1ull) s_sel[nsel + __popcll(keepc & ((1ull << t) - 1ull))] = i;
            if (t == cidx) keep_w = keepc;
            nsel += __popcll(keepc);
        }
        if (t < WORDS) s_keepw[t] = keep_w;
        if (t == 0) s_nsel = nsel;
    }
    __syncthreads();

    const int nsel = s_nsel;
    const int R = min(nsel, a.c.max_out);                                         // output rows of the frame
    if (nsel > a.c.max_out) flags |= PPN_MERGE_FLAG_OUT_OVERFLOW;
    if (t == 0) {
        a.out_count[f] = nsel;
        a.out_flags[f] = flags;
    }

    if (a.c.fuse) {
        // ---- keepers: the first kept partner of a duplicate
        for (int c = t; c < nc; c += THREADS) {
            int k = c;
            if (!((s_keepw[c / WAVE] >> (c % WAVE)) & 1ull)) {
                for (int w = 0; w <= c / WAVE; ++w) {
                    const unsigned long long m = s_mask[c * STRIDE + w] & s_keepw[w];
                    if (m) {
                        k = w * WAVE + __ffsll(m) - 1;
                        break;
                    }
                }
            }
            s_keeper[c] = k;
        }
        __syncthreads();
        // ---- members: row k, word w = the candidates of [64 w, 64 w + 64) that belong to k (k itself included)
        for (int q = t; q < R * nw; q += THREADS) {
            const int w = q / R, k = s_sel[q - w * R];
            const int c0 = w * WAVE, c1 = min(c0 + WAVE, nc);
            unsigned long long bits = 0ull;
            for (int c = c0; c < c1; ++c) bits |= s_keeper[c] == k ? 1ull << (c - c0) : 0ull;
            s_mask[k * STRIDE + w] = bits;
        }
        __syncthreads();
    }

    // ---- fuse and write (rules 5 and 6): one work item per (output person, keypoint)
    for (int q = t; q < R * K; q += THREADS) {
        const int r = q / K, j = q - r * K;
        const int k = s_sel[r];
        int best = -1;
        float bs = 0.f;
        size_t brow = 0;
        if (j == 0 || !a.c.fuse) {
            const size_t row = (((size_t)f * n + s_win[k]) * M + (s_src[k] - s_win[k] * M)) * K + j;
            if (a.kp_cell[row] >= 0) {
                best = k;
                bs = a.score[row];
                brow = row;
            }
        } else {
            for (int w = k / WAVE; w < nw; ++w) {
                unsigned long long m = s_mask[k * STRIDE + w];
                while (m) {
                    const int c = w * WAVE + __ffsll(m) - 1;
                    m &= m - 1ull;
                    const size_t row = (((size_t)f * n + s_win[c]) * M + (s_src[c] - s_win[c] * M)) * K + j;
                    if (a.kp_cell[row] >= 0) {
                        const float s = a.score[row];
                        if (best < 0 || s > bs) {
                            best = c;
                            bs = s;
                            brow = row;
                        }
                    }
                }
            }
        }
        const size_t o = ((size_t)f * a.c.max_out + r) * K + j;
        float4 ob = make_float4(0.f, 0.f, 0.f, 0.f);
        if (best >= 0)
            ob = map_box(reinterpret_cast<const float4*>(a.bbox)[brow], win_map(a.lay.win[s_win[best]], a.c.inH, a.c.inW));
        a.out_src[o] = best >= 0 ? s_src[best] : -1;
        reinterpret_cast<float4*>(a.out_bbox)[o] = ob;
        a.out_score[o] = best >= 0 ? bs : 0.f;
    }
}

}  // namespace

extern "C" int ppn_merge_windows(const ppn_merge_cfg* cfg, const ppn_window_layout* lay, const int32_t* count,
                                 const int32_t* kp_cell, const float* bbox, const float* score, int32_t frames,
                                 int32_t* out_count, int32_t* out_src, float* out_bbox, float* out_score, int32_t* out_flags,
                                 void* stream) {
    static const char who[] = "ppn_merge_windows";
    if (!cfg || !count || !kp_cell || !bbox || !score || !out_count || !out_src || !out_bbox || !out_score || !out_flags)
        return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", who);
    if (const int rc = ppn::check_layout(who, lay)) return rc;
    if (cfg->K < 1 || cfg->K > PPN_MAX_KP) return ppn::fail(PPN_E_INVALID, "%s: K %d outside 1..%d", who, cfg->K, PPN_MAX_KP);
    if (cfg->inH < 1 || cfg->inW < 1 || cfg->max_out < 1 || cfg->max_humans < 1 || cfg->max_humans > PPN_MATCH_MAX_PEOPLE ||
        frames < 1)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry (%d frames, input %dx%d, max_humans %d outside 1..%d, max_out %d)",
                         who, frames, cfg->inH, cfg->inW, cfg->max_humans, PPN_MATCH_MAX_PEOPLE, cfg->max_out);
    if (std::isnan(cfg->merge_thr)) return ppn::fail(PPN_E_INVALID, "%s: merge_thr is NaN", who);
    if (reinterpret_cast<uintptr_t>(bbox) % 16 || reinterpret_cast<uintptr_t>(out_bbox) % 16)
        return ppn::fail(PPN_E_INVALID, "%s: bbox and out_bbox must be 16-byte aligned", who);
    const MergeArgs a{*cfg, *lay, count, kp_cell, bbox, score, out_count, out_src, out_bbox, out_score, out_flags};
    merge_kernel<<<(unsigned)frames, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
