// PCKh matching of one batch of decoded people against the resident ground truth of a validation set
// (eval_helpers.assignGTmulti as evaluate.assign_gt_multi restates it; contract in include/ppn.h, NumPy restatement
// tests/validate_ref.py).
//
//   pckh_match_kernel    one workgroup of four waves per batch image.  Lane g of every wave keeps ground-truth person g's 17
//                        joints and head size in registers (PPN_MATCH_MAX_GT = 64 = one wave).  Wave w takes the people
//                        p = w, w + 4, ..: lanes 0..16 load the person's joints, every lane builds the 17-bit match mask of
//                        (p, g) and counts it, a wave max over (count, -g) gives best_gt[p] -- the first g of the largest
//                        count -- and its mask; one packed word per person goes to LDS and an integer LDS max over
//                        (count, -p) elects, per g, the first p of the largest count among the p whose best_gt is g.  After
//                        one barrier all threads write the rows: the person's scores, and the mask of the winners.
// The distance is dx = gx - px, dy = gy - py, dx*dx, dy*dy, their sum, sqrtf, a division by the head size and a comparison
// with the threshold, every step rounded to f32 on its own: the file is built with -ffp-contract=off and IEEE sqrt / divide.
// Integer maxima only: the result does not depend on which wave comes first.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int JOINTS = PPN_MATCH_JOINTS;             // 17; keypoint k = joint + 1, keypoint 0 is the instance
constexpr int KP = JOINTS + 1;
static_assert(PPN_MATCH_MAX_GT == WAVE, "one lane per ground-truth person");
static_assert(PPN_MATCH_MAX_PEOPLE <= 1024, "the election key keeps p in 10 bits");

struct MatchArgs {
    const int* count;            // [B]
    const int* kp_cell;          // [B][M][18]
    const float* bbox;           // [B][M][18][4] ymin, xmin, ymax, xmax
    const float* score;          // [B][M][18]
    const float* gt_xy;          // [N][gmax][17][2] x, y
    const float* gt_head;        // [N][gmax]
    const int* gt_count;         // [N]
    const int* image_index;      // [B]
    float* rec_score;            // [N][M][17]
    unsigned char* rec_label;    // [N][M][17]
    int* rec_count;              // [N]
    int* flags;
    int B, M, N, gmax;
    float thresh;
};

__global__ __launch_bounds__(THREADS) void pckh_match_kernel(MatchArgs a) {
    __shared__ unsigned person[PPN_MATCH_MAX_PEOPLE];    // best_gt | count << 6 | mask << 11
    __shared__ int winner[WAVE];                         // per g: count << 10 | (1023 - p) of the claiming person, 0: nobody
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const int n = a.image_index[b];
    if (n == -1) return;                                 // padding image of a ragged batch: nothing is written
    if (n < -1 || n >= a.N) {
        if (tid == 0) atomicOr(a.flags, PPN_MATCH_FLAG_INDEX);
        return;
    }
    const int G = a.gt_count[n];
    if (G < 0 || G > a.gmax) {
        if (tid == 0) atomicOr(a.flags, PPN_MATCH_FLAG_GT_COUNT);
        return;
    }
    const int P = min(max(a.count[b], 0), a.M);
    if (tid == 0) a.rec_count[n] = G > 0 ? P : 0;
    if (G == 0 || P == 0) return;                        // (uniform over the workgroup: no barrier is skipped by a part of it)

    float gx[JOINTS], gy[JOINTS], head = 0.f;
    const bool has_gt = lane < G;
#pragma unroll
    for (int j = 0; j < JOINTS; ++j) gx[j] = gy[j] = 0.f;
    if (has_gt) {
        const float2* g2 = reinterpret_cast<const float2*>(a.gt_xy) + ((size_t)n * a.gmax + lane) * JOINTS;
#pragma unroll
        for (int j = 0; j < JOINTS; ++j) {
            const float2 v = g2[j];
            gx[j] = v.x;
            gy[j] = v.y;
        }
        head = a.gt_head[(size_t)n * a.gmax + lane];
    }
    if (tid < WAVE) winner[tid] = 0;
    __syncthreads();

    for (int p = wave; p < P; p += THREADS / WAVE) {     // uniform per wave
        const size_t row = ((size_t)b * a.M + p) * KP;
        float x = 0.f, y = 0.f;                          // a missing joint is the point (0, 0)
        if (lane < JOINTS && a.kp_cell[row + lane + 1] >= 0) {
            const float4 bb = reinterpret_cast<const float4*>(a.bbox)[row + lane + 1];
            x = (bb.y + bb.w) / 2.f;
            y = (bb.x + bb.z) / 2.f;
        }
        unsigned mask = 0;
#pragma unroll
        for (int j = 0; j < JOINTS; ++j) {
            const float px = __shfl(x, j, WAVE), py = __shfl(y, j, WAVE);
            const float dx = gx[j] - px, dy = gy[j] - py;
            const float xx = dx * dx, yy = dy * dy;
            const float d = sqrtf(xx + yy) / head;
            mask |= (d <= a.thresh ? 1u : 0u) << j;      // false for a NaN (0 / 0) and for +inf (head size 0)
        }
        if (!has_gt) mask = 0;
        const int cnt = __popc(mask);
        int key = has_gt ? cnt << 6 | (WAVE - 1 - lane) : -1;      // larger count first, then the smaller g
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off, WAVE));
        const int best_g = WAVE - 1 - (key & (WAVE - 1)), best_cnt = key >> 6;
        const unsigned best_mask = (unsigned)__shfl((int)mask, best_g, WAVE);
        if (lane == 0) {
            person[p] = (unsigned)best_g | (unsigned)best_cnt << 6 | best_mask << 11;
            if (best_cnt > 0) atomicMax(&winner[best_g], best_cnt << 10 | (1023 - p));   // larger count, then the smaller p
        }
    }
    __syncthreads();

    for (int i = tid; i < P * JOINTS; i += THREADS) {
        const int p = i / JOINTS, j = i % JOINTS;
        const size_t src = ((size_t)b * a.M + p) * KP + j + 1;
        const size_t dst = ((size_t)n * a.M + p) * JOINTS + j;
        const unsigned w = person[p];
        const int g = w & (WAVE - 1), cnt = w >> 6 & 31;
        const bool claimed = cnt > 0 && winner[g] == (cnt << 10 | (1023 - p));
        a.rec_score[dst] = a.kp_cell[src] >= 0 ? a.score[src] : 0.f;
        a.rec_label[dst] = claimed ? (unsigned char)(w >> (11 + j) & 1u) : (unsigned char)0;
    }
}

}  // namespace

extern "C" int ppn_pckh_match(const int32_t* count, const int32_t* kp_cell, const float* bbox, const float* score,
                              int32_t batch, int32_t max_humans, const float* gt_xy, const float* gt_head,
                              const int32_t* gt_count, int32_t n_images, int32_t gmax, const int32_t* image_index,
                              float dist_thresh, float* rec_score, uint8_t* rec_label, int32_t* rec_count, int32_t* flags,
                              void* stream) {
    if (!count || !kp_cell || !bbox || !score || !gt_xy || !gt_head || !gt_count || !image_index || !rec_score ||
        !rec_label || !rec_count || !flags)
        return ppn::fail(PPN_E_INVALID, "ppn_pckh_match: NULL pointer");
    if (batch < 1 || max_humans < 1 || n_images < 1 || gmax < 1)
        return ppn::fail(PPN_E_INVALID, "ppn_pckh_match: bad geometry (batch %d, max_humans %d, %d images, gmax %d)", batch,
                         max_humans, n_images, gmax);
    if (gmax > PPN_MATCH_MAX_GT || max_humans > PPN_MATCH_MAX_PEOPLE)
        return ppn::fail(PPN_E_UNSUPPORTED, "ppn_pckh_match: gmax %d / max_humans %d beyond the limits %d / %d", gmax,
                         max_humans, PPN_MATCH_MAX_GT, PPN_MATCH_MAX_PEOPLE);
    if (!(dist_thresh == dist_thresh))
        return ppn::fail(PPN_E_INVALID, "ppn_pckh_match: dist_thresh is not a number");
    if (reinterpret_cast<uintptr_t>(bbox) % 16 || reinterpret_cast<uintptr_t>(gt_xy) % 8)
        return ppn::fail(PPN_E_INVALID, "ppn_pckh_match: bbox must be 16-byte and gt_xy 8-byte aligned");
    MatchArgs a{count, kp_cell, bbox, score, gt_xy, gt_head, gt_count, image_index, rec_score, rec_label, rec_count, flags,
                batch, max_humans, n_images, gmax, dist_thresh};
    pckh_match_kernel<<<(unsigned)batch, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
