// ST-GCN forward for one person per clip, exact f32 (contract in include/ppn.h, ppn_stgcn_*; restatement from the unfolded
// state dict in tests/stgcn_ref.py).  Activations between the stages are f32 [n][t][v][c], channels last, for the n active
// clips only; every kernel is launched for the capacity S * 64 and reads n from device memory.
//
//   stgcn_input_kernel   one workgroup per slot: the slot's rank among the active slots before it (a count over ids / length,
//                        integers only), the active list, and the clip's planes through data_bn into [t][v][3]
//   stgcn_gcn_kernel     one workgroup of four waves per (clip, tile of TT time steps).  Per chunk of 16 input channels: the
//                        tile's rows into LDS; y[(t, w)][p][ci] = sum_v x[t][v][ci] * A[p][v][w] (the contraction over the
//                        joints first) as small MFMAs D[ci][w] = x^T[ci][v] A[v][w], the units (t, p, 16 columns) dealt to the
//                        waves in turn, into LDS; then z += W x y on v_mfma_f32_16x16x4_f32, the weights as the A operand
//                        straight from global memory (packed on the host in fragment order), y as the B operand from LDS.
//                        Wave w owns the channel tiles w, w + 4, .. of 16 and every row tile (a y fragment is read once for
//                        up to four channel tiles), so a lane ends with four consecutive channels of one row: a 16-byte store
//   stgcn_tcn_kernel     the same row tiling over output time steps, 64 output channels per workgroup (wave w: 16 of them).
//                        Per chunk of 16 channels the input window of the tile ((tt - 1) * stride + 9 time steps, zeros
//                        outside [0, T) of the clip itself) goes to LDS once and serves all nine taps; for a projection shortcut the GEMM goes on over the block input's channels at
//                        t' * stride with weights the host scaled by sr / s3
//   stgcn_head_kernel    one workgroup per slot: mean over (t, v), the fully connected layer, arg-max (lowest index on ties)
// One output element is summed in one fixed order (chunks ascending, inside an MFMA the k order of the instruction), whatever
// else is active: no atomics, no split reductions.  Built without SLP vectorisation like every MFMA file (build.py NOSLP).
#include <climits>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int CH = 16;                       // channels per depth chunk
constexpr int MAXR = 160;                    // rows (t, v) of a tile: 8 x 18 = 144 for the default skeleton
constexpr int MAXRT = MAXR / 16;
constexpr int MAXP = PPN_STGCN_MAX_P;
constexpr int YS = MAXP * CH + 4;            // row pitch of the aggregated tile (floats): 52 = 4 x 13, 16-byte rows, odd in 16 B
constexpr int US = CH + 4;                   // row pitch of the temporal window
constexpr int AP = 32;                       // pitch of the zero-padded adjacency in LDS
constexpr int GCT = PPN_STGCN_MAX_C / 64;    // channel tiles of 16 per wave in the graph convolution
constexpr int WROWS = 544;                   // the largest window: K = 32, TT = 5, stride 2 -> 17 x 32
static_assert(MAXR % 16 == 0 && PPN_MAX_KP <= 32 && PPN_CLIP_SLOTS == 64, "");

__host__ __device__ inline int tile_steps(int K) {          // time steps per tile: TT * K <= MAXR
    const int t = MAXR / K;
    return t > 8 ? 8 : t;
}

__device__ __forceinline__ void mma4(f32x4& acc, const f32x4& a, const f32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// ---- selection and data_bn ---------------------------------------------------------------------------------------------------
struct InputArgs {
    const float* x;
    const int32_t* ids;
    const int32_t* length;
    const float* scale;
    const float* shift;
    int32_t* active;
    int32_t* n_active;
    int32_t* rank;
    float* x0;
    int K, T, min_len;
};

__global__ __launch_bounds__(THREADS) void stgcn_input_kernel(InputArgs a) {
    __shared__ int part[THREADS / WAVE];
    const int b = blockIdx.x, cap = gridDim.x, tid = threadIdx.x;
    int cnt = 0;
    for (int j = tid; j < b; j += THREADS) cnt += (a.ids[j] != 0 && a.length[j] >= a.min_len) ? 1 : 0;
    for (int o = WAVE / 2; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, WAVE);
    if ((tid & (WAVE - 1)) == 0) part[tid / WAVE] = cnt;
    __syncthreads();
    int r = 0;
    for (int i = 0; i < THREADS / WAVE; ++i) r += part[i];
    const bool on = a.ids[b] != 0 && a.length[b] >= a.min_len;
    if (tid == 0) {
        a.rank[b] = on ? r : -1;
        if (on) a.active[r] = b;
        else a.active[cap - 1 - (b - r)] = -1;          // b - r inactive slots lie before b: the tail is filled from the back
        if (b == cap - 1) *a.n_active = r + (on ? 1 : 0);
    }
    if (!on) return;
    const int TK = a.T * a.K;
    const float* src = a.x + (size_t)b * 3 * TK;
    float* dst = a.x0 + (size_t)r * TK * 3;
    for (int i = tid; i < TK * 3; i += THREADS) {
        const int c = i % 3, tv = i / 3, ch = (tv % a.K) * 3 + c;
        dst[i] = fmaf(src[c * TK + tv], a.scale[ch], a.shift[ch]);
    }
}

// ---- graph convolution --------------------------------------------------------------------------------------------------------
struct GcnArgs {
    const float* x;
    const float* w;
    const float* adj;
    const float* s0;
    const float* t0;
    const int32_t* n_active;
    float* out;
    int K, P, T, cin, cout, TT;
};

__global__ __launch_bounds__(THREADS, 2) void stgcn_gcn_kernel(GcnArgs a) {   // two workgroups per CU: <= 256 registers
    __shared__ __attribute__((aligned(16))) float xs[MAXR * CH];
    __shared__ __attribute__((aligned(16))) float ys[MAXR * YS];
    __shared__ float adj[MAXP * AP * AP];                       // [p][v][w], zero beyond K
    const int n = blockIdx.x;
    if (n >= *a.n_active) return;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int col = lane & 15, g = lane >> 4;
    const int K = a.K, P = a.P, cin = a.cin, cout = a.cout;
    const int t0 = blockIdx.y * a.TT;
    const int tt = min(a.TT, a.T - t0), rows = tt * K, rtiles = (rows + 15) >> 4;
    const int myct = (cout / 16 - wave + 3) / 4;                // this wave's tiles of 16 output channels: wave + 4 i
    const int ncc = (cin + CH - 1) / CH;
    const int nsteps = (K + 3) >> 2, ntiles = (K + 15) >> 4;    // the aggregation's depth steps (v) and column tiles (w)
    const size_t row0 = ((size_t)n * a.T + t0) * K;             // first row (t, v) of the tile in x and out

    for (int i = tid; i < P * AP * AP; i += THREADS) {
        const int p = i / (AP * AP), v = (i / AP) % AP, w = i % AP;
        adj[i] = (v < K && w < K) ? a.adj[(p * K + v) * K + w] : 0.f;
    }
    for (int i = tid; i < MAXR * YS; i += THREADS) ys[i] = 0.f;  // the rows past `rows` of the last row tile stay zero

    f32x4 acc[GCT][MAXRT];
#pragma unroll
    for (int i = 0; i < GCT; ++i)
#pragma unroll
        for (int r = 0; r < MAXRT; ++r) acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int cc = 0; cc < ncc; ++cc) {
        __syncthreads();                                        // the MFMAs of the chunk before have read ys
        for (int i = tid; i < rows * CH; i += THREADS) {
            const int r = i >> 4, ci = cc * CH + (i & 15);
            xs[i] = ci < cin ? a.x[(row0 + r) * cin + ci] : 0.f;
        }
        __syncthreads();
        // y[t][w][p][ci] = sum_v x[t][v][ci] adj[p][v][w] as D[ci][w] = A[ci][v] B[v][w]: a lane ends with four consecutive ci
        for (int unit = wave; unit < tt * P * ntiles; unit += THREADS / WAVE) {
            const int nt = unit % ntiles, p = (unit / ntiles) % P, t = unit / (ntiles * P);
            const float* ap = adj + p * AP * AP + nt * 16 + col;
            f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < nsteps; ++s) {
                const int v = 4 * s + g;                        // <= 31; a v past K takes 0, not what lies behind the row
                const float xv = v < K ? xs[(t * K + v) * CH + col] : 0.f;
                d = __builtin_amdgcn_mfma_f32_16x16x4f32(xv, ap[v * AP], d, 0, 0, 0);
            }
            const int w = nt * 16 + col;
            if (w < K) *reinterpret_cast<f32x4*>(ys + (t * K + w) * YS + p * CH + 4 * g) = d;
        }
        __syncthreads();
        if (myct > 0) {
            for (int p = 0; p < P; ++p) {
                f32x4 wf[GCT];
#pragma unroll
                for (int i = 0; i < GCT; ++i)
                    if (i < myct)
                        wf[i] = reinterpret_cast<const f32x4*>(a.w)[((size_t)((wave + 4 * i) * ncc + cc) * P + p) * WAVE + lane];
                const float* yp = ys + col * YS + p * CH + 4 * g;
#pragma unroll
                for (int r = 0; r < MAXRT; ++r) {
                    if (r < rtiles) {
                        const f32x4 yf = *reinterpret_cast<const f32x4*>(yp + r * 16 * YS);
#pragma unroll
                        for (int i = 0; i < GCT; ++i)
                            if (i < myct) mma4(acc[i][r], wf[i], yf);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < GCT; ++i) {
        if (i >= myct) break;
        const int ch = (wave + 4 * i) * 16 + 4 * g;             // D: row = 4 (lane >> 4) + reg is the channel, column the row
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(a.s0 + ch);
#pragma unroll
        for (int r = 0; r < MAXRT; ++r) {
            const int row = r * 16 + col;
            if (r < rtiles && row < rows) {
                const int w = row % K;
                const f32x4 sh = *reinterpret_cast<const f32x4*>(a.t0 + (size_t)w * cout + ch);
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaxf(fmaf(acc[i][r][j], s0[j], sh[j]), 0.f);
                *reinterpret_cast<f32x4*>(a.out + (row0 + row) * cout + ch) = o;
            }
        }
    }
}

// ---- temporal convolution -----------------------------------------------------------------------------------------------------
struct TcnArgs {
    const float* u;
    const float* x;
    const float* w;
    const float* s3;
    const float* t3;
    const int32_t* n_active;
    float* out;
    int K, T, To, cin, cout, stride, residual, TT;
};

__global__ __launch_bounds__(THREADS) void stgcn_tcn_kernel(TcnArgs a) {
    __shared__ __attribute__((aligned(16))) float us[WROWS * US];
    const int n = blockIdx.x;
    if (n >= *a.n_active) return;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int K = a.K, T = a.T, cout = a.cout, stride = a.stride;
    const int to0 = blockIdx.y * a.TT;
    const int tt = min(a.TT, a.To - to0), rows = tt * K, rtiles = (rows + 15) >> 4;
    const int ct = blockIdx.z * 4 + wave;
    const bool wave_on = ct * 16 < cout;
    const int ncc = cout / CH;
    const int tin0 = to0 * stride - 4, wrows = ((tt - 1) * stride + 9) * K;      // the window: rows (t_in - tin0, v)
    const long long first = (long long)tin0 * K;                                  // window row 0 as a row of the clip
    const float* uclip = a.u + (size_t)n * T * K * cout;

    int base[MAXRT];                                            // per row tile: this lane's row in the window at tap 0
#pragma unroll
    for (int r = 0; r < MAXRT; ++r) {
        const int row = min(r * 16 + (lane & 15), rows - 1);    // rows past the tile read a row of the tile; never stored
        const int tl = row / K;
        base[r] = (tl * stride * K + (row - tl * K)) * US + 4 * (lane >> 4);
    }
    f32x4 acc[MAXRT];
#pragma unroll
    for (int r = 0; r < MAXRT; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int cc = 0; cc < ncc; ++cc) {
        __syncthreads();
        for (int i = tid; i < wrows * 4; i += THREADS) {
            const int r = i >> 2, q = i & 3;
            const long long cr = first + r;                     // a row outside [0, T K) lies before or after THIS clip
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (cr >= 0 && cr < (long long)T * K) v = *reinterpret_cast<const f32x4*>(uclip + (size_t)cr * cout + cc * CH + q * 4);
            *reinterpret_cast<f32x4*>(us + r * US + q * 4) = v;
        }
        __syncthreads();
        if (wave_on) {
            const f32x4* wp = reinterpret_cast<const f32x4*>(a.w) + ((size_t)(ct * ncc + cc) * 9) * WAVE + lane;
            for (int k = 0; k < 9; ++k) {
                const f32x4 wf = wp[k * WAVE];
                const float* up = us + k * K * US;
#pragma unroll
                for (int r = 0; r < MAXRT; ++r)
                    if (r < rtiles) mma4(acc[r], wf, *reinterpret_cast<const f32x4*>(up + base[r]));
            }
        }
    }
    if (a.residual == PPN_STGCN_RES_PROJ) {
        const int cin = a.cin, nrc = (cin + CH - 1) / CH;
        const f32x4* wproj = reinterpret_cast<const f32x4*>(a.w) + (size_t)(cout / 16) * ncc * 9 * WAVE;
        for (int rc = 0; rc < nrc; ++rc) {
            __syncthreads();
            for (int i = tid; i < rows * CH; i += THREADS) {
                const int r = i >> 4, ci = rc * CH + (i & 15);
                const int tl = r / K, v = r - tl * K;
                us[r * US + (i & 15)] =
                    ci < cin ? a.x[(((size_t)n * T + (size_t)(to0 + tl) * stride) * K + v) * cin + ci] : 0.f;
            }
            __syncthreads();
            if (wave_on) {
                const f32x4 wf = wproj[(size_t)(ct * nrc + rc) * WAVE + lane];
#pragma unroll
                for (int r = 0; r < MAXRT; ++r)
                    if (r < rtiles)
                        mma4(acc[r], wf, *reinterpret_cast<const f32x4*>(us + min(r * 16 + (lane & 15), rows - 1) * US +
                                                                          4 * (lane >> 4)));
            }
        }
    }
    if (!wave_on) return;
    const int ch = ct * 16 + 4 * (lane >> 4);
    const f32x4 s3 = *reinterpret_cast<const f32x4*>(a.s3 + ch), t3 = *reinterpret_cast<const f32x4*>(a.t3 + ch);
    const size_t orow0 = ((size_t)n * a.To + to0) * K, irow0 = ((size_t)n * T + to0) * K;
#pragma unroll
    for (int r = 0; r < MAXRT; ++r) {
        const int row = r * 16 + (lane & 15);
        if (r < rtiles && row < rows) {
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaf(acc[r][j], s3[j], t3[j]);
            if (a.residual == PPN_STGCN_RES_IDENTITY) {         // cin == cout, stride 1: the same row of the block input
                const f32x4 xr = *reinterpret_cast<const f32x4*>(a.x + (irow0 + row) * cout + ch);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] += xr[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
            *reinterpret_cast<f32x4*>(a.out + (orow0 + row) * cout + ch) = o;
        }
    }
}

// ---- pooling, classifier, arg-max ---------------------------------------------------------------------------------------------
struct HeadArgs {
    const float* x;
    const float* w;
    const float* b;
    const int32_t* rank;
    float* logits;
    int32_t* label;
    int TK, C, num_class;
};

__global__ __launch_bounds__(THREADS) void stgcn_head_kernel(HeadArgs a) {
    __shared__ float pooled[PPN_STGCN_MAX_C];
    __shared__ float bv[THREADS];
    __shared__ int bi[THREADS];
    const int b = blockIdx.x, tid = threadIdx.x, nc = a.num_class, C = a.C;
    const int r = a.rank[b];
    float* lg = a.logits + (size_t)b * nc;
    if (r < 0) {
        for (int j = tid; j < nc; j += THREADS) lg[j] = 0.f;
        if (tid == 0) a.label[b] = -1;
        return;
    }
    if (tid < C) {
        const float* xp = a.x + (size_t)r * a.TK * C + tid;
        float s = 0.f;
        for (int i = 0; i < a.TK; ++i) s += xp[(size_t)i * C];
        pooled[tid] = s / (float)a.TK;
    }
    __syncthreads();
    float best = 0.f;
    int besti = INT_MAX;
    for (int j = tid; j < nc; j += THREADS) {
        float s = a.b[j];
        for (int c = 0; c < C; ++c) s = fmaf(pooled[c], a.w[(size_t)c * nc + j], s);
        lg[j] = s;
        if (besti == INT_MAX || s > best) best = s, besti = j;   // ascending j: the lowest index of equal values stays
    }
    bv[tid] = best;
    bi[tid] = besti;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const float ov = bv[tid + s];
            const int oi = bi[tid + s];
            if (oi != INT_MAX && (bi[tid] == INT_MAX || ov > bv[tid] || (ov == bv[tid] && oi < bi[tid]))) bv[tid] = ov, bi[tid] = oi;
        }
        __syncthreads();
    }
    if (tid == 0) a.label[b] = bi[0];
}

int check_desc(const char* fn, const ppn_stgcn_desc* d, bool block) {
    if (!d) return ppn::fail(PPN_E_INVALID, "%s: NULL descriptor", fn);
    if (d->dtype != PPN_F32) return ppn::fail(PPN_E_UNSUPPORTED, "%s: dtype %d: only PPN_F32 is built", fn, d->dtype);
    if (d->K < 1 || d->K > PPN_MAX_KP) return ppn::fail(PPN_E_INVALID, "%s: K %d outside 1..%d", fn, d->K, PPN_MAX_KP);
    if (d->T < 1 || d->T > PPN_CLIP_MAX_LEN) return ppn::fail(PPN_E_INVALID, "%s: T %d outside 1..%d", fn, d->T, PPN_CLIP_MAX_LEN);
    if (!block) return PPN_OK;
    if (d->P < 1 || d->P > PPN_STGCN_MAX_P) return ppn::fail(PPN_E_INVALID, "%s: P %d outside 1..%d", fn, d->P, PPN_STGCN_MAX_P);
    if (d->cout < 16 || d->cout % 16 || d->cout > PPN_STGCN_MAX_C)
        return ppn::fail(PPN_E_INVALID, "%s: cout %d must be a multiple of 16 up to %d", fn, d->cout, PPN_STGCN_MAX_C);
    if (d->cin != 3 && (d->cin < 16 || d->cin % 16 || d->cin > PPN_STGCN_MAX_C))
        return ppn::fail(PPN_E_INVALID, "%s: cin %d must be 3 or a multiple of 16 up to %d", fn, d->cin, PPN_STGCN_MAX_C);
    if (d->stride != 1 && d->stride != 2) return ppn::fail(PPN_E_INVALID, "%s: stride %d", fn, d->stride);
    if (d->residual != PPN_STGCN_RES_NONE && d->residual != PPN_STGCN_RES_IDENTITY && d->residual != PPN_STGCN_RES_PROJ)
        return ppn::fail(PPN_E_INVALID, "%s: unknown residual %d", fn, d->residual);
    if (d->residual == PPN_STGCN_RES_IDENTITY && (d->cin != d->cout || d->stride != 1))
        return ppn::fail(PPN_E_INVALID, "%s: an identity shortcut needs cin == cout and stride 1", fn);
    return PPN_OK;
}

int check_capacity(const char* fn, int32_t capacity) {
    if (capacity < 1 || capacity % PPN_CLIP_SLOTS || capacity > PPN_STGCN_MAX_STREAMS * PPN_CLIP_SLOTS)
        return ppn::fail(PPN_E_INVALID, "%s: capacity %d must be streams * %d, streams in 1..%d", fn, capacity, PPN_CLIP_SLOTS,
                         PPN_STGCN_MAX_STREAMS);
    return PPN_OK;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int ppn_stgcn_input(const ppn_stgcn_desc* d, const float* x, const int32_t* ids, const int32_t* length,
                               int32_t streams, int32_t min_len, const float* scale, const float* shift, int32_t* active,
                               int32_t* n_active, int32_t* rank, float* x0, void* stream) {
    if (const int rc = check_desc("ppn_stgcn_input", d, false)) return rc;
    if (!x || !ids || !length || !scale || !shift || !active || !n_active || !rank || !x0)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_input: NULL pointer");
    if (streams < 1 || streams > PPN_STGCN_MAX_STREAMS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_input: %d streams outside 1..%d", streams, PPN_STGCN_MAX_STREAMS);
    InputArgs a{x, ids, length, scale, shift, active, n_active, rank, x0, d->K, d->T, min_len};
    stgcn_input_kernel<<<(unsigned)streams * PPN_CLIP_SLOTS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_stgcn_gcn(const ppn_stgcn_desc* d, const float* x, const float* w, const float* adj, const float* s0,
                             const float* t0, const int32_t* n_active, int32_t capacity, float* out, void* stream) {
    if (const int rc = check_desc("ppn_stgcn_gcn", d, true)) return rc;
    if (const int rc = check_capacity("ppn_stgcn_gcn", capacity)) return rc;
    if (!x || !w || !adj || !s0 || !t0 || !n_active || !out) return ppn::fail(PPN_E_INVALID, "ppn_stgcn_gcn: NULL pointer");
    if (!aligned16(w) || !aligned16(s0) || !aligned16(t0) || !aligned16(out))
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_gcn: w, s0, t0 and out must be 16-byte aligned");
    const int TT = tile_steps(d->K);
    GcnArgs a{x, w, adj, s0, t0, n_active, out, d->K, d->P, d->T, d->cin, d->cout, TT};
    const dim3 grid((unsigned)capacity, (unsigned)((d->T + TT - 1) / TT));
    stgcn_gcn_kernel<<<grid, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_stgcn_tcn(const ppn_stgcn_desc* d, const float* u, const float* x, const float* w, const float* s3,
                             const float* t3, const int32_t* n_active, int32_t capacity, float* out, void* stream) {
    if (const int rc = check_desc("ppn_stgcn_tcn", d, true)) return rc;
    if (const int rc = check_capacity("ppn_stgcn_tcn", capacity)) return rc;
    if (!u || !w || !s3 || !t3 || !n_active || !out || (d->residual != PPN_STGCN_RES_NONE && !x))
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_tcn: NULL pointer");
    if (!aligned16(u) || !aligned16(w) || !aligned16(s3) || !aligned16(t3) || !aligned16(out) ||
        (d->residual == PPN_STGCN_RES_IDENTITY && !aligned16(x)))
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_tcn: u, x, w, s3, t3 and out must be 16-byte aligned");
    const int TT = tile_steps(d->K), To = (d->T - 1) / d->stride + 1;
    if (((TT - 1) * d->stride + 9) * d->K > WROWS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_tcn: window of %d rows beyond %d", ((TT - 1) * d->stride + 9) * d->K, WROWS);
    TcnArgs a{u, x, w, s3, t3, n_active, out, d->K, d->T, To, d->cin, d->cout, d->stride, d->residual, TT};
    const dim3 grid((unsigned)capacity, (unsigned)((To + TT - 1) / TT), (unsigned)((d->cout + 63) / 64));
    stgcn_tcn_kernel<<<grid, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_stgcn_head(const ppn_stgcn_desc* d, int32_t num_class, const float* x, const float* w, const float* b,
                              const int32_t* rank, int32_t streams, float* logits, int32_t* label, void* stream) {
    if (const int rc = check_desc("ppn_stgcn_head", d, false)) return rc;
    if (d->cout < 16 || d->cout % 16 || d->cout > PPN_STGCN_MAX_C)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_head: %d channels must be a multiple of 16 up to %d", d->cout, PPN_STGCN_MAX_C);
    if (num_class < 1 || num_class > PPN_STGCN_MAX_CLASS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_head: num_class %d outside 1..%d", num_class, PPN_STGCN_MAX_CLASS);
    if (streams < 1 || streams > PPN_STGCN_MAX_STREAMS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn_head: %d streams outside 1..%d", streams, PPN_STGCN_MAX_STREAMS);
    if (!x || !w || !b || !rank || !logits || !label) return ppn::fail(PPN_E_INVALID, "ppn_stgcn_head: NULL pointer");
    HeadArgs a{x, w, b, rank, logits, label, d->T * d->K, d->cout, num_class};
    stgcn_head_kernel<<<(unsigned)streams * PPN_CLIP_SLOTS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
