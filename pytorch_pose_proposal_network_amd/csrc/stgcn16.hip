// ST-GCN forward for one person per clip with IEEE half storage and v_mfma_f32_16x16x32_f16 (contract in include/ppn.h,
// ppn_stgcn16_*; restatement in tests/stgcn16_ref.py).  Activations between the stages are half [n][t][v][c], channels last
// (x0: [n][t][v][4], the fourth value zero), for the n active clips only; every kernel is launched for the capacity S * 64 and
// reads n from device memory.  The decomposition is csrc/stgcn.hip's; the operand staging is not: a fragment is 8 halves
// (16 bytes) per lane, lane l holding A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][column l & 15], and the
// depth step is 32.
//
//   stgcn16_input_kernel  stgcn_input_kernel's selection (the same integers), the clip's planes through data_bn into [t][v][4]
//   stgcn16_gcn_kernel    one workgroup of four waves per (clip, tile of TT time steps).  Per chunk of 32 input channels: the
//                         tile's rows TRANSPOSED into LDS, xt[t][ci][v], v padded to 32 with zeros, so that the aggregation
//                         y[(t, w)][p][ci] = sum_v x[t][v][ci] A[p][v][w] is ONE MFMA per (t, p, 16 ci, 16 w): D[ci][w] =
//                         xt[ci][v] At[w][v], both fragments one ds_read_b128 (the adjacency lies transposed in LDS too).  y is
//                         rounded once to half into ys[(t, w)][p][ci]; then z += W x y, the weights as the A operand straight
//                         from global memory (packed on the host in fragment order), y as the B operand from LDS.  Wave w owns
//                         the channel tiles w, w + 4, .. and every row tile; a lane ends with four consecutive channels of
//                         one row: an 8-byte store
//   stgcn16_tcn_kernel    the same row tiling over output time steps, 64 output channels per workgroup.  Per chunk of 32
//                         channels the input window of the tile goes to LDS once and serves all nine taps.  Wave w owns the row
//                         tiles w, w + 4, w + 8 and all (up to four) channel tiles: one fragment of the window feeds four MFMAs.
//                         The projection shortcut is further depth over the block input's channels
//   stgcn16_head_kernel   stgcn_head_kernel reading half
// LDS rows are pitched 80 bytes (xt, At, the window) and 208 bytes (ys): an odd number of 16-byte slots, so the sixteen rows of
// a ds_read_b128 fragment read fall on sixteen different slots of the 256-byte bank row.  A depth lane the data does not cover
// (v >= K, a channel >= cin / cout) is ZERO in both operands: stale half bits can be inf or NaN, and 0 * inf poisons a sum.
// One output element is summed in one fixed order, whatever else is active: no atomics, no split reductions.  Conversions to
// half round to nearest even and do not clamp.  Built without SLP vectorisation like every MFMA file (build.py NOSLP).
#include <climits>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 h16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 h16x4;

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int CH = 32;                       // channels per depth chunk: the MFMA's depth step
constexpr int MAXR = 160;                    // rows (t, v) of a tile: 8 x 18 = 144 for the default skeleton
constexpr int MAXRT = MAXR / 16;
constexpr int MAXTT = 8;
constexpr int MAXP = PPN_STGCN_MAX_P;
constexpr int VP = 40;                       // pitch (halves) of a row of 32 depth values: 80 bytes = 5 slots of 16
constexpr int YS = MAXP * CH + 8;            // pitch of the aggregated tile: 104 halves = 208 bytes = 13 slots
constexpr int GCT = PPN_STGCN_MAX_C / 64;    // channel tiles of 16 per wave in the graph convolution
constexpr int TCT = 4;                       // channel tiles per workgroup (and per wave) in the temporal convolution
constexpr int TRT = (MAXRT + 3) / 4;         // row tiles per wave there
constexpr int WROWS = 544;                   // the largest window: K = 32, TT = 5, stride 2 -> 17 x 32
static_assert(MAXR % 16 == 0 && PPN_MAX_KP <= 32 && PPN_CLIP_SLOTS == 64 && MAXR <= WROWS, "");

__host__ __device__ inline int tile_steps(int K) {          // time steps per tile: TT * K <= MAXR
    const int t = MAXR / K;
    return t > MAXTT ? MAXTT : t;
}

__device__ __forceinline__ f32x4 mma(const f32x4& acc, const h16x8& a, const h16x8& b) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
}

__device__ __forceinline__ h16x4 to_half4(const f32x4& v) {   // round to nearest even, no clamp: beyond 65504 -> inf
    return h16x4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
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
    _Float16* x0;
    int K, T, min_len;
};

__global__ __launch_bounds__(THREADS) void stgcn16_input_kernel(InputArgs a) {
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
    h16x4* dst = reinterpret_cast<h16x4*>(a.x0) + (size_t)r * TK;
    for (int tv = tid; tv < TK; tv += THREADS) {
        const int ch = (tv % a.K) * 3;
        h16x4 o;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (_Float16)fmaf(src[c * TK + tv], a.scale[ch + c], a.shift[ch + c]);
        o[3] = (_Float16)0.f;
        dst[tv] = o;
    }
}

// ---- graph convolution --------------------------------------------------------------------------------------------------------
struct GcnArgs {
    const _Float16* x;
    const _Float16* w;
    const _Float16* adj;
    const float* s0;
    const float* t0;
    const int32_t* n_active;
    _Float16* out;
    int K, P, T, cin, cout, TT;
};

__global__ __launch_bounds__(THREADS, 2) void stgcn16_gcn_kernel(GcnArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 xt[MAXTT * CH * VP];      // [t][ci][v], zero for v >= K
    __shared__ __attribute__((aligned(16))) _Float16 ys[MAXR * YS];            // [(t, w)][p][ci]
    __shared__ __attribute__((aligned(16))) _Float16 at[MAXP * 32 * VP];       // [p][w][v], zero beyond K
    const int n = blockIdx.x;
    if (n >= *a.n_active) return;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int col = lane & 15, g = lane >> 4;
    const int K = a.K, P = a.P, cin = a.cin, cout = a.cout;
    const int pitch = cin == 3 ? 4 : cin;                       // halves per row of x
    const int t0 = blockIdx.y * a.TT;
    const int tt = min(a.TT, a.T - t0), rows = tt * K, rtiles = (rows + 15) >> 4;
    const int myct = (cout / 16 - wave + 3) / 4;                // this wave's tiles of 16 output channels: wave + 4 i
    const int ncc = (cin + CH - 1) / CH;
    const int ntiles = (K + 15) >> 4;                           // the aggregation's column tiles (w)
    const size_t row0 = ((size_t)n * a.T + t0) * K;             // first row (t, v) of the tile in x and out
    const _Float16 zero = (_Float16)0.f;

    for (int i = tid; i < P * 32 * VP; i += THREADS) {
        const int p = i / (32 * VP), w = (i / VP) % 32, v = i % VP;
        at[i] = (v < K && w < K) ? a.adj[(p * K + v) * K + w] : zero;
    }
    for (int i = tid; i < MAXTT * CH * VP; i += THREADS) xt[i] = zero;   // the depth lanes v >= K stay zero
    for (int i = tid; i < MAXR * YS; i += THREADS) ys[i] = zero;         // the rows past `rows` of the last row tile stay zero

    f32x4 acc[GCT][MAXRT];
#pragma unroll
    for (int i = 0; i < GCT; ++i)
#pragma unroll
        for (int r = 0; r < MAXRT; ++r) acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int cc = 0; cc < ncc; ++cc) {
        __syncthreads();                                        // the MFMAs of the chunk before have read ys and xt
        for (int i = tid; i < rows * (CH / 4); i += THREADS) {  // four channels of one row: 8 bytes
            const int r = i >> 3, q = i & 7, ci = cc * CH + 4 * q;
            h16x4 v = h16x4{zero, zero, zero, zero};
            if (ci < pitch) v = *reinterpret_cast<const h16x4*>(a.x + (row0 + r) * pitch + ci);
            if (cin == 3) v[3] = zero;                          // the pad channel is a depth lane past the data
            const int t = r / K;
            _Float16* dst = xt + (t * CH + 4 * q) * VP + (r - t * K);
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j * VP] = v[j];
        }
        __syncthreads();
        // y[t][w][p][ci] = sum_v x[t][v][ci] adj[p][v][w] as D[ci][w] = A[ci][v] B[v][w]: a lane ends with four consecutive ci
        for (int unit = wave; unit < tt * P * ntiles * 2; unit += THREADS / WAVE) {
            const int ch = unit & 1, nt = (unit >> 1) % ntiles, p = ((unit >> 1) / ntiles) % P, t = (unit >> 1) / (ntiles * P);
            const h16x8 xa = *reinterpret_cast<const h16x8*>(xt + (t * CH + ch * 16 + col) * VP + 8 * g);
            const h16x8 ab = *reinterpret_cast<const h16x8*>(at + (p * 32 + nt * 16 + col) * VP + 8 * g);
            const f32x4 d = mma(f32x4{0.f, 0.f, 0.f, 0.f}, xa, ab);
            const int w = nt * 16 + col;
            if (w < K) *reinterpret_cast<h16x4*>(ys + (t * K + w) * YS + p * CH + ch * 16 + 4 * g) = to_half4(d);
        }
        __syncthreads();
        if (myct > 0) {
            for (int p = 0; p < P; ++p) {
                h16x8 wf[GCT];
#pragma unroll
                for (int i = 0; i < GCT; ++i)
                    if (i < myct)
                        wf[i] = reinterpret_cast<const h16x8*>(a.w)[((size_t)((wave + 4 * i) * ncc + cc) * P + p) * WAVE + lane];
                const _Float16* yp = ys + col * YS + p * CH + 8 * g;
#pragma unroll
                for (int r = 0; r < MAXRT; ++r) {
                    if (r < rtiles) {
                        const h16x8 yf = *reinterpret_cast<const h16x8*>(yp + r * 16 * YS);
#pragma unroll
                        for (int i = 0; i < GCT; ++i)
                            if (i < myct) acc[i][r] = mma(acc[i][r], wf[i], yf);
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
                *reinterpret_cast<h16x4*>(a.out + (row0 + row) * cout + ch) = to_half4(o);
            }
        }
    }
}

// ---- temporal convolution -----------------------------------------------------------------------------------------------------
struct TcnArgs {
    const _Float16* u;
    const _Float16* x;
    const _Float16* w;
    const float* s3;
    const float* t3;
    const int32_t* n_active;
    _Float16* out;
    int K, T, To, cin, cout, stride, residual, TT;
};

__global__ __launch_bounds__(THREADS, 2) void stgcn16_tcn_kernel(TcnArgs a) {
    __shared__ __attribute__((aligned(16))) _Float16 us[WROWS * VP];
    const int n = blockIdx.x;
    if (n >= *a.n_active) return;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int col = lane & 15, g = lane >> 4;
    const int K = a.K, T = a.T, cout = a.cout, stride = a.stride;
    const int to0 = blockIdx.y * a.TT;
    const int tt = min(a.TT, a.To - to0), rows = tt * K, rtiles = (rows + 15) >> 4;
    const int ct0 = blockIdx.z * TCT;
    const int nct = min(TCT, cout / 16 - ct0);                  // channel tiles of this workgroup: >= 1 by the grid
    const int ncc = (cout + CH - 1) / CH;
    const int tin0 = to0 * stride - 4, wrows = ((tt - 1) * stride + 9) * K;      // the window: rows (t_in - tin0, v)
    const long long first = (long long)tin0 * K;                                  // window row 0 as a row of the clip
    const _Float16* uclip = a.u + (size_t)n * T * K * cout;
    const _Float16 zero = (_Float16)0.f;
    const h16x8 zero8 = h16x8{zero, zero, zero, zero, zero, zero, zero, zero};

    int base[TRT];                                              // per row tile of this wave: the lane's row in the window at tap 0
    int prow[TRT];                                              // and in the shortcut's rows
#pragma unroll
    for (int r = 0; r < TRT; ++r) {
        const int row = min((wave + 4 * r) * 16 + col, rows - 1);   // rows past the tile read a row of the tile; never stored
        const int tl = row / K;
        base[r] = (tl * stride * K + (row - tl * K)) * VP + 8 * g;
        prow[r] = row * VP + 8 * g;
    }
    f32x4 acc[TCT][TRT];
#pragma unroll
    for (int i = 0; i < TCT; ++i)
#pragma unroll
        for (int r = 0; r < TRT; ++r) acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int cc = 0; cc < ncc; ++cc) {
        __syncthreads();
        for (int i = tid; i < wrows * 4; i += THREADS) {        // eight channels of one row: 16 bytes
            const int r = i >> 2, q = i & 3, c0 = cc * CH + q * 8;
            const long long cr = first + r;                     // a row outside [0, T K) lies before or after THIS clip
            h16x8 v = zero8;                                    // and a channel >= cout is a depth lane past the data
            if (c0 < cout && cr >= 0 && cr < (long long)T * K) v = *reinterpret_cast<const h16x8*>(uclip + (size_t)cr * cout + c0);
            *reinterpret_cast<h16x8*>(us + r * VP + q * 8) = v;
        }
        __syncthreads();
        const h16x8* wp = reinterpret_cast<const h16x8*>(a.w) + lane;
        for (int k = 0; k < 9; ++k) {
            h16x8 wf[TCT];
#pragma unroll
            for (int i = 0; i < TCT; ++i)
                if (i < nct) wf[i] = wp[((size_t)((ct0 + i) * ncc + cc) * 9 + k) * WAVE];
            const _Float16* up = us + k * K * VP;
#pragma unroll
            for (int r = 0; r < TRT; ++r) {
                if (wave + 4 * r < rtiles) {
                    const h16x8 uf = *reinterpret_cast<const h16x8*>(up + base[r]);
#pragma unroll
                    for (int i = 0; i < TCT; ++i)
                        if (i < nct) acc[i][r] = mma(acc[i][r], wf[i], uf);
                }
            }
        }
    }
    if (a.residual == PPN_STGCN_RES_PROJ) {
        const int cin = a.cin, nrc = (cin + CH - 1) / CH, pitch = cin == 3 ? 4 : cin;
        const h16x8* wproj = reinterpret_cast<const h16x8*>(a.w) + (size_t)(cout / 16) * ncc * 9 * WAVE + lane;
        for (int rc = 0; rc < nrc; ++rc) {
            __syncthreads();
            for (int i = tid; i < rows * (CH / 4); i += THREADS) {      // four channels of one row: 8 bytes
                const int r = i >> 3, q = i & 7, ci = rc * CH + 4 * q;
                const int tl = r / K, v = r - tl * K;
                h16x4 xv = h16x4{zero, zero, zero, zero};
                if (ci < pitch)
                    xv = *reinterpret_cast<const h16x4*>(a.x + (((size_t)n * T + (size_t)(to0 + tl) * stride) * K + v) * pitch + ci);
                if (cin == 3) xv[3] = zero;
                *reinterpret_cast<h16x4*>(us + r * VP + 4 * q) = xv;
            }
            __syncthreads();
            h16x8 wf[TCT];
#pragma unroll
            for (int i = 0; i < TCT; ++i)
                if (i < nct) wf[i] = wproj[(size_t)((ct0 + i) * nrc + rc) * WAVE];
#pragma unroll
            for (int r = 0; r < TRT; ++r) {
                if (wave + 4 * r < rtiles) {
                    const h16x8 xf = *reinterpret_cast<const h16x8*>(us + prow[r]);
#pragma unroll
                    for (int i = 0; i < TCT; ++i)
                        if (i < nct) acc[i][r] = mma(acc[i][r], wf[i], xf);
                }
            }
        }
    }
    const size_t orow0 = ((size_t)n * a.To + to0) * K, irow0 = ((size_t)n * T + to0) * K;
#pragma unroll
    for (int i = 0; i < TCT; ++i) {
        if (i >= nct) break;
        const int ch = (ct0 + i) * 16 + 4 * g;
        const f32x4 s3 = *reinterpret_cast<const f32x4*>(a.s3 + ch), t3 = *reinterpret_cast<const f32x4*>(a.t3 + ch);
#pragma unroll
        for (int r = 0; r < TRT; ++r) {
            const int row = (wave + 4 * r) * 16 + col;
            if (wave + 4 * r < rtiles && row < rows) {
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaf(acc[i][r][j], s3[j], t3[j]);
                if (a.residual == PPN_STGCN_RES_IDENTITY) {     // cin == cout, stride 1: the same row of the block input
                    const h16x4 xr = *reinterpret_cast<const h16x4*>(a.x + (irow0 + row) * cout + ch);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] += (float)xr[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
                *reinterpret_cast<h16x4*>(a.out + (orow0 + row) * cout + ch) = to_half4(o);
            }
        }
    }
}

// ---- pooling, classifier, arg-max ---------------------------------------------------------------------------------------------
struct HeadArgs {
    const _Float16* x;
    const float* w;
    const float* b;
    const int32_t* rank;
    float* logits;
    int32_t* label;
    int TK, C, num_class;
};

__global__ __launch_bounds__(THREADS) void stgcn16_head_kernel(HeadArgs a) {
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
        const _Float16* xp = a.x + (size_t)r * a.TK * C + tid;
        float s = 0.f;
        for (int i = 0; i < a.TK; ++i) s += (float)xp[(size_t)i * C];
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
    if (d->dtype != PPN_F16) return ppn::fail(PPN_E_UNSUPPORTED, "%s: dtype %d: these entry points are PPN_F16's", fn, d->dtype);
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

extern "C" int ppn_stgcn16_input(const ppn_stgcn_desc* d, const float* x, const int32_t* ids, const int32_t* length,
                                 int32_t streams, int32_t min_len, const float* scale, const float* shift, int32_t* active,
                                 int32_t* n_active, int32_t* rank, void* x0, void* stream) {
    if (const int rc = check_desc("ppn_stgcn16_input", d, false)) return rc;
    if (!x || !ids || !length || !scale || !shift || !active || !n_active || !rank || !x0)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_input: NULL pointer");
    if (streams < 1 || streams > PPN_STGCN_MAX_STREAMS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_input: %d streams outside 1..%d", streams, PPN_STGCN_MAX_STREAMS);
    if (!aligned16(x0)) return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_input: x0 must be 16-byte aligned");
    InputArgs a{x, ids, length, scale, shift, active, n_active, rank, static_cast<_Float16*>(x0), d->K, d->T, min_len};
    stgcn16_input_kernel<<<(unsigned)streams * PPN_CLIP_SLOTS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_stgcn16_gcn(const ppn_stgcn_desc* d, const void* x, const void* w, const void* adj, const float* s0,
                               const float* t0, const int32_t* n_active, int32_t capacity, void* out, void* stream) {
    if (const int rc = check_desc("ppn_stgcn16_gcn", d, true)) return rc;
    if (const int rc = check_capacity("ppn_stgcn16_gcn", capacity)) return rc;
    if (!x || !w || !adj || !s0 || !t0 || !n_active || !out) return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_gcn: NULL pointer");
    if (!aligned16(x) || !aligned16(w) || !aligned16(s0) || !aligned16(t0) || !aligned16(out))
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_gcn: x, w, s0, t0 and out must be 16-byte aligned");
    const int TT = tile_steps(d->K);
    GcnArgs a{static_cast<const _Float16*>(x), static_cast<const _Float16*>(w), static_cast<const _Float16*>(adj), s0, t0,
              n_active, static_cast<_Float16*>(out), d->K, d->P, d->T, d->cin, d->cout, TT};
    const dim3 grid((unsigned)capacity, (unsigned)((d->T + TT - 1) / TT));
    stgcn16_gcn_kernel<<<grid, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_stgcn16_tcn(const ppn_stgcn_desc* d, const void* u, const void* x, const void* w, const float* s3,
                               const float* t3, const int32_t* n_active, int32_t capacity, void* out, void* stream) {
    if (const int rc = check_desc("ppn_stgcn16_tcn", d, true)) return rc;
    if (const int rc = check_capacity("ppn_stgcn16_tcn", capacity)) return rc;
    if (!u || !w || !s3 || !t3 || !n_active || !out || (d->residual != PPN_STGCN_RES_NONE && !x))
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_tcn: NULL pointer");
    if (!aligned16(u) || !aligned16(w) || !aligned16(s3) || !aligned16(t3) || !aligned16(out) ||
        (d->residual != PPN_STGCN_RES_NONE && !aligned16(x)))
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_tcn: u, x, w, s3, t3 and out must be 16-byte aligned");
    const int TT = tile_steps(d->K), To = (d->T - 1) / d->stride + 1;
    if (((TT - 1) * d->stride + 9) * d->K > WROWS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_tcn: window of %d rows beyond %d", ((TT - 1) * d->stride + 9) * d->K, WROWS);
    TcnArgs a{static_cast<const _Float16*>(u), static_cast<const _Float16*>(x), static_cast<const _Float16*>(w), s3, t3,
              n_active, static_cast<_Float16*>(out), d->K, d->T, To, d->cin, d->cout, d->stride, d->residual, TT};
    const dim3 grid((unsigned)capacity, (unsigned)((To + TT - 1) / TT), (unsigned)((d->cout + 63) / 64));
    stgcn16_tcn_kernel<<<grid, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_stgcn16_head(const ppn_stgcn_desc* d, int32_t num_class, const void* x, const float* w, const float* b,
                                const int32_t* rank, int32_t streams, float* logits, int32_t* label, void* stream) {
    if (const int rc = check_desc("ppn_stgcn16_head", d, false)) return rc;
    if (d->cout < 16 || d->cout % 16 || d->cout > PPN_STGCN_MAX_C)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_head: %d channels must be a multiple of 16 up to %d", d->cout, PPN_STGCN_MAX_C);
    if (num_class < 1 || num_class > PPN_STGCN_MAX_CLASS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_head: num_class %d outside 1..%d", num_class, PPN_STGCN_MAX_CLASS);
    if (streams < 1 || streams > PPN_STGCN_MAX_STREAMS)
        return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_head: %d streams outside 1..%d", streams, PPN_STGCN_MAX_STREAMS);
    if (!x || !w || !b || !rank || !logits || !label) return ppn::fail(PPN_E_INVALID, "ppn_stgcn16_head: NULL pointer");
    HeadArgs a{static_cast<const _Float16*>(x), w, b, rank, logits, label, d->T * d->K, d->cout, num_class};
    stgcn16_head_kernel<<<(unsigned)streams * PPN_CLIP_SLOTS, THREADS, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
