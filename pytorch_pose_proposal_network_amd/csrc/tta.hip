// Horizontal-flip test-time averaging: merge the head of a frame with the head of its mirror image, and stage the
// doubled batch (contract in include/ppn.h, NumPy restatement tests/tta_ref.py).
//
//   tta_limb_kernel<V>   HBM-bound: streams the limb block of BOTH heads once (2 x E*sH*sW planes of H*W cells per image).
//                        grid = (E * SS, batch, cell groups): a workgroup owns the window rows s of one slice (of SS) of one
//                        (edge, image) and Q * V consecutive cells.  Thread (q, r) walks the rows s = begin + r, + NS, .. of
//                        its V cells: plane s of A forwards, plane (edge_mirror[e], ly, sW-1-lx) of Bm with the V cells taken
//                        from the mirrored columns of the same grid row (one contiguous vector, reversed in registers), so
//                        both reads are coalesced.  Four rows (eight loads) are issued before the first add.  m = (a + b) *
//                        0.5f goes to out_head when asked for, and into a strict-greater running maximum (first s within a
//                        thread).  The NS partial keys of a cell meet in LDS; the slice's key is stored (SS = 1) or folded
//                        into out_keys with a u64 atomicMax (SS > 1; the unary launch in front of it zeroes out_keys).  A key is value
//                        bits << 32 | ~s, values are >= 0, so the integer maximum is the largest value and then the lowest
//                        s, whatever order the slices arrive in.
//   tta_unary_kernel     the 6K unary channels, one thread per value: keypoint permutation, column mirror, 1 - x on group 2;
//                        it also clears out_keys for a split limb pass.
//   tta_stage_kernel     dst = [src | src with every row of `width` elements reversed], elements of 3 or 4 bytes.
// Built with -ffp-contract=off and without fast-math: one IEEE add and one multiply per value, subnormals kept.
#include "common.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>

namespace {

constexpr int ROWS_IN_FLIGHT = 4;        // rows per trip: 2 * ROWS_IN_FLIGHT vector loads before the first use

template <int V> __device__ __forceinline__ void load_fwd(const float* p, float (&a)[V]);
template <> __device__ __forceinline__ void load_fwd<1>(const float* p, float (&a)[1]) { a[0] = *p; }
template <> __device__ __forceinline__ void load_fwd<4>(const float* p, float (&a)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
}
// the V cells at p in descending address order: cell i of the thread is mirrored column i of the vector
template <int V> __device__ __forceinline__ void load_rev(const float* p, float (&a)[V]);
template <> __device__ __forceinline__ void load_rev<1>(const float* p, float (&a)[1]) { a[0] = *p; }
template <> __device__ __forceinline__ void load_rev<4>(const float* p, float (&a)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    a[0] = v.w; a[1] = v.z; a[2] = v.y; a[3] = v.x;
}
template <int V> __device__ __forceinline__ void store_fwd(float* p, const float (&a)[V]);
template <> __device__ __forceinline__ void store_fwd<1>(float* p, const float (&a)[1]) { *p = a[0]; }
template <> __device__ __forceinline__ void store_fwd<4>(float* p, const float (&a)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
}

struct LimbArgs {
    const float* a;                      // [B][C][ncell]
    const float* b;
    unsigned long long* keys;            // [B][E][ncell]
    float* head;                         // [B][C][ncell] or NULL
    int C, e_chan0, S, sW, W, ncell, E;
    int nvec;                            // ncell / V
    int Q, NS;                           // cell vectors per workgroup, row slices per workgroup
    int SS, rows_per_slice;              // window slices per (edge, image), ceil(S / SS)
    int edge_mirror[PPN_MAX_EDGES];
};

template <int V>
__global__ void __launch_bounds__(1024) tta_limb_kernel(LimbArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(smem);      // [NS][Q * V]

    const int edge = blockIdx.x / p.SS, slice = blockIdx.x % p.SS, img = blockIdx.y;
    const int t = threadIdx.x, q = t % p.Q, r = t / p.Q;
    const int qg = blockIdx.z * p.Q + q;                                          // cell vector within the plane
    const int ncl = p.Q * V;
    const int s_begin = slice * p.rows_per_slice, s_end = min(p.S, s_begin + p.rows_per_slice);

    if (r < p.NS) {
        unsigned long long key[V];
#pragma unroll
        for (int i = 0; i < V; ++i) key[i] = 0ull;                                // below every real key
        if (qg < p.nvec && s_begin + r < s_end) {
            const int c0 = qg * V, gi = c0 / p.W, gj = c0 % p.W;                  // V divides W when V > 1: one grid row
            const int cm = gi * p.W + (p.W - V - gj);                             // first (lowest) mirrored cell
            const size_t img_off = (size_t)img * p.C * p.ncell;
            const float* pa = p.a + img_off + ((size_t)p.e_chan0 + (size_t)edge * p.S) * p.ncell + c0;
            const float* pb = p.b + img_off + ((size_t)p.e_chan0 + (size_t)p.edge_mirror[edge] * p.S) * p.ncell + cm;
            float* ph = p.head ? p.head + img_off + ((size_t)p.e_chan0 + (size_t)edge * p.S) * p.ncell + c0 : nullptr;

            float best[V];
            int bidx[V];
#pragma unroll
            for (int i = 0; i < V; ++i) { best[i] = -1.f; bidx[i] = 0; }
            const int first = s_begin + r;
            const int step_lx = p.NS % p.sW;
            int lx = first % p.sW;                                                // column of row s in the window
            for (int s0 = first; s0 < s_end; s0 += ROWS_IN_FLIGHT * p.NS) {
                float va[ROWS_IN_FLIGHT][V], vb[ROWS_IN_FLIGHT][V];
                int lxu = lx;
#pragma unroll
                for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
                    const int s = s0 + u * p.NS;
                    const bool in = s < s_end;                                    // a row past the slice re-reads the first
                    const int sa = in ? s : first;
                    const int sb = in ? s + (p.sW - 1 - 2 * lxu) : first;         // (ly, sW-1-lx); any valid row when !in
                    load_fwd<V>(pa + (size_t)sa * p.ncell, va[u]);
                    load_rev<V>(pb + (size_t)sb * p.ncell, vb[u]);
                    lxu += step_lx;
                    if (lxu >= p.sW) lxu -= p.sW;
                }
                lx = lxu;
#pragma unroll
                for (int u = 0; u < ROWS_IN_FLIGHT; ++u) {
                    const int s = s0 + u * p.NS;
                    const bool in = s < s_end;
                    float m[V];
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        m[i] = (va[u][i] + vb[u][i]) * 0.5f;
                        if (in && m[i] > best[i]) { best[i] = m[i]; bidx[i] = s; }     // strict: first maximum of this thread
                    }
                    if (ph && in) store_fwd<V>(ph + (size_t)s * p.ncell, m);
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                key[i] = (unsigned long long)__float_as_uint(best[i]) << 32 | (unsigned)~(unsigned)bidx[i];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) s_key[(size_t)r * ncl + V * q + i] = key[i];
    }
    __syncthreads();
    for (int cell = t; cell < ncl; cell += blockDim.x) {
        const int cg = blockIdx.z * ncl + cell;
        if (cg >= p.ncell) continue;
        unsigned long long k = s_key[cell];
        for (int rr = 1; rr < p.NS; ++rr) {
            const unsigned long long o = s_key[(size_t)rr * ncl + cell];
            k = o > k ? o : k;
        }
        unsigned long long* dst = p.keys + ((size_t)img * p.E + edge) * p.ncell + cg;
        if (p.SS == 1) *dst = k;
        else if (k) atomicMax(dst, k);
    }
}

struct UnaryArgs {
    const float* a;
    const float* b;
    float* unary;                        // [B][6K][ncell]
    float* head;                         // [B][C][ncell] or NULL
    int C, K, W, ncell;
    long long total;                     // B * 6K * ncell
    unsigned long long* zero_keys;       // out_keys when the limb pass folds into it with atomicMax, else NULL
    long long n_keys;                    // B * E * ncell
    int kp_mirror[PPN_MAX_KP];
};

__global__ void __launch_bounds__(256) tta_unary_kernel(UnaryArgs p) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p.zero_keys && idx < p.n_keys) p.zero_keys[idx] = 0ull;
    if (idx >= p.total) return;
    const int cell = (int)(idx % p.ncell);
    const long long chan_img = idx / p.ncell;
    const int ch = (int)(chan_img % (6 * p.K)), img = (int)(chan_img / (6 * p.K));
    const int g = ch / p.K, k = ch % p.K;
    const int gi = cell / p.W, gj = cell % p.W;
    const size_t img_off = (size_t)img * p.C * p.ncell;
    const float va = p.a[img_off + (size_t)ch * p.ncell + cell];
    float vb = p.b[img_off + ((size_t)g * p.K + p.kp_mirror[k]) * p.ncell + gi * p.W + (p.W - 1 - gj)];
    if (g == 2) vb = 1.0f - vb;                                                   // the cell-relative x offset
    const float m = (va + vb) * 0.5f;
    p.unary[idx] = m;
    if (p.head) p.head[img_off + (size_t)ch * p.ncell + cell] = m;
}

template <typename T, int N>
__global__ void __launch_bounds__(256)
tta_stage_kernel(const T* __restrict__ src, T* __restrict__ dst, long long rows, int width) {
    const long long total = rows * width;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // element of N values
    if (idx >= total) return;
    const long long row = idx / width;
    const int col = (int)(idx % width);
    const long long rev = total + row * width + (width - 1 - col);
    T v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = src[idx * N + i];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        dst[idx * N + i] = v[i];
        dst[rev * N + i] = v[i];
    }
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// m[0 .. n-1] is an involution of [0, n)
bool involution(const int32_t* m, int n) {
    for (int i = 0; i < n; ++i)
        if (m[i] < 0 || m[i] >= n || m[m[i]] != i) return false;
    return true;
}

}  // namespace

extern "C" int ppn_tta_merge(const ppn_tta_cfg* cfg, const float* head_a, const float* head_b, int32_t batch,
                             float* out_unary, uint64_t* out_keys, float* out_head, void* stream) {
    if (!cfg || !head_a || !head_b || !out_unary || !out_keys)
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: NULL pointer");
    if (cfg->K < 1 || cfg->K > PPN_MAX_KP || cfg->E < 0 || cfg->E > PPN_MAX_EDGES)
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: K %d / E %d outside 1..%d / 0..%d", cfg->K, cfg->E, PPN_MAX_KP,
                         PPN_MAX_EDGES);
    if (cfg->sH < 1 || cfg->sW < 1 || cfg->H < 1 || cfg->W < 1 || batch < 1 || batch > 65535)
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: bad geometry (window %d x %d, grid %d x %d, batch %d)", cfg->sH,
                         cfg->sW, cfg->H, cfg->W, batch);
    if ((long long)cfg->sH * cfg->sW > (1 << 20) || (long long)cfg->H * cfg->W > (1 << 24))
        return ppn::fail(PPN_E_UNSUPPORTED, "ppn_tta_merge: window %d x %d or grid %d x %d too large", cfg->sH, cfg->sW,
                         cfg->H, cfg->W);
    if (!involution(cfg->kp_mirror, cfg->K))
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: kp_mirror is not an involution of [0, %d)", cfg->K);
    if (!involution(cfg->edge_mirror, cfg->E))
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: edge_mirror is not an involution of [0, %d)", cfg->E);
    const int K = cfg->K, E = cfg->E, S = cfg->sH * cfg->sW, W = cfg->W, ncell = cfg->H * cfg->W;
    const long long C = 6ll * K + (long long)E * S;
    if (C > 0x7fffffff) return ppn::fail(PPN_E_UNSUPPORTED, "ppn_tta_merge: %lld channels", C);
    const size_t head_bytes = (size_t)batch * C * ncell * sizeof(float);
    const size_t unary_bytes = (size_t)batch * 6 * K * ncell * sizeof(float);
    const size_t keys_bytes = (size_t)batch * E * ncell * sizeof(uint64_t);
    if (out_head && (overlaps(out_head, head_bytes, head_a, head_bytes) || overlaps(out_head, head_bytes, head_b, head_bytes)))
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: out_head aliases an input head");
    if (overlaps(out_unary, unary_bytes, head_a, head_bytes) || overlaps(out_unary, unary_bytes, head_b, head_bytes) ||
        overlaps(out_keys, keys_bytes, head_a, head_bytes) || overlaps(out_keys, keys_bytes, head_b, head_bytes))
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: out_unary / out_keys alias an input head");
    if (reinterpret_cast<uintptr_t>(head_a) % 4 || reinterpret_cast<uintptr_t>(head_b) % 4 ||
        reinterpret_cast<uintptr_t>(out_unary) % 4 || reinterpret_cast<uintptr_t>(out_head) % 4 ||
        reinterpret_cast<uintptr_t>(out_keys) % 8)
        return ppn::fail(PPN_E_INVALID, "ppn_tta_merge: misaligned pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);

    // Launch geometry of the limb pass.  V: 16-byte vectors when a grid row is a whole number of them and everything is
    // 16-byte aligned (a function of the shape and the pointers).  Q x NS threads: Q cell vectors, NS window-row slices.
    // SS: window slices per (edge, image), combined by atomicMax -- the only free choice, PPN_TTA_SPLIT (read per call) sets it.
    const bool al16 = (reinterpret_cast<uintptr_t>(head_a) | reinterpret_cast<uintptr_t>(head_b) |
                       reinterpret_cast<uintptr_t>(out_head)) % 16 == 0;
    const int V = (W % 4 == 0 && al16) ? 4 : 1;
    LimbArgs p{};
    p.a = head_a; p.b = head_b; p.keys = reinterpret_cast<unsigned long long*>(out_keys); p.head = out_head;
    p.C = (int)C; p.e_chan0 = 6 * K; p.S = S; p.sW = cfg->sW; p.W = W; p.ncell = ncell; p.E = E;
    p.nvec = ncell / V;
    p.Q = std::min(p.nvec, 256);
    p.NS = std::max(1, std::min(std::min(1024 / p.Q, 8), S));
    const int CG = (p.nvec + p.Q - 1) / p.Q;
    if (CG > 65535) return ppn::fail(PPN_E_UNSUPPORTED, "ppn_tta_merge: grid of %d cells is too large", ncell);
    // enough workgroups for several rounds of the 256 CUs, but at least ROWS_IN_FLIGHT rows per thread
    const int ss_max = std::max(1, S / (ROWS_IN_FLIGHT * p.NS));
    const long long wgs = std::max<long long>(1, (long long)E * batch * CG);
    int SS = (int)std::min<long long>((2048 + wgs - 1) / wgs, ss_max);
    if (const char* env = getenv("PPN_TTA_SPLIT")) {
        const int v = atoi(env);
        if (v > 0) SS = std::min(v, S);
    }
    p.SS = SS;
    p.rows_per_slice = (S + SS - 1) / SS;
    if ((long long)E * SS > 0x7fffffff) return ppn::fail(PPN_E_UNSUPPORTED, "ppn_tta_merge: %d x %d slices", E, SS);
    for (int e = 0; e < E; ++e) p.edge_mirror[e] = cfg->edge_mirror[e];

    {   // the 6K unary channels; the same launch clears the keys a split limb pass folds into (a kernel on the stream, not a
        // memset node: a captured graph ran a memset node out of order with the kernels around it, see plan.hip)
        UnaryArgs u{};
        u.a = head_a; u.b = head_b; u.unary = out_unary; u.head = out_head;
        u.C = (int)C; u.K = K; u.W = W; u.ncell = ncell;
        u.total = (long long)batch * 6 * K * ncell;
        u.zero_keys = SS > 1 ? p.keys : nullptr;
        u.n_keys = (long long)batch * E * ncell;
        for (int k = 0; k < K; ++k) u.kp_mirror[k] = cfg->kp_mirror[k];
        const long long blocks = (std::max(u.total, u.n_keys) + 255) / 256;
        if (blocks > 0x7fffffff) return ppn::fail(PPN_E_UNSUPPORTED, "ppn_tta_merge: %lld unary values", u.total);
        tta_unary_kernel<<<(unsigned)blocks, 256, 0, st>>>(u);
        PPN_LAUNCH_CHECK();
    }
    if (E == 0) return PPN_OK;
    const int threads = (p.Q * p.NS + 63) / 64 * 64;
    const size_t lds = (size_t)p.NS * p.Q * V * sizeof(unsigned long long);        // Q * NS <= 1024: at most 32 KB
    const dim3 grid((unsigned)(E * SS), (unsigned)batch, (unsigned)CG);
    if (V == 4)
        hipLaunchKernelGGL(tta_limb_kernel<4>, grid, dim3(threads), lds, st, p);
    else
        hipLaunchKernelGGL(tta_limb_kernel<1>, grid, dim3(threads), lds, st, p);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_tta_stage(const void* src, void* dst, int64_t rows, int32_t width, int32_t elem_bytes, void* stream) {
    if (!src || !dst) return ppn::fail(PPN_E_INVALID, "ppn_tta_stage: NULL pointer");
    if (elem_bytes != 3 && elem_bytes != 4)
        return ppn::fail(PPN_E_INVALID, "ppn_tta_stage: elem_bytes %d (3: u8 RGB pixels, 4: f32)", elem_bytes);
    if (rows < 0 || width < 1 || rows > (1ll << 40) / width)
        return ppn::fail(PPN_E_INVALID, "ppn_tta_stage: %lld rows of %d elements", (long long)rows, width);
    if (rows == 0) return PPN_OK;
    const size_t bytes = (size_t)rows * width * elem_bytes;
    if (overlaps(src, bytes, dst, 2 * bytes)) return ppn::fail(PPN_E_INVALID, "ppn_tta_stage: dst overlaps src");
    if (elem_bytes == 4 && (reinterpret_cast<uintptr_t>(src) % 4 || reinterpret_cast<uintptr_t>(dst) % 4))
        return ppn::fail(PPN_E_INVALID, "ppn_tta_stage: 4-byte elements need 4-byte aligned pointers");
    const long long blocks = (rows * width + 255) / 256;
    if (blocks > 0x7fffffff) return ppn::fail(PPN_E_UNSUPPORTED, "ppn_tta_stage: %lld elements", (long long)rows * width);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (elem_bytes == 4)
        tta_stage_kernel<uint32_t, 1><<<(unsigned)blocks, 256, 0, st>>>(static_cast<const uint32_t*>(src),
                                                                          static_cast<uint32_t*>(dst), rows, width);
    else
        tta_stage_kernel<uint8_t, 3><<<(unsigned)blocks, 256, 0, st>>>(static_cast<const uint8_t*>(src),
                                                                         static_cast<uint8_t*>(dst), rows, width);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
