// Split-K convolution for launches too small to fill the GPU (ppn_conv_desc.flags & PPN_CONV_SPLIT_K; batch 1-4 inference).
//
// The large-tile kernel prices a launch by whole rounds of 256 CUs: with fewer tiles than CUs every workgroup walks the
// whole GEMM depth alone while most CUs idle (a 512 -> 512 3x3 layer at 24 x 24 and batch 1: 20 workgroups x 72 K steps).
// Here the depth is cut into slabs of kSlabElems (splitk_partition.h) and the launch becomes two:
//
//   1. conv_splitk_partial_kernel: grid = pixel tiles x channel tiles x slabs.  Same implicit GEMM, same packed weights
//      (ppn_conv_tiling: tap-major for Cout < 64, channel-chunk-major above), same staging and MFMA sequence as
//      conv_igemm_kernel (conv.hip) over ITS K steps; the f32 accumulator tile goes to workspace[slab][pixel][cout_pad]
//      with plain 16-byte stores.  No atomics.
//   2. conv_splitk_reduce_kernel: sums the slabs in the fixed order 0 .. S-1 and applies the epilogue of ppn_conv_desc
//      (scale1/shift1/act1, residual, out_raw, out_act = act2(scale2 * raw + shift2), 16-bit stores incl. PPN_CONV_OUT_BF16)
//      with the operation order of conv_igemm_kernel's epilogue.
//
// Two launches on one stream: no spin-wait and no cross-workgroup ordering, so nothing can hang, and a captured plan stays
// one chain.  Determinism: the partition is a function of K alone, every workspace element is written by exactly one
// workgroup and summed in one order, so a result depends neither on the grid nor on what runs beside it; image i of a batch
// gets bit for bit what it gets alone.
#include "conv_common.h"
#include "launchers.h"

namespace {

using namespace ppnconv;
using namespace ppnsplitk;

struct SplitKArgs {
    float* ws;            // [slabs][M][cout_pad] f32
    int cout_pad;
    int steps_per_slab;
    int korder1;          // packed depth order: 1 channel-chunk-major (k_order 1), 0 tap-major (k_order 0)
    int slabs;
};

// BP x BC accumulator tile per 256-thread workgroup over the K steps of slab blockIdx.y; WP x WC waves.  Cin % BK == 0.
template <typename T, int BP, int BC, int WP, int WC>
__global__ void __launch_bounds__(256) conv_splitk_partial_kernel(ConvKArgs a, SplitKArgs k) {
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BK = 8 * EPC;                    // 128-byte rows
    constexpr int ES = sizeof(T);
    constexpr int NXI = BP / 32;                   // activation-tile load instructions per thread
    constexpr int NWI = BC / 32;                   // weight-tile load instructions per thread
    constexpr int TP = BP / WP / 16, TC = BC / WC / 16;
    constexpr int STAGE = (BP + BC) * 128;         // bytes per stage buffer
    static_assert(WP * WC == 4, "4 waves");
    static_assert(TP >= 1 && TC >= 1 && BC % 32 == 0, "tile too small");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wp = wave / WC, wc = wave % WC;
    const int slab = blockIdx.y;

    // XCD-aware tile order as in conv_igemm_kernel: consecutive logical tiles share an L2
    int ptile, ctile;
    {
        const int nb = gridDim.x, id = blockIdx.x;
        const int xcd = id & 7, loc = id >> 3, q = nb >> 3, r = nb & 7;
        const int logical = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
        ptile = fast_div(logical, a.div_nct);
        ctile = logical - ptile * a.n_ctiles;
    }
    const int m0 = ptile * BP, c0 = ctile * BC;

    // ---- per-lane loader state (LDS slot (row, s) holds global chunk s ^ ((row>>1)&7)) --------------------------
    const int lrow = lane >> 3;
    const int chunk = (lane & 7) ^ (((lane >> 4) & 3) | ((wave & 1) << 2));
    const int ntaps = a.ks * a.ks;
    int xbase[NXI];
    unsigned xmask[NXI];
#pragma unroll
    for (int j = 0; j < NXI; ++j) {
        const int row = (j * 4 + wave) * 8 + lrow;
        const int m = m0 + row;
        const bool vm = m < a.M;
        const int mm = vm ? m : 0;
        const int b = fast_div(mm, a.div_howo), rem = mm - b * a.HoWo;
        const int oy = fast_div(rem, a.div_wo), ox = rem - oy * a.Wo;
        const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
        xbase[j] = ((b * a.H + iy0) * a.W + ix0) * a.Cin;
        unsigned mk = 0, cx = 0;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
            cx |= (dx < a.ks && (unsigned)(ix0 + dx * a.dil) < (unsigned)a.W) ? (1u << dx) : 0u;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
            mk |= (dy < a.ks && (unsigned)(iy0 + dy * a.dil) < (unsigned)a.H) ? (cx << (dy * a.ks)) : 0u;
        xmask[j] = vm ? mk : 0u;                   // a pixel past M gathers the zero page and is never stored
    }
    const char* wptr[NWI];
#pragma unroll
    for (int j = 0; j < NWI; ++j) {
        const int row = (j * 4 + wave) * 8 + lrow;  // c0 + row < cout_pad: BC divides cout_pad
        wptr[j] = a.wgt + ((size_t)(c0 + row) * a.Ktot + chunk * EPC) * ES;
    }

    const int nsteps = a.Ktot / BK;
    const int s_begin = slab * k.steps_per_slab;
    const int s_end = min(s_begin + k.steps_per_slab, nsteps);
    // (tap, first channel) of K step s_begin; then advanced step by step in the packed order
    const int cpt = a.Cin / BK;                    // K steps per tap
    int u_tap, u_ci0;
    if (k.korder1) { u_tap = s_begin % ntaps; u_ci0 = (s_begin / ntaps) * BK; }
    else { u_tap = s_begin / cpt; u_ci0 = (s_begin % cpt) * BK; }

    auto issue_loads = [&](int step, int buf) {
        char* xs = smem + buf * STAGE;
        char* ws = xs + BP * 128;
        const int dy = u_tap >= 6 ? 2 : (u_tap >= 3 ? 1 : 0);          // ks == 3; a 1x1 has tap 0 only
        const int dx = u_tap - dy * 3;
        const int tapoff = (dy * a.dil * a.W + dx * a.dil) * a.Cin + u_ci0 + chunk * EPC;
#pragma unroll
        for (int j = 0; j < NXI; ++j) {
            const bool ok = (xmask[j] >> u_tap) & 1u;
            const char* g = ok ? a.src + (ptrdiff_t)(xbase[j] + tapoff) * ES : a.zero;
            glds16(g, xs + (j * 4 + wave) * 1024);
        }
        if (k.korder1) {
            if (++u_tap == ntaps) { u_tap = 0; u_ci0 += BK; }
        } else {
            u_ci0 += BK;
            if (u_ci0 >= a.Cin) { u_ci0 = 0; ++u_tap; }
        }
#pragma unroll
        for (int j = 0; j < NWI; ++j) glds16(wptr[j] + (size_t)step * BK * ES, ws + (j * 4 + wave) * 1024);
    };

    // ---- per-lane fragment read offsets --------------------------------------------------------------------------
    const int frow = lane & 15, fq = lane >> 4;
    const int fswz = (frow >> 1) & 7;
    int foff[2];
    foff[0] = frow * 128 + (((0 + fq) ^ fswz) << 4);
    foff[1] = frow * 128 + (((4 + fq) ^ fswz) << 4);
    const int x_tile_off = wp * (BP / WP) * 128;
    const int w_tile_off = BP * 128 + wc * (BC / WC) * 128;

    f32x4 acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int j = 0; j < TP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    issue_loads(s_begin, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int s = s_begin; s < s_end; ++s) {
        const int buf = (s - s_begin) & 1;
        if (s + 1 < s_end) issue_loads(s + 1, buf ^ 1);
        const char* xs = smem + buf * STAGE + x_tile_off;
        const char* ws = smem + buf * STAGE + w_tile_off;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            f32x4 wf[TC], xf[TP];
#pragma unroll
            for (int i = 0; i < TC; ++i) wf[i] = *reinterpret_cast<const f32x4*>(ws + i * 16 * 128 + foff[ks]);
#pragma unroll
            for (int j = 0; j < TP; ++j) xf[j] = *reinterpret_cast<const f32x4*>(xs + j * 16 * 128 + foff[ks]);
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < TP; ++j) mma_step(acc[i][j], wf[i], xf[j], (T*)nullptr);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ---- the accumulators as they are: each lane holds 4 consecutive channels of one pixel = one 16-byte store ------
    float* wsp = k.ws + (size_t)slab * (size_t)a.M * k.cout_pad;
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int j = 0; j < TP; ++j) {
            const int m = m0 + wp * (BP / WP) + j * 16 + frow;
            const int ch = c0 + wc * (BC / WC) + i * 16 + 4 * fq;     // ch + 3 < c0 + BC <= cout_pad
            if (m < a.M) *reinterpret_cast<f32x4*>(wsp + (size_t)m * k.cout_pad + ch) = acc[i][j];
        }
}

// One thread per (pixel, 8 channels): sum of the slabs in the order 0 .. S-1, then conv_igemm_kernel's NHWC epilogue.
// T: the launch's dtype (residual loads); OB: outputs stored as bf16 (PPN_CONV_OUT_BF16, T = _Float16).
template <typename T, bool OB>
__global__ void __launch_bounds__(256) conv_splitk_reduce_kernel(ConvKArgs a, SplitKArgs k) {
    constexpr int ES = sizeof(T);
    const int cgs = a.Cout >> 3;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)a.M * cgs;
    if (idx >= total) return;
    const int m = (int)(idx / cgs), c = (int)(idx - (long long)m * cgs) * 8;
    const size_t slab_stride = (size_t)a.M * k.cout_pad;
    const float* p = k.ws + (size_t)m * k.cout_pad + c;
    float v[8];
    load8<float>(reinterpret_cast<const char*>(p), v);
    for (int s = 1; s < k.slabs; ++s) {
        float t[8];
        load8<float>(reinterpret_cast<const char*>(p + (size_t)s * slab_stride), t);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += t[i];
    }
    // none / ReLU / LeakyReLU(0.1) as  max(t, t * slope)  with slope 1 / 0 / 0.1 (the NHWC path has no sigmoid)
    const float slope1 = a.act1 == PPN_ACT_RELU ? 0.f : (a.act1 == PPN_ACT_LRELU ? 0.1f : 1.f);
    const float slope2 = a.act2 == PPN_ACT_RELU ? 0.f : (a.act2 == PPN_ACT_LRELU ? 0.1f : 1.f);
    const size_t off = ((size_t)m * a.Cout + c) * ES;                  // outputs have the element size of T either way
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float s1 = a.scale1 ? a.scale1[c + i] : 1.f, b1 = a.shift1 ? a.shift1[c + i] : 0.f;
        const float t1 = v[i] * s1 + b1;
        v[i] = fmaxf(t1, t1 * slope1);
    }
    if (a.residual) {
        float r[8];
        load8<T>(a.residual + off, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += r[i];
    }
    if (a.out_raw) {
        if (OB) store8<__bf16>(a.out_raw + off, v);
        else store8<T>(a.out_raw + off, v);
    }
    if (a.out_act) {
        float u[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float s2 = a.scale2 ? a.scale2[c + i] : 1.f, b2 = a.shift2 ? a.shift2[c + i] : 0.f;
            const float t2 = v[i] * s2 + b2;
            u[i] = fmaxf(t2, t2 * slope2);
        }
        if (OB) store8<__bf16>(a.out_act + off, u);
        else store8<T>(a.out_act + off, u);
    }
}

template <typename T>
int launch_partial(const ConvKArgs& a, const SplitKArgs& k, hipStream_t st) {
    constexpr int BP = kTileP, BC = kTileC;
    auto fn = conv_splitk_partial_kernel<T, BP, BC, 2, 2>;
    constexpr int lds = 2 * (BP + BC) * 128;
    static int max_lds_set = 0;
    PPN_LDS_ONCE(max_lds_set, reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(fn, dim3(a.n_ctiles * a.n_ptiles, k.slabs), dim3(256), lds, st, a, k);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

template <typename T, bool OB>
int launch_reduce(const ConvKArgs& a, const SplitKArgs& k, hipStream_t st) {
    const long long total = (long long)a.M * (a.Cout >> 3);
    hipLaunchKernelGGL((conv_splitk_reduce_kernel<T, OB>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, k);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

}  // namespace

// the segment's scope checks, partition and kernel arguments come from conv_route.cpp
int ppn::splitk_launch(const ppn_conv_desc* d, const ConvSegment& s, hipStream_t st) {
    const ConvKArgs& a = s.args;
    SplitKArgs k;
    k.ws = static_cast<float*>(d->splitk_ws);
    k.cout_pad = d->cout_pad;
    k.steps_per_slab = s.splitk.steps_per_slab;
    k.korder1 = d->cout >= 64 ? 1 : 0;             // ppn_conv_tiling: the large-tile layers' packs are channel-chunk-major
    k.slabs = s.splitk.slabs;
    int rc;
    if (d->dtype == PPN_F32) rc = launch_partial<float>(a, k, st);
    else if (d->dtype == PPN_F16) rc = launch_partial<_Float16>(a, k, st);
    else rc = launch_partial<__bf16>(a, k, st);
    if (rc != PPN_OK) return rc;
    if (d->dtype == PPN_F32) return launch_reduce<float, false>(a, k, st);
    if (d->dtype == PPN_BF16) return launch_reduce<__bf16, false>(a, k, st);
    return a.out_bf16 ? launch_reduce<_Float16, true>(a, k, st) : launch_reduce<_Float16, false>(a, k, st);
}
