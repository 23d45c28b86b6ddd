// DRN-D stem in ONE kernel, split-f16 ("x3") arithmetic: the fused stem of csrc/stem012.hip at the accuracy of the exact
// modes (float16x3, float16 with an exact prefix).  layer0 7x7 3->16 + BN + ReLU, layer1 3x3 16->16 + BN + ReLU, layer2 3x3
// stride 2 16->32 + BN + ReLU (drn.py:123-133), input normalisation fused, second output relu(raw * s3 + b3); outputs f32
// NHWC [B, Ho, Wo, 32] -- what the three exact-f32 launches write.
//
// Numerical contract = a PPN_F16X3 convolution (csrc/conv_big.hip, X3): every activation that stays on chip is the half pair
// (hi, lo') = (half(v), half((v - hi) * 2^11)); every weight likewise, after a per-layer power of two ws = w * 2^s (s chosen
// here from the layer's largest |w|, so that no lo' part falls into the half subnormals); products a_hi w_hi + a_hi w_lo +
// a_lo w_hi on v_mfma_f32_16x16x32_f16 with f32 accumulation (the dropped lo x lo term is 2^-22 relative).  Two accumulators
// per output tile: `m` takes hi x hi, `c` the two cross terms (both carry the 2^11 of their lo' operand), v = (m + c 2^-11)
// 2^-s; BN and ReLU in f32 on that.  u8 frames keep stem012.hip's exact-input scheme: the patch holds the integer x - 128
// (exact in half) and a fourth "inside the image" channel, the normalisation is folded into layer 0's weights, so layer 0
// needs only the two weight halves.  f32 NCHW input is split into pairs like the rings.
//
// Same walk as stem012.hip (a workgroup owns 16 layer-2 rows x 48 layer-2 columns, chunks of 2 layer-2 rows, rolling
// rings), with pair-valued rings: a (plane, pixel) slot holds 16 bytes [hi of 4 channels | lo' of 4 channels], so one
// ds_read_b128 brings a lane both halves and layer 1 / layer 2 issue as many LDS reads per pixel as the 16-bit kernel.  The
// layer-1 ring keeps even and odd pixels apart (layer 2 reads it with stride 2: contiguous 16-byte slots per 16 lanes).
// 2 x 88 VGPRs of split weights: one workgroup of 4 waves per CU (one wave per SIMD, the unified 512-entry register file).
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

constexpr int SW2 = 48;                 // layer-2 columns per strip
constexpr int BAND2 = 16;               // layer-2 rows per work unit
constexpr int NS = 7;                   // 16-pixel segments per layer-0 / layer-1 row
constexpr int W1 = NS * 16;             // layer-1 columns held: x1 = 2*C2 - 1 + i
constexpr int W0 = W1 + 8;              // layer-0 columns held: x0 = 2*C2 - 2 + i
constexpr int WI = W1 + 8;              // input columns held:   xi = 2*C2 - 5 + i
constexpr int HP = W1 / 2;              // layer-1 ring: pixels per parity half (56 = 8 mod 16: the two halves of a 16-lane write
                                        // land on opposite 128-byte halves of the banks)
constexpr int R0 = 6, R1 = 5, RI = 10;  // ring / patch rows
constexpr int RAWS = 368;               // raw u8 row: 120 px x 3 B (+ alignment slack), a multiple of 16
constexpr int LDS_IN = RI * WI * 16;    // patch [RI][WI] x (u8: 8 B = 4 halves; f32: 16 B = hi4 | lo4)
constexpr int LDS_L0 = R0 * 4 * W0 * 16;        // layer-0 ring [row][plane q][pixel] x (hi4 | lo4)
constexpr int LDS_L1 = R1 * 4 * 2 * HP * 16;    // layer-1 ring [row][plane q][parity][pixel / 2] x (hi4 | lo4)
constexpr int LDS_RAW = RI * RAWS;
constexpr int LDS_CST = 4 * 32 * 4 + 16;        // layer-2 epilogue constants [scale2 * 2^-s2 | shift2 | scale3 | shift3][32], max |w| x 3
constexpr int OFF_L0 = LDS_IN, OFF_L1 = OFF_L0 + LDS_L0, OFF_RAW = OFF_L1 + LDS_L1, OFF_CST = OFF_RAW + LDS_RAW;
constexpr int LDS_BYTES = OFF_CST + LDS_CST;
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup per CU");

struct StemX3Args {
    const void* src;                    // u8 [B,H,W,3] or f32 [B,3,H,W]
    const float *w0, *s0, *b0;          // [16][3][7][7], folded BN scale / shift [16]
    const float *w1, *s1, *b1;          // [16][16][3][3], [16]
    const float *w2, *s2, *b2;          // [32][16][3][3], [32]
    const float *s3, *b3;               // second output: relu(v * s3 + b3)  (NULL: no second output)
    float* out_raw;                     // NHWC f32 [B,Ho,Wo,32] or NULL
    float* out_act;                     // NHWC f32 [B,Ho,Wo,32] or NULL
    int B, H, W, Ho, Wo;
    float mean[3], stdv[3];
    int nstrips, nbands;
};

template <typename F, int... I>
__device__ __forceinline__ void sfor_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void sfor(F&& f) {
    sfor_impl(f, std::make_integer_sequence<int, N>{});
}

// single LDS reads the compiler can neither merge nor move: their waits are explicit
template <int OFF>
__device__ __forceinline__ u32x2 lds_read64(unsigned addr) {
    u32x2 v;
    asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <int OFF>
__device__ __forceinline__ u32x4 lds_read128(unsigned addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}

__device__ __forceinline__ f32x4 mfma(f16x8 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

constexpr float kLoScale = 2048.f, kLoInv = 1.f / 2048.f;

__device__ __forceinline__ _Float16 half_hi(float v) { return (_Float16)fminf(fmaxf(v, -65504.f), 65504.f); }
__device__ __forceinline__ _Float16 half_lo(float v, _Float16 hi) { return (_Float16)((v - (float)hi) * kLoScale); }

// BN + ReLU of the pair of accumulator tiles -> 16 bytes [hi of 4 channels | lo' of 4 channels] (zero where !inside)
__device__ __forceinline__ u32x4 bn_relu_pair(const f32x4& m, const f32x4& c, const float (&sc)[4], const float (&sh)[4],
                                              bool inside) {
    f16x4 h, l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float t = fmaf(c[r], kLoInv, m[r]) * sc[r] + sh[r];
        const float v = t > 0.f ? t : 0.f;
        h[r] = half_hi(v);
        l[r] = half_lo(v, h[r]);
    }
    const u32x2 ph = __builtin_bit_cast(u32x2, h), pl = __builtin_bit_cast(u32x2, l);
    u32x4 p = {ph.x, ph.y, pl.x, pl.y};
    if (!inside) p = u32x4{0u, 0u, 0u, 0u};
    return p;
}

// the 2^s of a layer whose largest |w| is `wmax`: wmax * 2^s in [2^14, 2^15)
__device__ __forceinline__ int weight_scale_log2(float wmax) {
    if (!(wmax > 0.f)) return 0;
    int e;
    (void)frexpf(wmax, &e);             // wmax = m 2^e, m in [0.5, 1)
    return 15 - e;
}

template <bool U8>
__global__ void __launch_bounds__(256, 1) stem012_x3_kernel(StemX3Args a) {
    constexpr int PX = U8 ? 8 : 16;     // bytes per patch pixel
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* in_p = smem;
    char* l0_p = smem + OFF_L0;
    char* l1_p = smem + OFF_L1;
    char* raw_p = smem + OFF_RAW;
    float* cst_p = reinterpret_cast<float*>(smem + OFF_CST);
    unsigned* wmax_p = reinterpret_cast<unsigned*>(smem + OFF_CST + 4 * 32 * 4);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ch = lane & 15, g = lane >> 4, col = lane & 15;

    // ---- split weights as MFMA A fragments (rows = output channels), k layout of stem012.hip ----------------------
    f16x8 wh0[7], wl0[7];                 // per dy: k = (dx = 2g + (i>>2), c = i&3)
    f16x8 wh1[5], wl1[5];                 // k-step kk: k = 8g+i -> tap 2kk + (g>>1), ci = (g&1)*8 + i
    f16x8 wh2[2][5], wl2[2][5];
    int sw0, sw1, sw2;                    // per-layer weight scale 2^s
    {
        float* wl = reinterpret_cast<float*>(smem);      // [16*147 | 16*144 | 32*144] f32 over the not-yet-used patch + rings
        constexpr int N0 = 16 * 147, N1 = 16 * 144, N2 = 32 * 144;
        static_assert((N0 + N1 + N2) * 4 <= OFF_RAW, "weight staging must fit below the raw rows");
        if (tid < 3) wmax_p[tid] = 0u;
        for (int i = tid; i < N0; i += 256) wl[i] = a.w0[i];
        for (int i = tid; i < N1; i += 256) wl[N0 + i] = a.w1[i];
        for (int i = tid; i < N2; i += 256) wl[N0 + N1 + i] = a.w2[i];
        __syncthreads();
        // layer 0's EFFECTIVE weights: w / std_c and the mean term sum_c w_c (128 - mean_c) / std_c (u8), or w (f32 input)
        auto w0_eff = [&](int co, int c, int dy, int dx) -> float {
            const float* wc = wl + co * 3 * 49;
            if constexpr (U8) {
                if (c < 3) return wc[(c * 7 + dy) * 7 + dx] / a.stdv[c];
                float v = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) v += wc[(k * 7 + dy) * 7 + dx] * ((128.f - a.mean[k]) / a.stdv[k]);
                return v;
            } else {
                return c < 3 ? wc[(c * 7 + dy) * 7 + dx] : 0.f;
            }
        };
        float m0 = 0.f, m1 = 0.f, m2 = 0.f;
        for (int i = tid; i < 16 * 4 * 49; i += 256) {
            const int co = i / 196, r = i % 196, c = r / 49, t = r % 49;
            m0 = fmaxf(m0, fabsf(w0_eff(co, c, t / 7, t % 7)));
        }
        for (int i = tid; i < N1; i += 256) m1 = fmaxf(m1, fabsf(wl[N0 + i]));
        for (int i = tid; i < N2; i += 256) m2 = fmaxf(m2, fabsf(wl[N0 + N1 + i]));
        atomicMax(&wmax_p[0], __float_as_uint(m0));      // non-negative floats order like their bit patterns
        atomicMax(&wmax_p[1], __float_as_uint(m1));
        atomicMax(&wmax_p[2], __float_as_uint(m2));
        __syncthreads();
        sw0 = weight_scale_log2(__uint_as_float(wmax_p[0]));
        sw1 = weight_scale_log2(__uint_as_float(wmax_p[1]));
        sw2 = weight_scale_log2(__uint_as_float(wmax_p[2]));
        auto split = [](f16x8& hv, f16x8& lv, int i, float w, int s) {
            const float ws = ldexpf(w, s);
            const _Float16 h = (_Float16)ws;
            hv[i] = h;
            lv[i] = half_lo(ws, h);
        };
#pragma unroll
        for (int dy = 0; dy < 7; ++dy)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int dx = 2 * g + hf;
                const bool ok = dx < 7;
                const int dxc = ok ? dx : 6;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float v = ok ? w0_eff(ch, c, dy, dxc) : 0.f;
                    split(wh0[dy], wl0[dy], 4 * hf + c, v, sw0);
                }
            }
        const float* wd = wl + N0 + ch * 16 * 9;
#pragma unroll
        for (int kk = 0; kk < 5; ++kk) {
            const int tap = 2 * kk + (g >> 1), tapc = tap < 9 ? tap : 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = wd[((g & 1) * 8 + i) * 9 + tapc];
                split(wh1[kk], wl1[kk], i, tap < 9 ? v : 0.f, sw1);
            }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const float* we = wl + N0 + N1 + (ct * 16 + ch) * 16 * 9;
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) {
                const int tap = 2 * kk + (g >> 1), tapc = tap < 9 ? tap : 8;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float v = we[((g & 1) * 8 + i) * 9 + tapc];
                    split(wh2[ct][kk], wl2[ct][kk], i, tap < 9 ? v : 0.f, sw2);
                }
            }
        }
    }
    // BN scales carry the weights' 2^-s (a power of two: exact); layer 2's constants wait in LDS
    float sc0[4], sh0[4], sc1[4], sh1[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc0[r] = ldexpf(a.s0[4 * g + r], -sw0); sh0[r] = a.b0[4 * g + r];
        sc1[r] = ldexpf(a.s1[4 * g + r], -sw1); sh1[r] = a.b1[4 * g + r];
    }
    if (tid < 128) {
        const int c = tid & 31, which = tid >> 5;
        float v;
        if (which == 0) v = ldexpf(a.s2[c], -sw2);
        else if (which == 1) v = a.b2[c];
        else if (which == 2) v = a.s3 ? a.s3[c] : 1.f;
        else v = a.b3 ? a.b3[c] : 0.f;
        cst_p[tid] = v;
    }
    // per-lane tap geometry of the 3x3 k-steps: tap t = 2kk + (g>>1) -> (dy, dx); the dead half of k-step 4 reads tap 0
    int tdy[5], tdx[5];
#pragma unroll
    for (int kk = 0; kk < 5; ++kk) {
        const int tap = 2 * kk + (g >> 1), t = tap < 9 ? tap : 0;
        tdy[kk] = t / 3; tdx[kk] = t - (t / 3) * 3;
    }
    const unsigned smem_base = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;   // LDS byte address

    const int units = a.B * a.nbands * a.nstrips;
    for (int unit = blockIdx.x; unit < units; unit += gridDim.x) {
        int u = unit;
        const int strip = u % a.nstrips; u /= a.nstrips;
        const int band = u % a.nbands;
        const int b = u / a.nbands;
        const int C2 = strip * SW2, R2 = band * BAND2;
        const int R2e = min(R2 + BAND2, a.Ho);
        const int x0b = 2 * C2 - 2;                    // image column of layer-0 ring column 0
        const int x1b = 2 * C2 - 1;                    // image column of layer-1 ring column 0
        const int xib = 2 * C2 - 5;                    // image column of input patch column 0

        // u8 source: input rows yi0 .. yi0+nrows-1 into the raw buffer by LDS-DMA, as stem012.hip (aligned dwords; rows
        // outside the image are skipped and never looked at)
        const int xs = xib < 0 ? 0 : xib;
        const int nb_row = (min(xib + WI, a.W) - xs) * 3;
        auto request_input = [&](int yi0, int nrows) {
            if constexpr (U8) {
                const unsigned char* base = static_cast<const unsigned char*>(a.src);
                for (int q = wave; q < nrows * 2; q += 4) {
                    const int r = q >> 1, half = q & 1;
                    const int gy = yi0 + r;
                    if (gy < 0 || gy >= a.H) continue;                               // wave-uniform
                    const size_t S = (((size_t)b * a.H + gy) * a.W + xs) * 3;
                    const size_t A = S & ~(size_t)3;
                    const int k = half * 64 + lane;
                    if (k < RAWS / 4 && A + 4 * (size_t)k < S + nb_row)
                        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(base + A + 4 * (size_t)k),
                                                         (void __attribute__((address_space(3)))*)(raw_p + r * RAWS + half * 256),
                                                         4, 0, 0);
                }
            }
        };
        // raw rows (u8) / the f32 image -> patch rows 0 .. nrows-1, zero outside the image (patch row 0 = input row yi0)
        auto convert_input = [&](int yi0, int nrows) {
            if (tid >= 2 * WI) return;
            const int prow = tid >= WI ? 1 : 0, px = tid - prow * WI;
            const int gx = xib + px;
            const bool colok = gx >= 0 && gx < a.W;
            if constexpr (U8) {
                const unsigned base = smem_base + (unsigned)OFF_RAW + prow * RAWS + (colok ? (gx - xs) * 3 : 0);
                const unsigned sh0 = (((unsigned)b * a.H + (unsigned)(yi0 + prow)) * a.W + xs) * 3u;
                const unsigned dsh = 2u * a.W * 3u;
                unsigned v[RI / 2][3];
#pragma unroll
                for (int k = 0; k < RI / 2; ++k) {
                    const unsigned ad = base + 2 * k * RAWS + ((sh0 + k * dsh) & 3u);
                    asm volatile("ds_read_u8 %0, %1" : "=v"(v[k][0]) : "v"(ad));
                    asm volatile("ds_read_u8 %0, %1 offset:1" : "=v"(v[k][1]) : "v"(ad));
                    asm volatile("ds_read_u8 %0, %1 offset:2" : "=v"(v[k][2]) : "v"(ad));
                }
                // the wait is tied to the 15 values (see stem012.hip: an untied wait lets the compiler use them early)
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(v[0][0]), "+v"(v[0][1]), "+v"(v[0][2]), "+v"(v[1][0]), "+v"(v[1][1]), "+v"(v[1][2]),
                               "+v"(v[2][0]), "+v"(v[2][1]), "+v"(v[2][2]), "+v"(v[3][0]), "+v"(v[3][1]), "+v"(v[3][2]),
                               "+v"(v[4][0]), "+v"(v[4][1]), "+v"(v[4][2])::"memory");
                static_assert(RI / 2 == 5, "the wait above names 5 x 3 values");
#pragma unroll
                for (int k = 0; k < RI / 2; ++k) {
                    const int py = prow + 2 * k;
                    if (py >= nrows) break;
                    const int gy = yi0 + py;
                    u32x2 o = {0u, 0u};
                    if (colok && gy >= 0 && gy < a.H) {
                        // the integer x - 128, exact in half; fourth channel: half(1.0) = inside the image
                        f16x4 t;
#pragma unroll
                        for (int c = 0; c < 3; ++c) t[c] = (_Float16)(float)((int)v[k][c] - 128);
                        t[3] = (_Float16)1.f;
                        o = __builtin_bit_cast(u32x2, t);
                    }
                    *reinterpret_cast<u32x2*>(in_p + ((size_t)py * WI + px) * PX) = o;
                }
            } else {
#pragma unroll
                for (int k = 0; k < RI / 2; ++k) {
                    const int py = prow + 2 * k;
                    if (py >= nrows) break;
                    const int gy = yi0 + py;
                    u32x4 o = {0u, 0u, 0u, 0u};
                    if (colok && gy >= 0 && gy < a.H) {
                        const float* sp = static_cast<const float*>(a.src) + ((size_t)b * 3 * a.H + gy) * a.W + gx;
                        const size_t plane = (size_t)a.H * a.W;
                        f16x4 h, l;
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const float x = sp[c * plane];
                            h[c] = half_hi(x);
                            l[c] = half_lo(x, h[c]);
                        }
                        h[3] = l[3] = (_Float16)0.f;
                        const u32x2 ph = __builtin_bit_cast(u32x2, h), pl = __builtin_bit_cast(u32x2, l);
                        o = u32x4{ph.x, ph.y, pl.x, pl.y};
                    }
                    *reinterpret_cast<u32x4*>(in_p + ((size_t)py * WI + px) * PX) = o;
                }
            }
        };
        auto input_landed = [&]() {
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        };
        // layer-0 rows y .. y+nrows-1 (patch row 0 = input row y - 3) -> ring; wave w computes row y + w
        auto layer0 = [&](int y, int nrows) {
            if (wave >= nrows) return;
            const int gy = y + wave;
            const bool rowok = gy >= 0 && gy < a.H;
            const unsigned rd = smem_base + (unsigned)((wave * WI + col + 2 * g) * PX);            // patch (row, col + 2g)
            char* wr = l0_p + ((size_t)(((gy + 2 * R0) % R0) * 4 + g) * W0 + col) * 16;
            if constexpr (U8) {
                // the patch is exact: two products per k-step (w_hi x, w_lo' x); the 14 reads of segment sg + 1 in flight
                // under the MFMA chain of segment sg, as stem012.hip
                u32x2 p0[2][7], p1[2][7];
                auto fetch = [&](auto sgc, auto setc) {
                    constexpr int sg = decltype(sgc)::value, st = decltype(setc)::value;
                    sfor<7>([&](auto dyc) {
                        constexpr int dy = decltype(dyc)::value;
                        p0[st][dy] = lds_read64<dy * WI * PX + sg * 16 * PX>(rd);
                        p1[st][dy] = lds_read64<dy * WI * PX + sg * 16 * PX + PX>(rd);
                    });
                };
                fetch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
                sfor<NS>([&](auto sgc) {
                    constexpr int sg = decltype(sgc)::value, cur = sg & 1;
                    if constexpr (sg + 1 < NS) {
                        fetch(std::integral_constant<int, sg + 1>{}, std::integral_constant<int, cur ^ 1>{});
                        asm volatile("s_waitcnt lgkmcnt(14)" ::: "memory");
                    } else {
                        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 m = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int dy = 0; dy < 7; ++dy) {
                        const u32x4 xb = {p0[cur][dy].x, p0[cur][dy].y, p1[cur][dy].x, p1[cur][dy].y};
                        m = mfma(wh0[dy], xb, m);
                        c = mfma(wl0[dy], xb, c);
                    }
                    const int gx = x0b + sg * 16 + col;
                    *reinterpret_cast<u32x4*>(wr + sg * 256) = bn_relu_pair(m, c, sc0, sh0, rowok && gx >= 0 && gx < a.W);
                });
            } else {
                // f32 input: pair-valued patch, three products per k-step; 14 x 16-byte reads per segment, not pipelined
                // (forward() of a float tensor is not the serving path)
#pragma unroll 1
                for (int sg = 0; sg < NS; ++sg) {
                    u32x4 p0[7], p1[7];
                    sfor<7>([&](auto dyc) {
                        constexpr int dy = decltype(dyc)::value;
                        p0[dy] = lds_read128<dy * WI * PX>(rd + sg * 16 * PX);
                        p1[dy] = lds_read128<dy * WI * PX + PX>(rd + sg * 16 * PX);
                    });
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 m = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int dy = 0; dy < 7; ++dy) {
                        const u32x4 xh = {p0[dy].x, p0[dy].y, p1[dy].x, p1[dy].y};
                        const u32x4 xl = {p0[dy].z, p0[dy].w, p1[dy].z, p1[dy].w};
                        m = mfma(wh0[dy], xh, m);
                        c = mfma(wl0[dy], xh, c);
                        c = mfma(wh0[dy], xl, c);
                    }
                    const int gx = x0b + sg * 16 + col;
                    *reinterpret_cast<u32x4*>(wr + sg * 256) = bn_relu_pair(m, c, sc0, sh0, rowok && gx >= 0 && gx < a.W);
                }
            }
        };
        // layer-1 rows y .. y+nrows-1 from layer-0 rows y-1 .. y+nrows -> ring; wave w computes row y + w
        auto layer1 = [&](int y, int nrows) {
            if (wave >= nrows) return;
            const int gy = y + wave;
            const bool rowok = gy >= 0 && gy < a.H;
            const int s0 = (gy - 1 + 2 * R0) % R0;                        // ring slot of layer-0 row gy - 1
            unsigned rd[5];                                               // LDS byte address of (row, plane 2h, col + dx)
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) {
                int s = s0 + tdy[kk];
                s = s >= R0 ? s - R0 : s;
                rd[kk] = smem_base + (unsigned)(OFF_L0 + ((s * 4 + 2 * (g & 1)) * W0 + col + tdx[kk]) * 16);
            }
            // pixel x = 16 sg + col: parity col & 1, slot 8 sg + col / 2
            char* wr = l1_p + ((size_t)((((gy + 2 * R1) % R1) * 4 + g) * 2 + (col & 1)) * HP + (col >> 1)) * 16;
            u32x4 q0[2][5], q1[2][5];
            auto fetch = [&](auto sgc, auto setc) {
                constexpr int sg = decltype(sgc)::value, st = decltype(setc)::value;
#pragma unroll
                for (int kk = 0; kk < 5; ++kk) {
                    q0[st][kk] = lds_read128<sg * 256>(rd[kk]);
                    q1[st][kk] = lds_read128<sg * 256 + W0 * 16>(rd[kk]);
                }
            };
            fetch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
            sfor<NS>([&](auto sgc) {
                constexpr int sg = decltype(sgc)::value, cur = sg & 1;
                if constexpr (sg + 1 < NS) {
                    fetch(std::integral_constant<int, sg + 1>{}, std::integral_constant<int, cur ^ 1>{});
                    asm volatile("s_waitcnt lgkmcnt(10)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
                __builtin_amdgcn_sched_barrier(0);
                f32x4 m = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 5; ++kk) {
                    const u32x4 xh = {q0[cur][kk].x, q0[cur][kk].y, q1[cur][kk].x, q1[cur][kk].y};
                    const u32x4 xl = {q0[cur][kk].z, q0[cur][kk].w, q1[cur][kk].z, q1[cur][kk].w};
                    m = mfma(wh1[kk], xh, m);
                    c = mfma(wl1[kk], xh, c);
                    c = mfma(wh1[kk], xl, c);
                }
                const int gx = x1b + sg * 16 + col;
                *reinterpret_cast<u32x4*>(wr + sg * 128) = bn_relu_pair(m, c, sc1, sh1, rowok && gx >= 0 && gx < a.W);
            });
        };
        // layer-2 rows oy0 .. oy0+nrows-1 (stride 2) from layer-1 rows 2oy-1 .. -> HBM; waves 0,1 take row 0, waves 2,3
        // row 1: the even wave segments 0 and 1, the odd wave segment 2
        auto layer2 = [&](int oy0, int nrows) {
            const int ry = wave >> 1;
            if (ry >= nrows) return;
            const int oy = oy0 + ry;
            const int s0 = (2 * oy - 1 + 2 * R1) % R1;
            const int sg0 = (wave & 1) * 2, nsg = (wave & 1) ? 1 : 2;
            unsigned rd[5];                                               // (row, plane 2h, parity of dx, pixel / 2)
#pragma unroll
            for (int kk = 0; kk < 5; ++kk) {
                int s = s0 + tdy[kk];
                s = s >= R1 ? s - R1 : s;
                rd[kk] = smem_base + (unsigned)(OFF_L1 + ((((s * 4 + 2 * (g & 1)) * 2 + (tdx[kk] & 1)) * HP) +
                                                          sg0 * 16 + col + (tdx[kk] >> 1)) * 16);
            }
            for (int sg = 0; sg < nsg; ++sg) {
                const int ox = C2 + (sg0 + sg) * 16 + col;
                u32x4 q0[5], q1[5];
#pragma unroll
                for (int kk = 0; kk < 5; ++kk) {
                    q0[kk] = lds_read128<0>(rd[kk] + sg * 256);
                    q1[kk] = lds_read128<2 * HP * 16>(rd[kk] + sg * 256);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                f32x4 m[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
                f32x4 c[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int kk = 0; kk < 5; ++kk) {
                    const u32x4 xh = {q0[kk].x, q0[kk].y, q1[kk].x, q1[kk].y};
                    const u32x4 xl = {q0[kk].z, q0[kk].w, q1[kk].z, q1[kk].w};
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        m[ct] = mfma(wh2[ct][kk], xh, m[ct]);
                        c[ct] = mfma(wl2[ct][kk], xh, c[ct]);
                        c[ct] = mfma(wh2[ct][kk], xl, c[ct]);
                    }
                }
                if (oy < a.Ho && ox < a.Wo) {
                    const size_t pix = ((size_t)b * a.Ho + oy) * a.Wo + ox;
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        const f32x4 sc2 = *reinterpret_cast<const f32x4*>(cst_p + ct * 16 + 4 * g);
                        const f32x4 sh2 = *reinterpret_cast<const f32x4*>(cst_p + 32 + ct * 16 + 4 * g);
                        const f32x4 sc3 = *reinterpret_cast<const f32x4*>(cst_p + 64 + ct * 16 + 4 * g);
                        const f32x4 sh3 = *reinterpret_cast<const f32x4*>(cst_p + 96 + ct * 16 + 4 * g);
                        f32x4 ov, ou;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float t = fmaf(c[ct][r], kLoInv, m[ct][r]) * sc2[r] + sh2[r];
                            const float v = t > 0.f ? t : 0.f;               // BN + ReLU (drn.py:198-200)
                            const float w2 = v * sc3[r] + sh3[r];
                            ov[r] = v;
                            ou[r] = w2 > 0.f ? w2 : 0.f;                     // next block's relu(bn1(x)) (drn.py:45-46)
                        }
                        const size_t o = pix * 32 + ct * 16 + 4 * g;
                        if (a.out_raw) *reinterpret_cast<f32x4*>(a.out_raw + o) = ov;
                        if (a.out_act) *reinterpret_cast<f32x4*>(a.out_act + o) = ou;
                    }
                }
            }
        };

        // ---- warm-up of the band: layer-0 rows 2R2-2 .. 2R2, layer-1 row 2R2-1 (the schedule of stem012.hip) --------
        lds_barrier();                                  // the previous unit's readers are done with every buffer
        request_input(2 * R2 - 5, 9);
        input_landed();
        convert_input(2 * R2 - 5, 9);
        lds_barrier();
        request_input(2 * R2 - 2, RI);
        layer0(2 * R2 - 2, 3);
        lds_barrier();
        layer1(2 * R2 - 1, 1);
        for (int r2 = R2; r2 < R2e; r2 += 2) {
            input_landed();                             // input rows 2r2-2 .. 2r2+7; also: layer1 of the previous chunk done
            convert_input(2 * r2 - 2, RI);
            lds_barrier();
            if (r2 + 2 < R2e) request_input(2 * r2 + 2, RI);
            if (r2 > R2) layer2(r2 - 2, 2);
            layer0(2 * r2 + 1, 4);
            lds_barrier();
            layer1(2 * r2, 4);
        }
        lds_barrier();
        const int last = R2 + ((R2e - R2 - 1) / 2) * 2;
        layer2(last, min(2, R2e - last));
    }
}

}  // namespace

namespace ppn {
template <bool U8>
static int stem012_x3_launch_T(const StemX3Args& a, unsigned grid, hipStream_t st) {
    static int max_lds_set = 0;
    PPN_LDS_ONCE(max_lds_set, reinterpret_cast<const void*>(stem012_x3_kernel<U8>), hipFuncAttributeMaxDynamicSharedMemorySize,
                 LDS_BYTES);
    hipLaunchKernelGGL((stem012_x3_kernel<U8>), dim3(grid), dim3(256), LDS_BYTES, st, a);
    return PPN_OK;
}

// PPN_STEM_IO(PPN_F16X3, PPN_F32): the arguments were checked by stem012_launch (csrc/stem012.hip)
int stem012_x3_launch(int src_is_u8, const void* src, int batch, int h, int w, const float* w0, const float* s0,
                      const float* b0, const float* mean, const float* stdv, const float* w1, const float* s1,
                      const float* b1, const float* w2, const float* s2, const float* b2, const float* s3, const float* b3,
                      void* out_raw, void* out_act, hipStream_t st) {
    StemX3Args a;
    a.src = src; a.w0 = w0; a.s0 = s0; a.b0 = b0; a.w1 = w1; a.s1 = s1; a.b1 = b1; a.w2 = w2; a.s2 = s2; a.b2 = b2;
    a.s3 = s3; a.b3 = b3; a.out_raw = static_cast<float*>(out_raw); a.out_act = static_cast<float*>(out_act);
    a.B = batch; a.H = h; a.W = w;
    a.Ho = (h + 2 - 3) / 2 + 1; a.Wo = (w + 2 - 3) / 2 + 1;
    for (int i = 0; i < 3; ++i) { a.mean[i] = mean ? mean[i] : 0.f; a.stdv[i] = stdv ? stdv[i] : 1.f; }
    a.nstrips = (a.Wo + SW2 - 1) / SW2; a.nbands = (a.Ho + BAND2 - 1) / BAND2;
    const long long units = (long long)batch * a.nstrips * a.nbands;
    if (units > 0x7fffffffLL) return fail(PPN_E_UNSUPPORTED, "too many tiles");
    if ((long long)batch * h * w * 3 > 0xffffffffLL) return fail(PPN_E_UNSUPPORTED, "frames too large for 32-bit byte offsets");
    const unsigned grid = (unsigned)(units < 256 ? units : 256);      // persistent: one workgroup per CU
    const int rc = src_is_u8 ? stem012_x3_launch_T<true>(a, grid, st) : stem012_x3_launch_T<false>(a, grid, st);
    if (rc != PPN_OK) return rc;
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
}  // namespace ppn
