// Shared device helpers of the fused implicit-GEMM convolution kernels (conv.hip, conv_big.hip, conv_splitk.hip, conv_head.hip,
// conv64.hip); the argument structs the host fills are in conv_args.h.
#pragma once
#include <hip/hip_bf16.h>

#include "common.h"
#include "conv_args.h"

namespace ppnconv {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;

// n / d for the divider make_fastdiv(d) built on the host (conv_args.h)
__device__ __forceinline__ int fast_div(int n, const FastDiv& f) {   // n >= 0
    const unsigned t = __umulhi(f.mul, (unsigned)n);
    return (int)((t + (((unsigned)n - t) >> f.sh1)) >> f.sh2);
}

template <typename T>
struct Elem;
template <>
struct Elem<float> {
    static constexpr int EPC = 4;  // elements per 16-byte chunk
};
template <>
struct Elem<__bf16> {
    static constexpr int EPC = 8;
};
template <>
struct Elem<_Float16> {
    static constexpr int EPC = 8;
};

// sigmoid as exp + reciprocal instructions (v_exp_f32, v_rcp_f32: ~1 ulp each, far inside the 1e-4 head tolerance);
// every head value -- materialised or folded into arg-max keys -- goes through this one function.
__device__ __forceinline__ float sigmoid_fast(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

__device__ __forceinline__ float apply_act(float v, int act) {
    switch (act) {
        case PPN_ACT_RELU: return v > 0.f ? v : 0.f;
        case PPN_ACT_LRELU: return v > 0.f ? v : v * 0.1f;      // nn.LeakyReLU(0.1), model.py:88
        case PPN_ACT_SIGMOID: return sigmoid_fast(v);
        default: return v;
    }
}

__device__ __forceinline__ void glds16(const char* gptr, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)gptr,
                                     (void __attribute__((address_space(3)))*)lds_wave_base, 16, 0, 0);
}

// One K-substep (4 chunks = 128 B/4 of a row): acc += Wfrag x Xfrag
__device__ __forceinline__ void mma_step(f32x4& acc, const f32x4& wf, const f32x4& xf, float*) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.x, xf.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.y, xf.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.z, xf.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf.w, xf.w, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma_step(f32x4& acc, const f32x4& wf, const f32x4& xf, __bf16*) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf), __builtin_bit_cast(bf16x8, xf),
                                                  acc, 0, 0, 0);
}

__device__ __forceinline__ void mma_step(f32x4& acc, const f32x4& wf, const f32x4& xf, _Float16*) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wf), __builtin_bit_cast(f16x8, xf), acc, 0, 0, 0);
}

template <typename T>
__device__ __forceinline__ void load8(const char* p, float* v);
template <>
__device__ __forceinline__ void load8<float>(const char* p, float* v) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 16);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <>
__device__ __forceinline__ void load8<__bf16>(const char* p, float* v) {
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    const unsigned u[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __uint_as_float(u[i] << 16);
        v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
}
template <>
__device__ __forceinline__ void load8<_Float16>(const char* p, float* v) {
    const f16x8 a = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)a[i];
}
// IEEE half overflows to +-inf past 65504; the f16 mode stores RAW pre-activation residual streams, and one inf becomes
// a NaN in the next residual add / BN affine and a garbage decode.  Every f16 store path clamps to the largest finite
// half instead (one v_med3_f32; a NaN stays a NaN).
__device__ __forceinline__ float clamp_f16(float v) { return __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f); }

template <typename T>
__device__ __forceinline__ void store8(char* p, const float* v);
template <>
__device__ __forceinline__ void store8<float>(char* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(p + 16) = make_float4(v[4], v[5], v[6], v[7]);
}
template <>
__device__ __forceinline__ void store8<__bf16>(char* p, const float* v) {
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i];                 // RNE, v_cvt_pk_bf16_f32
    *reinterpret_cast<bf16x8*>(p) = o;
}

template <>
__device__ __forceinline__ void store8<_Float16>(char* p, const float* v) {
    f16x8 o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (_Float16)clamp_f16(v[i]);    // RNE (v_cvt_f16_f32) on a value held inside the finite range
    *reinterpret_cast<f16x8*>(p) = o;
}

// PPN_F16X3 storage: a value v as the half pair (hi, lo') = (half(v), half((v - hi) * 2^11)); lo' is kept at hi's
// magnitude so that it never falls into the half subnormals while hi is normal.  `lo_bytes`: distance hi -> lo' block.
constexpr float kX3LoScale = 2048.f, kX3LoInv = 1.f / 2048.f;
__device__ __forceinline__ void store8_x3(char* p, size_t lo_bytes, const float* v) {
    f16x8 h, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = (_Float16)clamp_f16(v[i]);
        l[i] = (_Float16)clamp_f16((v[i] - (float)h[i]) * kX3LoScale);   // the difference is exact in f32; |.| <= ulp(hi)/2 * 2^11
    }
    *reinterpret_cast<f16x8*>(p) = h;
    *reinterpret_cast<f16x8*>(p + lo_bytes) = l;
}
__device__ __forceinline__ void load8_x3(const char* p, size_t lo_bytes, float* v) {
    const f16x8 h = *reinterpret_cast<const f16x8*>(p), l = *reinterpret_cast<const f16x8*>(p + lo_bytes);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i] + (float)l[i] * kX3LoInv;
}

}  // namespace ppnconv
