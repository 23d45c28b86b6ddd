// Train-time augmentation on the device (aug.py:13-160, IAA + ToNormalizedTensor): one image kernel and one label kernel
// between raw u8 pictures + annotations and (x, person arrays for csrc/encode.hip).  The host builds, per image, the
// forward map F (source pixel -> output pixel: rotate + scale about the centre, crop, centre-aligned resize) and its
// inverse in float64 and rounds both to f32 [2][3]; the kernels use only those twelve numbers per image (no sin / cos).
//
//   augment_image_kernel   one thread per V adjacent output x of one row: ONE bilinear resampling pass through F^-1
//                          (2^11 fixed-point weights, constant border 0 outside the picture's own valid h x w), u8 NHWC
//                          and / or the normalised f32 NCHW planes.  V = 4: one 16-byte store per plane and lane (a wave
//                          writes 1 KiB contiguous per plane) and three 4-byte stores for the 12 u8 bytes.
//   augment_people_kernel  one workgroup per image, one thread per person: keypoints and head boxes through F, keypoints
//                          outside the frame zeroed, boxes clipped, people without a keypoint dropped by a STABLE
//                          compaction (encode.hip applies people in order), for any pmax (chunks of 256 people).
// Every f32 operation is written out in a fixed order and the file is built with -ffp-contract=off, so the outputs are
// bit-exact with the NumPy restatement tests/augment_ref.py.  HBM-bound: writes 15 bytes per output pixel, reads <= 4
// source pixels (L2 serves the overlap).
//
// Options on top of that (include/ppn.h; NumPy restatement tests/augment_jitter_ref.py), each its own instantiation, so the
// plain kernels keep their arithmetic:
//   COLOR   (ppn_augment_images_color)   saturation, per-channel gain / offset and counter-based splitmix64 noise in i32 on
//                                        the interpolated values, in registers in front of the same stores.
//   MIRROR  (ppn_augment_people_mirror)  in a mirrored image point slot j reads slot kp_mirror[j + 1] - 1 (coordinates and
//                                        visible bit).  The reflection itself is part of F / F^-1: neither kernel knows it.
#include "common.h"

namespace {

struct AugImgArgs {
    const unsigned char* src;    // [B][Hs][Ws][3]
    const int* src_hw;           // [B][2]: valid (h, w) of each picture
    const float* inv;            // [B][2][3]: output pixel -> source pixel
    unsigned char* dst_u8;       // [B][Hd][Wd][3] or NULL
    float* dst_f32;              // [B][3][Hd][Wd] or NULL
    int B, Hs, Ws, Hd, Wd;
    const int* color;            // [B][10] (COLOR instantiations only)
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// splitmix64 output number idx (0-based) of the stream started at key: prng.raw_u64(key, n)[idx]
__device__ __forceinline__ unsigned long long splitmix_at(unsigned long long key, unsigned long long idx) {
    unsigned long long z = key + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// One image's colour parameters, clamped (include/ppn.h).  `>>` on a negative int is an arithmetic shift here.
struct ColorParams {
    int sat, gain[3], off[3], nq;
    unsigned long long key;
};

__device__ __forceinline__ ColorParams load_color(const int* q) {
    ColorParams p;
    p.sat = clampi(q[0], 0, 512);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        p.gain[c] = clampi(q[1 + c], 0, 1024);
        p.off[c] = clampi(q[4 + c], -255, 255);
    }
    p.nq = clampi(q[7], 0, 4096);
    p.key = (unsigned long long)(unsigned int)q[8] | ((unsigned long long)(unsigned int)q[9] << 32);
    return p;
}

__device__ __forceinline__ void color_pixel(const ColorParams& p, unsigned long long idx, int* v) {
    const int y = (77 * v[0] + 150 * v[1] + 29 * v[2] + 128) >> 8;
    unsigned long long z = 0;
    if (p.nq) z = splitmix_at(p.key, idx);                        // nq == 0: d == 0 whatever z is
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int c1 = clampi(y + (((v[c] - y) * p.sat + 128) >> 8), 0, 255);
        const int c2 = ((c1 * p.gain[c] + 128) >> 8) + p.off[c];
        const int t = (int)((z >> (21 * c)) & 0x1FFFFFull);
        const int s = 2 * ((t & 127) + ((t >> 7) & 127) + ((t >> 14) & 127)) - 381;
        const int d = (s * p.nq + (1 << 13)) >> 14;
        v[c] = clampi(c2 + d, 0, 255);
    }
}

__device__ __forceinline__ int tap(const unsigned char* img, int Ws, int h, int w, int y, int x, int c) {
    return (x >= 0 && x < w && y >= 0 && y < h) ? (int)img[((size_t)y * Ws + x) * 3 + c] : 0;
}

template <int V, bool COLOR>
__global__ void __launch_bounds__(256) augment_image_kernel(AugImgArgs a) {
    const int WV = a.Wd / V;
    const long long total = (long long)a.B * a.Hd * WV;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ox0 = (int)(i % WV) * V;
    const int oy = (int)((i / WV) % a.Hd);
    const int b = (int)(i / ((long long)WV * a.Hd));
    const unsigned char* img = a.src + (size_t)b * a.Hs * a.Ws * 3;
    const int h = min(a.src_hw[2 * b], a.Hs), w = min(a.src_hw[2 * b + 1], a.Ws);   // never beyond this image's slot
    const float* m = a.inv + 6 * b;
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
    const float fy = (float)oy;
    int v[V][3];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float fxo = (float)(ox0 + j);
        const float sx = (m00 * fxo + m01 * fy) + m02;
        const float sy = (m10 * fxo + m11 * fy) + m12;
        const float flx = floorf(sx), fly = floorf(sy);
        const int a1 = (int)rintf((sx - flx) * 2048.f), a0 = 2048 - a1;
        const int b1 = (int)rintf((sy - fly) * 2048.f), b0 = 2048 - b1;
        // far-away (or NaN) coordinates: any index whose four taps are all outside gives 0, whatever the weights
        const int ix = (int)fminf(fmaxf(flx, -2.f), (float)a.Ws), iy = (int)fminf(fmaxf(fly, -2.f), (float)a.Hs);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int t0 = tap(img, a.Ws, h, w, iy, ix, c) * a0 + tap(img, a.Ws, h, w, iy, ix + 1, c) * a1;
            const int t1 = tap(img, a.Ws, h, w, iy + 1, ix, c) * a0 + tap(img, a.Ws, h, w, iy + 1, ix + 1, c) * a1;
            v[j][c] = (b0 * t0 + b1 * t1 + (1 << 21)) >> 22;      // <= 255 * 2^22 + 2^21 < 2^31
        }
    }
    if constexpr (COLOR) {
        const ColorParams p = load_color(a.color + 10 * b);
        const unsigned long long idx0 = (unsigned long long)oy * (unsigned long long)a.Wd + (unsigned long long)ox0;
#pragma unroll
        for (int j = 0; j < V; ++j) color_pixel(p, idx0 + j, v[j]);
    }
    if (a.dst_u8) {
        unsigned char* o = a.dst_u8 + (((size_t)b * a.Hd + oy) * a.Wd + ox0) * 3;
        if constexpr (V == 4) {
            unsigned int q[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {                         // bytes 4k .. 4k+3 of the 12: byte n = v[n / 3][n % 3]
                q[k] = 0;
#pragma unroll
                for (int n = 0; n < 4; ++n) q[k] |= (unsigned int)v[(4 * k + n) / 3][(4 * k + n) % 3] << (8 * n);
            }
            unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
            o4[0] = q[0]; o4[1] = q[1]; o4[2] = q[2];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (unsigned char)v[0][c];
        }
    }
    if (a.dst_f32) {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};      // aug.py:139-140
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = a.dst_f32 + (((size_t)b * 3 + c) * a.Hd + oy) * a.Wd + ox0;
            if constexpr (V == 4) {
                *reinterpret_cast<float4*>(o) =
                    make_float4(((float)v[0][c] - mean[c]) / stdv[c], ((float)v[1][c] - mean[c]) / stdv[c],
                                ((float)v[2][c] - mean[c]) / stdv[c], ((float)v[3][c] - mean[c]) / stdv[c]);
            } else {
                o[0] = ((float)v[0][c] - mean[c]) / stdv[c];
            }
        }
    }
}

struct AugPplArgs {
    const float* people;         // [B][pmax][5 + 2*(K-1)]
    const int* visible;          // [B][pmax]
    const int* count;            // [B]
    const float* fwd;            // [B][2][3]: source pixel -> output pixel
    float* people_out;
    int* visible_out;
    int* count_out;
    int B, pmax, K, Hd, Wd;
};

// keypoint k (1-based slot j = k - 1) of person P through F: in frame -> (x', y'), otherwise (0, 0)
__device__ __forceinline__ void map_keypoint(const float* f, float outW, float outH, float x, float y, float* ox, float* oy) {
    *ox = 0.f; *oy = 0.f;
    if (x == 0.f && y == 0.f) return;                             // absent (aug.py:27)
    const float tx = (f[0] * x + f[1] * y) + f[2];
    const float ty = (f[3] * x + f[4] * y) + f[5];
    if (tx >= 0.f && tx < outW && ty >= 0.f && ty < outH) { *ox = tx; *oy = ty; }      // aug.py:69-75
}

struct AugMirror {
    const int* flag;             // [B]: != 0 -> this image is mirrored
    int src[PPN_MAX_KP];         // point slot j reads point slot src[j] = kp_mirror[j + 1] - 1
};

// MIRROR: `m` is read and, in a flagged image, every read of point slot j (coordinates, visible bit) goes to m->src[j].
template <bool MIRROR>
__device__ __forceinline__ void augment_people_body(const AugPplArgs& a, const AugMirror* m) {
    __shared__ int s_keep[256];
    const int b = blockIdx.x, t = threadIdx.x;
    bool flip = false;
    if constexpr (MIRROR) flip = m->flag[b] != 0;
    auto slot = [&](int j) -> int {
        if constexpr (MIRROR) return flip ? m->src[j] : j;
        else return j;
    };
    const int nk = a.K - 1, stride = 5 + 2 * nk;
    const float outW = (float)a.Wd, outH = (float)a.Hd;
    float f[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) f[i] = a.fwd[6 * b + i];
    const int np = min(max(a.count[b], 0), a.pmax);
    const float* Pin = a.people + (size_t)b * a.pmax * stride;
    float* Pout = a.people_out + (size_t)b * a.pmax * stride;
    int kept = 0;                                                 // survivors of the chunks before this one (uniform)
    for (int p0 = 0; p0 < np; p0 += 256) {
        const int p = p0 + t;
        const float* P = Pin + (size_t)p * stride;
        int keep = 0;
        if (p < np) {
            for (int j = 0; j < nk; ++j) {
                float x, y;
                const int sj = slot(j);
                map_keypoint(f, outW, outH, P[5 + 2 * sj], P[6 + 2 * sj], &x, &y);
                keep |= (x != 0.f || y != 0.f) ? 1 : 0;           // aug.py:104: dropped when every value is 0
            }
        }
        s_keep[t] = keep;
        __syncthreads();
        int before = 0, all = 0;
        for (int j = 0; j < 256; ++j) {
            const int k = s_keep[j];
            all += k;
            before += j < t ? k : 0;
        }
        __syncthreads();
        if (keep) {
            float* Q = Pout + (size_t)(kept + before) * stride;
            const int vis_in = a.visible[b * a.pmax + p];
            int vis = vis_in;
            if constexpr (MIRROR) {
                if (flip) {                                       // bit j <- bit src[j]; bits without a slot are copied
                    unsigned int u = (unsigned int)vis_in & ~((1u << nk) - 1u);
                    for (int j = 0; j < nk; ++j) u |= (((unsigned int)vis_in >> m->src[j]) & 1u) << j;
                    vis = (int)u;
                }
            }
            for (int j = 0; j < nk; ++j) {
                float x, y;
                const int sj = slot(j);
                map_keypoint(f, outW, outH, P[5 + 2 * sj], P[6 + 2 * sj], &x, &y);
                Q[5 + 2 * j] = x; Q[6 + 2 * j] = y;
                if (x == 0.f && y == 0.f) vis &= (int)~(1u << j);      // aug.py:108-110; no bit is ever set
            }
            // head box: floor-divided half sizes (aug.py:35-38), four corners through F, min / max, clip (aug.py:84-102)
            const float hw = floorf(P[2] / 2.f), hh = floorf(P[3] / 2.f);
            const float x1 = P[0] - hw, x2 = P[0] + hw, y1 = P[1] - hh, y2 = P[1] + hh;
            const float cx[4] = {x1, x2, x1, x2}, cy[4] = {y1, y1, y2, y2};
            float lx = 0.f, ux = 0.f, ly = 0.f, uy = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float tx = (f[0] * cx[i] + f[1] * cy[i]) + f[2];
                const float ty = (f[3] * cx[i] + f[4] * cy[i]) + f[5];
                lx = i ? fminf(lx, tx) : tx; ux = i ? fmaxf(ux, tx) : tx;
                ly = i ? fminf(ly, ty) : ty; uy = i ? fmaxf(uy, ty) : ty;
            }
            lx = fminf(fmaxf(lx, 0.f), outW); ux = fminf(fmaxf(ux, 0.f), outW);
            ly = fminf(fmaxf(ly, 0.f), outH); uy = fminf(fmaxf(uy, 0.f), outH);
            Q[0] = (lx + ux) / 2.f; Q[1] = (ly + uy) / 2.f; Q[2] = ux - lx; Q[3] = uy - ly;      // aug.py:128-131
            Q[4] = P[4];
            a.visible_out[b * a.pmax + kept + before] = vis;
        }
        kept += all;
    }
    for (int i = kept * stride + t; i < a.pmax * stride; i += 256) Pout[i] = 0.f;
    for (int i = kept + t; i < a.pmax; i += 256) a.visible_out[b * a.pmax + i] = 0;
    if (t == 0) a.count_out[b] = kept;
}

__global__ void __launch_bounds__(256) augment_people_kernel(AugPplArgs a) { augment_people_body<false>(a, nullptr); }

__global__ void __launch_bounds__(256) augment_people_mirror_kernel(AugPplArgs a, AugMirror m) {
    augment_people_body<true>(a, &m);
}

int check_image_args(const char* who, const void* src, const void* src_hw, const void* inv, int batch, int src_h, int src_w,
                     int out_h, int out_w, const void* dst_u8, const void* dst_f32) {
    if (!src || !src_hw || !inv) return ppn::fail(PPN_E_INVALID, "%s: NULL input", who);
    if (!dst_u8 && !dst_f32) return ppn::fail(PPN_E_INVALID, "%s: NULL output (give dst_u8, dst_f32 or both)", who);
    if (batch < 1 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || src_h > (1 << 20) || src_w > (1 << 20))
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry %d x %dx%d -> %dx%d", who, batch, src_h, src_w, out_h, out_w);
    return PPN_OK;
}

}  // namespace

extern "C" int ppn_augment_images(const uint8_t* src, const int32_t* src_hw, const float* inv, int32_t batch, int32_t src_h,
                                  int32_t src_w, int32_t out_h, int32_t out_w, uint8_t* dst_u8, float* dst_f32,
                                  void* stream) {
    if (!src || !src_hw || !inv) return ppn::fail(PPN_E_INVALID, "ppn_augment_images: NULL input");
    if (!dst_u8 && !dst_f32) return ppn::fail(PPN_E_INVALID, "ppn_augment_images: NULL output (give dst_u8, dst_f32 or both)");
    if (batch < 1 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || src_h > (1 << 20) || src_w > (1 << 20))
        return ppn::fail(PPN_E_INVALID, "ppn_augment_images: bad geometry %d x %dx%d -> %dx%d", batch, src_h, src_w, out_h,
                         out_w);
    const bool vec = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(dst_f32) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(dst_u8) % 4 == 0;
    const long long total = (long long)batch * out_h * (out_w / (vec ? 4 : 1));
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return ppn::fail(PPN_E_INVALID, "ppn_augment_images: output too large");
    AugImgArgs a{src, src_hw, inv, dst_u8, dst_f32, batch, src_h, src_w, out_h, out_w, nullptr};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) augment_image_kernel<4, false><<<(unsigned)blocks, 256, 0, st>>>(a);
    else augment_image_kernel<1, false><<<(unsigned)blocks, 256, 0, st>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_augment_images_color(const uint8_t* src, const int32_t* src_hw, const float* inv, const int32_t* color,
                                        int32_t batch, int32_t src_h, int32_t src_w, int32_t out_h, int32_t out_w,
                                        uint8_t* dst_u8, float* dst_f32, void* stream) {
    const char* who = "ppn_augment_images_color";
    if (!color) return ppn::fail(PPN_E_INVALID, "%s: NULL color", who);
    if (int rc = check_image_args(who, src, src_hw, inv, batch, src_h, src_w, out_h, out_w, dst_u8, dst_f32)) return rc;
    for (const void* in : {(const void*)src, (const void*)src_hw, (const void*)inv, (const void*)color})
        if (in == dst_u8 || in == dst_f32) return ppn::fail(PPN_E_INVALID, "%s: outputs must not alias the inputs", who);
    const bool vec = out_w % 4 == 0 && reinterpret_cast<uintptr_t>(dst_f32) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(dst_u8) % 4 == 0;
    const long long total = (long long)batch * out_h * (out_w / (vec ? 4 : 1));
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return ppn::fail(PPN_E_INVALID, "%s: output too large", who);
    AugImgArgs a{src, src_hw, inv, dst_u8, dst_f32, batch, src_h, src_w, out_h, out_w, color};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) augment_image_kernel<4, true><<<(unsigned)blocks, 256, 0, st>>>(a);
    else augment_image_kernel<1, true><<<(unsigned)blocks, 256, 0, st>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_augment_people(const float* people, const int32_t* visible, const int32_t* count, const float* fwd,
                                  int32_t batch, int32_t pmax, int32_t K, int32_t out_h, int32_t out_w, float* people_out,
                                  int32_t* visible_out, int32_t* count_out, void* stream) {
    if (!people || !visible || !count || !fwd || !people_out || !visible_out || !count_out)
        return ppn::fail(PPN_E_INVALID, "ppn_augment_people: NULL pointer");
    if (people == people_out || visible == visible_out || count == count_out)
        return ppn::fail(PPN_E_INVALID, "ppn_augment_people: outputs must not alias the inputs");
    if (batch < 1 || pmax < 1 || K < 1 || K > PPN_MAX_KP || out_h < 1 || out_w < 1)
        return ppn::fail(PPN_E_INVALID, "ppn_augment_people: bad geometry (batch %d, pmax %d, K %d, %dx%d)", batch, pmax, K,
                         out_h, out_w);
    AugPplArgs a{people, visible, count, fwd, people_out, visible_out, count_out, batch, pmax, K, out_h, out_w};
    augment_people_kernel<<<batch, 256, 0, static_cast<hipStream_t>(stream)>>>(a);
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}

extern "C" int ppn_augment_people_mirror(const float* people, const int32_t* visible, const int32_t* count, const float* fwd,
                                         const int32_t* mirror, const int32_t* kp_mirror, int32_t batch, int32_t pmax,
                                         int32_t K, int32_t out_h, int32_t out_w, float* people_out, int32_t* visible_out,
                                         int32_t* count_out, void* stream) {
    const char* who = "ppn_augment_people_mirror";
    if (!people || !visible || !count || !fwd || !kp_mirror || !people_out || !visible_out || !count_out)
        return ppn::fail(PPN_E_INVALID, "%s: NULL pointer", who);
    if (people == people_out || visible == visible_out || count == count_out || mirror == visible_out || mirror == count_out)
        return ppn::fail(PPN_E_INVALID, "%s: outputs must not alias the inputs", who);
    if (batch < 1 || pmax < 1 || K < 1 || K > PPN_MAX_KP || out_h < 1 || out_w < 1)
        return ppn::fail(PPN_E_INVALID, "%s: bad geometry (batch %d, pmax %d, K %d, %dx%d)", who, batch, pmax, K, out_h, out_w);
    if (kp_mirror[0] != 0) return ppn::fail(PPN_E_INVALID, "%s: kp_mirror[0] = %d, the instance mirrors to itself", who, kp_mirror[0]);
    for (int k = 0; k < K; ++k)
        if (kp_mirror[k] < 0 || kp_mirror[k] >= K || kp_mirror[kp_mirror[k]] != k)
            return ppn::fail(PPN_E_INVALID, "%s: kp_mirror is not an involution on 0..%d (entry %d)", who, K - 1, k);
    AugPplArgs a{people, visible, count, fwd, people_out, visible_out, count_out, batch, pmax, K, out_h, out_w};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!mirror) {
        augment_people_kernel<<<batch, 256, 0, st>>>(a);
    } else {
        AugMirror m{};
        m.flag = mirror;
        for (int j = 0; j + 1 < K; ++j) m.src[j] = kp_mirror[j + 1] - 1;      // >= 0: only keypoint 0 maps to 0
        augment_people_mirror_kernel<<<batch, 256, 0, st>>>(a, m);
    }
    PPN_LAUNCH_CHECK();
    return PPN_OK;
}
