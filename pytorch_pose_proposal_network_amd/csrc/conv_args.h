// Plain argument structs of the fused implicit-GEMM convolution kernels: what the route (conv_route.cpp) fills and the kernels
// (conv.hip, conv_big.hip, conv_splitk.hip) read.  Host-only, no HIP types.
#pragma once

namespace ppnconv {

// Division by a launch-invariant divisor (Granlund-Montgomery, round-up variant): exact for every 32-bit unsigned
// dividend, 4 VALU instructions instead of the ~35 of an emulated integer division.  The index arithmetic at the
// head of a workgroup sits on the critical path of its first loads.  (The device side, fast_div, is in conv_common.h.)
struct FastDiv {
    unsigned mul, sh1, sh2;
};
inline FastDiv make_fastdiv(unsigned d) {
    unsigned l = 0;
    while ((1ull << l) < d) ++l;                                     // ceil(log2 d)
    const unsigned long long m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
    return FastDiv{(unsigned)m, l < 1 ? l : 1u, l > 0 ? l - 1 : 0u};
}

struct ConvKArgs {
    const char* src;
    const char* wgt;
    const float* scale1;
    const float* shift1;
    const char* residual;
    char* out_raw;
    const float* scale2;
    const float* shift2;
    char* out_act;
    const char* zero;
    int B, H, W, Cin, Ho, Wo, Cout, ks, stride, dil, pad;
    int Ktot;      // padded GEMM depth (multiple of BK)
    int M;         // end of this launch's output-pixel range (B*Ho*Wo for a whole-tensor launch)
    int m_base;    // first output pixel of this launch (ppn_conv_desc.m_begin): tile p covers m_base + p*BP ...
    int HoWo;
    FastDiv div_howo, div_wo, div_nct;   // dividers by HoWo, Wo, n_ctiles
    int act1, act2, nchw;
    int log2Cin;
    int n_ctiles, n_ptiles;
    // fused head mode (ppn_conv_desc.argmax_keys): unary channels -> compact tensor, limb windows -> arg-max keys
    float* unary_out;                 // f32 [B][unary_ch][HoWo]
    unsigned long long* amax_keys;    // u64 [B][n_edges][HoWo], zeroed by the caller
    int unary_ch, window;             // 6K (108), sH*sW (441)
    // fused 1x1 projection shortcut (ppn_conv_desc.src2): extra K steps gathered from a second tensor
    const char* src2;                 // NHWC [B][H2][W2][Cin2]
    int H2, W2, Cin2, stride2;
    int nsteps_main;                  // K steps of the main convolution; the rest belong to the shortcut
    unsigned src2_bytes;
    int lo_off;                       // PPN_F16X3: bytes from a pixel's hi block to its lo' block in the SOURCE tensor
    int out_bf16;                     // PPN_F16 launch whose NHWC outputs are stored as bf16 (PPN_CONV_OUT_BF16)
    int out_plain;                    // PPN_F16X3 launch whose NHWC outputs are stored as plain half (PPN_CONV_X3_PLAIN_OUT)
    const char* pf_ptr;               // ppn_conv_desc.prefetch: the next launch's weights, touched line by line (large-tile kernel)
    unsigned pf_lines, pf_per_wg;     // 128-byte lines in all / per workgroup (at most 2 per thread; set at the launch: it knows NW)
    // ppn_conv_desc.stats_*: BatchNorm partial sums from the epilogue (large-tile kernel, ST instantiations)
    double* st_partial;
    int st_mode, st_act;
    const char* st_x;
    const float *st_gamma, *st_beta, *st_mean, *st_rstd;
    // strip loader of the large-tile kernel (SP instantiations): image rows per 192-pixel tile (0 = off), strip pitch in pixels
    // and the divider by it
    int sp_rows, sp_pitch;
    FastDiv sp_div;
};

// conv_big.hip: 512-thread, (BP x BC) = ({128,144,192,256} x {64,128,256}) tiles for Cin % K-step == 0 layers
struct BigTile {
    int bp, bc;
};
// the large tiles whose single-output 16-bit epilogue exists (the whole tile as 16-bit rows in the staging LDS) AND that carry the
// BatchNorm-statistics instantiation: kFastFits of the kernel, restated for the host
constexpr bool stats_tile_ok(int bp, int bc) {
    return bc >= 128 && (unsigned long long)bp * (unsigned long long)(bc * 2 + 16) <= 2ull * (unsigned long long)(bp + bc) * 128;
}
// edge-aligned limb tile of the head conv (ppn_conv_desc.limb_edge_pad): 128 pixels x one edge's window padded to 448 rows
constexpr int kEdgeTileBP = 128, kEdgeTileBC = 448;

}  // namespace ppnconv
