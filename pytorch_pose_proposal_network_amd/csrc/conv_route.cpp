// The dispatch of ppn_conv2d_fused / a plan's conv entries: one pure routing pass in front of the launchers (conv_route.h).
// Everything that decides WHERE a descriptor runs is here -- validation, kernel, tile, two-segment split, strip loader, BatchNorm
// statistics, the kernel arguments, the tuning knobs and their entry points; the kernels' files hold what needs the device.
#include "conv_route.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>

namespace ppnconv {

using ppnsplitk::kTileC;
using ppnsplitk::kTileP;

static bool tile_shape_ok(int bp, int bc) {
    if (bp == 144) return bc == 256;                     // the 8 x 1 wave grid exists for the 256-channel tile only
    return (bp == 128 || bp == 192 || bp == 256) && (bc == 64 || bc == 128 || bc == 256) && !(bc == 64 && bp == 192);
}

RouteKnobs& knobs() {
    static RouteKnobs k = [] {
        RouteKnobs e{};
        auto off = [](const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; };
        e.tile_policy = getenv("PPN_CONV_CONT") ? 1 : 0;
        int bp = 0, bc = 0;
        const char* ov = getenv("PPN_CONV_TILE");
        if (ov && sscanf(ov, "%d,%d", &bp, &bc) == 2 && tile_shape_ok(bp, bc)) { e.ov_bp = bp; e.ov_bc = bc; }
        e.conv64_on = off("PPN_CONV64") ? 0 : 1;
        e.strip_on = off("PPN_CONV_STRIP") ? 0 : 1;
        e.waves = getenv("PPN_CONV_WAVES") ? atoi(getenv("PPN_CONV_WAVES")) : 8;                  // tuning knob
        e.policy1_mask = getenv("PPN_POLICY1_MASK") ? atoi(getenv("PPN_POLICY1_MASK")) : 7;       // experiment knob, see big_tile_for
        // relative efficiency of the 144 x 256 tile in the cost model below (PPN_EFF144 overrides: 0 takes the tile out).
        // Measured (round 4, same box, in sequence): the five 24 x 24 512 -> 512 layers 106.5 -> 94.9 us (= 0.93 on this scale), but
        // layer5's 256 -> 256 launches 101.5 -> 118 / 87.8 -> 96.1 us against 192 x 128 at three rounds (= 0.82-0.87): 0.90 picks it
        // for the former only.  It shortens a LONE launch by filling all 256 CUs with smaller, less efficient workgroups (CU-time
        // per launch +19 %): with three lanes in flight the same switch cost 3.5 % of the images/s (10.69 k vs 11.07 k, two
        // interleaved pairs of runs), so plans that share the GPU (PPN_CONV_SHARED_GPU) never take it.
        e.eff144 = getenv("PPN_EFF144") ? atof(getenv("PPN_EFF144")) : 0.90;
        return e;
    }();
    return k;
}

namespace {

bool dtype_ok(int dtype) { return dtype == PPN_F32 || dtype == PPN_BF16 || dtype == PPN_F16 || dtype == PPN_F16X3; }

// The LARGEST channel tile the large-tile kernel may pick for a Cout (it chooses per problem size): packed weights are padded to
// it (ppn_conv_tiling), so any smaller power-of-two tile fits too.
int pad_tile_for(int cout) { return cout >= 256 ? 256 : (cout >= 128 ? 128 : 64); }

// tile of the generic kernel (conv.hip)
BigTile choose_tile(int cout) {
    if (cout <= 16) return {256, 16};
    if (cout <= 32) return {256, 32};
    if (cout <= 64) return {128, 64};
    return {128, 128};
}

int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

// Pick the large tile: channels 256 / 128 / 64 by Cout, pixel height so that the fewest CU-rounds are wasted
// (256 CUs; one workgroup per CU, two for the 64-channel tile whose LDS footprint is 80 KB).
// ksteps: K steps of the launch (0 = unknown); shared_gpu: the launch shares the GPU with other streams' launches
// (ppn_conv_desc.flags & PPN_CONV_SHARED_GPU): tiles that only shorten a LONE launch are left out
bool big_tile_for(const RouteKnobs& k, int cout, long long m, BigTile* out, int ksteps = 0, bool shared_gpu = false) {
    if (cout < 64) return false;
    // a forced tile applies to every layer whose padded Cout it divides
    if (k.ov_bp > 0 && k.ov_bc <= ((cout + 63) / 64) * 64 && k.ov_bc <= pad_tile_for(cout)) {
        out->bp = k.ov_bp; out->bc = k.ov_bc;
        return true;
    }
    if (cout >= 4096) {
        // the head conv (512 -> 7605, K = 512) writes 17.5 MB/image and is store-bound: a 192x128 tile keeps
        // two workgroups per CU so one's epilogue stores overlap the other's main loop (measured 322 vs 399 us)
        out->bp = 192; out->bc = 128;
        return true;
    }
    // time ~ ceil(tiles / 256 CUs) * tile area / eff(tile); eff = relative throughput of a tile shape measured on
    // the 48x48x512 3x3 layers at batch 32 (tools/bench_conv.py with PPN_CONV_TILE), i.e. how well its FLOPs per
    // staged byte feed the MFMA pipe.  For Cout = 256 the 128-channel tile wins through quantisation
    // (768 workgroups = 3 full rounds instead of 384 = 1.5).
    struct Cand { int bp, bc; double eff; };
    // 144 x 256 (round 4; 8 waves side by side along the channels, each 32 channels x all 144 pixels): 18 432 pixels x 512
    // channels (the five 24 x 24 layers of DRN-D-22 at batch 32) = exactly 256 workgroups = one full round, where 192 x 256
    // leaves 64 of the 256 CUs idle; and 73 728 x 256 (layer5) = 512 = two rounds.  Same K order: results unchanged.
    // (round 4, measured and removed: a 288 x 256 tile -- 4 x 2 wave grid, 36 MFMA tiles per wave, 256 VGPRs with 6 spilled --
    // makes layer5's 73 728 x 256 launches ONE round of 256 workgroups: 93.9 -> 77.8 us alone, but -1.7 % images/s with three
    // lanes (a 136 KB workgroup holds its CU alone for 78 us; two 80 KB workgroups of 192 x 128 share one), nothing on a
    // single lane or the training step, and on the 512-channel layers its two rounds take what 192 x 256's three do.)
    const Cand cands[] = {{256, 256, 1.27}, {192, 256, 1.10}, {144, 256, k.eff144}, {128, 256, 0.92}, {256, 128, 0.90},
                          {192, 128, 0.95}, {128, 128, 0.87}, {256, 64, 0.60},      {128, 64, 0.55}};
    int bc_max = pad_tile_for(cout);
    const int bc_min = cout >= 256 ? 128 : bc_max;
    // 1x1 projections (<= 8 K steps) are prologue/epilogue-bound: the 128-channel tile's shorter epilogue wins over the
    // 256-channel tile's staging efficiency (tools/ab_tiles.py: 256->512 at 48x48 32.5 vs 38.4 us, 512->512 stride 2
    // 15.9 vs 17.1, 128->512 at 24x24 10.7 vs 11.6)
    if (ksteps > 0 && ksteps <= 8 && bc_max == 256) bc_max = 128;
    double best = 1e30;
    for (const Cand& cd : cands) {
        if (cd.bc > bc_max || cd.bc < bc_min || cd.eff <= 0.0 || (shared_gpu && cd.bp == 144)) continue;
        const long long tiles = ((m + cd.bp - 1) / cd.bp) * ((cout + cd.bc - 1) / cd.bc);
        // policy 1 (several launches in flight on different streams, ppn_set_conv_tile_policy): another stream's
        // workgroups fill a partial last round, so only the tile's efficiency counts
        // (round 4, measured and dropped: under PPN_CONV_SHARED_GPU, launches with fewer tiles than CUs -- the 24 x 24 layers --
        // priced by efficiency alone, i.e. 256 x 256 tiles on 144 of the CUs: 10.79 / 10.79 k images/s against 10.83 / 10.84 k
        // with the whole-round rule, interleaved runs on one box, and 3.25 vs 3.16 ms for the conv stack in sequence)
        // PPN_POLICY1_MASK (experiment knob, with policy 1): bit 0 = 512-wide layers at >= 65 536 pixels, bit 1 = 512-wide below that,
        // bit 2 = the narrower layers: which classes are priced by fractional rounds
        const int cls = cout >= 512 ? (m >= 65536 ? 1 : 2) : 4;
        const bool frac = k.tile_policy == 1 && (k.policy1_mask & cls);
        const double rounds = frac ? (double)tiles / 256.0 : (double)((tiles + 255) / 256);
        const double cost = rounds * cd.bp * cd.bc / cd.eff;
        if (cost < best) { best = cost; out->bp = cd.bp; out->bc = cd.bc; }
    }
    return true;
}

// Two-segment launch (tile policy 2, opt-in): the most efficient tile (256x256: 1.27 vs 1.10 for 192x256) wastes most
// of a round when its workgroup count is not a multiple of the 256 CUs (73 728 pixels x 512 channels = 576 tiles =
// 2.25 rounds), which is why the single-tile choice settles for 192x256 there (768 = 3 rounds).  Cutting the pixel
// range instead -- whole rounds of the big tile, then ONE round of a small tile over the remaining pixels -- should cost
// 2 x 51.6 k + 18.8 k = 122 k units instead of 134 k.  MEASURED (round 2, tools/ab_split.sh): the 256x256 segments do
// run at 1.28-1.46 PFLOP/s (0.51-0.58 of peak) instead of 1.14-1.28, but the lone 128x128 round takes 55-58 us instead of
// the ~35 the model assumes (one small workgroup per CU stages 2x the bytes per FLOP of the big tile through the same
// L2->LDS path; a four-stage pipeline changed nothing), so the layer is not faster (277 us either way) and the extra
// launches cost 1.8 % (three lanes) to 3.6 % (one lane) of throughput.  Not the default; kept for the pixel-range
// interface it exercises.  Returns the cut (0: single launch): pixels [0, cut) run whole rounds of the most efficient tile, the
// rest a smaller tile that fills one more round.  Only for Cout >= 256, where efficiencies were measured.
long long big_split_for(const RouteKnobs& k, int cout, long long m) {
    BigTile single;
    if (k.tile_policy != 2 || cout < 256 || cout >= 4096 || !big_tile_for(k, cout, m, &single) || k.ov_bp > 0) return 0;
    struct Cand { int bp, bc; double eff; };
    static const Cand cands[] = {{256, 256, 1.27}, {192, 256, 1.10}, {128, 256, 0.92}, {256, 128, 0.90},
                                 {192, 128, 0.95}, {128, 128, 0.87}};
    auto rounds_cost = [&](const Cand& cd, long long mm) {
        const long long tiles = ((mm + cd.bp - 1) / cd.bp) * ((cout + cd.bc - 1) / cd.bc);
        return (double)((tiles + 255) / 256) * cd.bp * cd.bc / cd.eff;
    };
    double best_single = 1e30;
    for (const Cand& cd : cands) best_single = std::min(best_single, rounds_cost(cd, m));
    double best = best_single * 0.96;                    // the second launch must pay for its own start-up
    long long cut = 0;
    for (const Cand& p : cands) {
        const long long ct = (cout + p.bc - 1) / p.bc;
        if (256 % ct != 0) continue;
        const long long rounds = (m / p.bp) * ct / 256;  // whole rounds of whole tiles
        if (rounds < 1) continue;
        const long long m1 = rounds * 256 / ct * p.bp;
        if (m1 >= m) continue;
        double tail = 1e30;
        for (const Cand& q : cands) tail = std::min(tail, rounds_cost(q, m - m1));
        const double cost = (double)rounds * p.bp * p.bc / p.eff + tail;
        if (cost < best) { best = cost; cut = m1; }
    }
    return cut;
}

// Does a launch of this tile carry the BatchNorm-statistics epilogue (ppn_conv_desc.stats_mode)?  conv_route adds the per-launch
// conditions of the single-output 16-bit epilogue.
bool big_stats_ok(const RouteKnobs& k, int dtype, BigTile t) {
    return dtype == PPN_BF16 && k.waves == 8 && stats_tile_ok(t.bp, t.bc);
}

// Does this launch take the strip loader (kernel flag SP)?  3x3, stride 1, "same" padding on the 192 x 256 tile of a 16-bit mode,
// plain NHWC epilogues, and every tile R = 192 / Wo whole rows of one image; the strip of R rows at pitch P = Wo + margins
// (P = Wo (mod 8), room for 2 * dil columns of padding) must fit the 256-row buffer.
bool strip_eligible(const RouteKnobs& k, const ConvKArgs& a, int dtype, BigTile t, int* rows, int* pitch) {
    if (!k.strip_on || k.waves != 8 || t.bp != 192 || t.bc != 256 || (dtype != PPN_BF16 && dtype != PPN_F16)) return false;
    if (a.ks != 3 || a.stride != 1 || a.dil < 1 || a.pad != a.dil || a.Ho != a.H || a.Wo != a.W || a.Ktot != 9 * a.Cin) return false;
    if (a.src2 || a.st_mode != 0 || a.nchw || a.amax_keys || a.unary_out) return false;
    if (192 % a.Wo != 0 || a.HoWo % 192 != 0 || a.m_base % 192 != 0 || (a.M - a.m_base) % 192 != 0) return false;
    const int r = 192 / a.Wo, p = a.Wo + 8 * ((2 * a.dil + 7) / 8);
    if (r * p > 256) return false;
    *rows = r; *pitch = p;
    return true;
}

// 64 -> 64 3x3 stride 1 in the 16-bit modes: the scope of the register-resident filter bank kernel (conv64.hip)
bool conv64_supported(const RouteKnobs& k, const ppn_conv_desc* d) {
    if (!k.conv64_on || (d->flags & PPN_CONV_NO_FILTER_BANK)) return false;
    return (d->dtype == PPN_BF16 || d->dtype == PPN_F16) && d->cin == 64 && d->cout == 64 && d->ksize == 3 && d->stride == 1 &&
           d->dilation == 1 && d->pad == 1 && !d->src2 && !d->out_nchw_f32 && !d->argmax_keys && d->k_total == 576 &&
           d->cout_pad == 64 && d->m_count == 0 && d->act1 != PPN_ACT_SIGMOID && d->act2 != PPN_ACT_SIGMOID;
}

// stem3x3.hip: 3x3, pad 1, Cin 16, Cout in {16,32}, stride in {1,2}; weight in the reference layout (f32, device).
bool stem3x3_supported(int cin, int cout, int ksize, int stride, int dilation, int pad) {
    return cin == 16 && (cout == 16 || cout == 32) && ksize == 3 && (stride == 1 || stride == 2) && dilation == 1 && pad == 1;
}

// THE fill of the kernel arguments from a descriptor: pixels [m_lo, m_hi) in bp x bc tiles; stats: the launch delivers the
// BatchNorm statistics the descriptor asks for.  The strip loader and the prefetch share per workgroup, which follow from these
// arguments, are added by the caller where the segment has them.
void fill_args(const ppn_conv_desc* d, long long m_lo, long long m_hi, int bp, int bc, int nsteps_main, bool stats, ConvKArgs* out) {
    const bool x3 = d->dtype == PPN_F16X3;
    const int log2c = ilog2_exact(d->cin);
    ConvKArgs a{};
    a.src = static_cast<const char*>(d->src);
    a.wgt = static_cast<const char*>(d->weight);
    a.scale1 = d->scale1; a.shift1 = d->shift1;
    a.residual = static_cast<const char*>(d->residual);
    a.out_raw = static_cast<char*>(d->out_raw);
    a.scale2 = d->scale2; a.shift2 = d->shift2;
    a.out_act = static_cast<char*>(d->out_act);
    a.zero = static_cast<const char*>(d->zero_page);
    a.B = d->batch; a.H = d->in_h; a.W = d->in_w; a.Cin = x3 ? 2 * d->cin : d->cin; a.Ho = d->out_h; a.Wo = d->out_w; a.Cout = d->cout;
    a.ks = d->ksize; a.stride = d->stride; a.dil = d->dilation; a.pad = d->pad;
    a.Ktot = d->k_total; a.M = (int)m_hi; a.m_base = (int)m_lo; a.HoWo = d->out_h * d->out_w;
    a.div_howo = make_fastdiv((unsigned)a.HoWo); a.div_wo = make_fastdiv((unsigned)d->out_w);
    a.act1 = d->act1; a.act2 = d->act2; a.nchw = d->out_nchw_f32;
    a.log2Cin = log2c < 0 ? 0 : log2c;
    a.n_ctiles = d->cout_pad / bc;
    a.div_nct = make_fastdiv((unsigned)a.n_ctiles);
    a.n_ptiles = (int)((m_hi - m_lo + bp - 1) / bp);
    a.src2 = static_cast<const char*>(d->src2);
    a.H2 = d->src2 ? d->in2_h : 1; a.W2 = d->src2 ? d->in2_w : 1; a.Cin2 = d->src2 ? d->cin2 : 0;
    a.stride2 = d->src2 ? d->stride2 : 1;
    a.nsteps_main = nsteps_main;
    a.src2_bytes = d->src2 ? (unsigned)((size_t)d->batch * d->in2_h * d->in2_w * d->cin2 * (d->dtype == PPN_F32 ? 4 : 2)) : 0u;
    a.unary_out = d->unary_out;
    a.amax_keys = reinterpret_cast<unsigned long long*>(d->argmax_keys);
    a.unary_ch = d->unary_channels;
    a.window = d->limb_window;
    a.lo_off = x3 ? d->cin * 2 : 0;                                   // source pixel = [hi(cin) | lo'(cin)] halves
    a.out_plain = (d->flags & PPN_CONV_X3_PLAIN_OUT) ? 1 : 0;
    a.pf_ptr = static_cast<const char*>(d->prefetch);
    a.pf_lines = (d->prefetch && d->prefetch_bytes > 0) ? (unsigned)std::min<long long>(d->prefetch_bytes / 128, 1 << 24) : 0u;
    a.out_bf16 = (d->flags & PPN_CONV_OUT_BF16) ? 1 : 0;
    if (stats) {
        a.st_partial = static_cast<double*>(d->stats_partial);
        a.st_mode = d->stats_mode; a.st_act = d->stats_act;
        a.st_x = static_cast<const char*>(d->stats_x);
        a.st_gamma = d->stats_gamma; a.st_beta = d->stats_beta; a.st_mean = d->stats_mean; a.st_rstd = d->stats_rstd;
    }
    a.sp_div = make_fastdiv(1);
    *out = a;
}

// Scope of the split-K path (conv_splitk.hip) and the partition of a descriptor.  Pointers are not looked at.
int splitk_check(const ppn_conv_desc* d, ppnsplitk::Partition* part) {
    if (!d) return ppn::fail(PPN_E_INVALID, "conv desc is NULL");
    if (!dtype_ok(d->dtype)) return ppn::fail(PPN_E_INVALID, "bad dtype %d", d->dtype);
    if (d->dtype == PPN_F16X3) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: no PPN_F16X3 form");
    if (d->src2) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: no fused projection shortcut (src2)");
    if (d->out_nchw_f32 || d->argmax_keys || d->unary_out || d->limb_edge_pad)
        return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: NHWC outputs only (no NCHW head, arg-max or edge-tile mode)");
    if (d->stats_mode != 0) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: no BatchNorm statistics (stats_mode)");
    if (d->flags & PPN_CONV_X3_PLAIN_OUT) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: no PPN_CONV_X3_PLAIN_OUT");
    if ((d->flags & PPN_CONV_OUT_BF16) && d->dtype != PPN_F16)
        return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_OUT_BF16: a PPN_F16 launch");
    if (d->batch < 1 || d->in_h < 1 || d->in_w < 1 || d->cin < 1 || d->cout < 1 || d->stride < 1 || d->dilation < 1 || d->pad < 0)
        return ppn::fail(PPN_E_INVALID, "bad conv geometry");
    if (d->ksize != 1 && d->ksize != 3) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: ksize 1 or 3 (got %d)", d->ksize);
    const int bk = d->dtype == PPN_F32 ? 32 : 64;
    if (d->cin % bk != 0) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: cin %d must be a multiple of the K step %d", d->cin, bk);
    if (d->m_count != 0) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: whole-tensor launches only (m_count = 0)");
    if (d->act1 < PPN_ACT_NONE || d->act1 > PPN_ACT_LRELU || d->act2 < PPN_ACT_NONE || d->act2 > PPN_ACT_LRELU)
        return ppn::fail(PPN_E_UNSUPPORTED, "sigmoid is only implemented for the NCHW head output");
    if (d->cout % 8 != 0) return ppn::fail(PPN_E_UNSUPPORTED, "NHWC output needs cout %% 8 == 0 (got %d)", d->cout);
    if (d->cout_pad < d->cout || d->cout_pad % kTileC != 0)
        return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: cout_pad %d must be a multiple of %d and >= cout", d->cout_pad, kTileC);
    const int eff = d->dilation * (d->ksize - 1) + 1;
    const int oh = (d->in_h + 2 * d->pad - eff) / d->stride + 1, ow = (d->in_w + 2 * d->pad - eff) / d->stride + 1;
    if (oh != d->out_h || ow != d->out_w || oh < 1 || ow < 1)
        return ppn::fail(PPN_E_INVALID, "out size %dx%d inconsistent with %dx%d", d->out_h, d->out_w, oh, ow);
    const long long kreal = (long long)d->ksize * d->ksize * d->cin;
    if (d->k_total != kreal) return ppn::fail(PPN_E_INVALID, "k_total %d != %lld", d->k_total, kreal);
    const long long m = (long long)d->batch * d->out_h * d->out_w;
    const long long in_elems = (long long)d->batch * d->in_h * d->in_w * d->cin;
    if (m > 0x7fffffffLL || in_elems > 0x7fffffffLL || m * d->cout > 0x7fffffffLL * 8)
        return ppn::fail(PPN_E_UNSUPPORTED, "tensor too large for 32-bit indexing");
    if (!ppnsplitk::partition(d->dtype == PPN_F32, d->k_total, m, d->cout_pad, part))
        return ppn::fail(PPN_E_INVALID, "PPN_CONV_SPLIT_K: the GEMM depth cannot be partitioned");
    return PPN_OK;
}

// opt-in split-K pair of launches: its own scope checks, never a fallback to the other kernels
int route_splitk(const ppn_conv_desc* d, ConvSegment* s) {
    ppnsplitk::Partition& p = s->splitk;
    if (const int rc = splitk_check(d, &p)) return rc;
    if (!d->src || !d->weight || !d->zero_page) return ppn::fail(PPN_E_INVALID, "NULL src/weight/zero_page");
    if (!d->out_raw && !d->out_act) return ppn::fail(PPN_E_INVALID, "conv has no output");
    if (!d->splitk_ws || d->splitk_ws_bytes < p.ws_bytes)
        return ppn::fail(PPN_E_INVALID, "PPN_CONV_SPLIT_K: splitk_ws is NULL or holds %lld of the %lld bytes "
                                        "ppn_conv_splitk_workspace asks for", (long long)d->splitk_ws_bytes, p.ws_bytes);
    if ((reinterpret_cast<size_t>(d->splitk_ws) & 15) != 0)
        return ppn::fail(PPN_E_INVALID, "PPN_CONV_SPLIT_K: splitk_ws must be 16-byte aligned");
    s->kernel = Kernel::SplitK;
    s->m_hi = p.m;
    s->bp = kTileP; s->bc = kTileC;
    // (the fields fill_args sets beyond the geometry, operands and epilogue -- log2Cin, the src2, head, prefetch and strip
    // fields -- are not read by the split-K kernels)
    fill_args(d, 0, p.m, kTileP, kTileC, p.nsteps, false, &s->args);
    if ((long long)s->args.n_ctiles * s->args.n_ptiles > 0x7fffffffLL || p.slabs > 65535)
        return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_SPLIT_K: grid too large");
    return PPN_OK;
}

// One launch: the whole tensor, or the pixel range m_begin / m_count names.  *cut > 0: not routed, the caller routes the two ranges
// [0, cut) and [cut, all) instead (tile policy 2).
int route_segment(const ppn_conv_desc* d, const RouteKnobs& k, ConvSegment* s, long long* cut) {
    *cut = 0;
    const bool x3 = d->dtype == PPN_F16X3;
    const int bk = d->dtype == PPN_F32 ? 32 : 64, epc = d->dtype == PPN_F32 ? 4 : 8;
    if (d->batch < 1 || d->in_h < 1 || d->in_w < 1 || d->cin < 1 || d->cout < 1 || d->stride < 1 || d->dilation < 1 || d->pad < 0)
        return ppn::fail(PPN_E_INVALID, "bad conv geometry");
    if (d->ksize < 1 || d->ksize > 5) return ppn::fail(PPN_E_UNSUPPORTED, "ksize %d not supported by the generic kernel", d->ksize);
    if (d->cin % epc != 0) return ppn::fail(PPN_E_UNSUPPORTED, "cin %d must be a multiple of %d", d->cin, epc);
    const int eff = d->dilation * (d->ksize - 1) + 1;
    const int oh = (d->in_h + 2 * d->pad - eff) / d->stride + 1, ow = (d->in_w + 2 * d->pad - eff) / d->stride + 1;
    if (oh != d->out_h || ow != d->out_w)
        return ppn::fail(PPN_E_INVALID, "out size %dx%d inconsistent with %dx%d", d->out_h, d->out_w, oh, ow);
    s->dtype = d->dtype;
    s->m_lo = 0; s->m_hi = (long long)d->batch * d->out_h * d->out_w;
    if (stem3x3_supported(d->cin, d->cout, d->ksize, d->stride, d->dilation, d->pad) && d->k_total == 144 &&
        d->cout_pad == d->cout && !d->residual && !d->out_nchw_f32 &&
        ((d->act1 == PPN_ACT_RELU && d->scale1 && d->shift1) ||
         (d->act1 == PPN_ACT_NONE && !d->scale1 && !d->shift1 && !d->out_act)) &&
        (!d->out_act || d->act2 == PPN_ACT_RELU)) {
        // stem3x3.hip is instantiated for float and __bf16: an IEEE-half tensor would be read as bf16 bits
        if (d->dtype != PPN_F32 && d->dtype != PPN_BF16)
            return ppn::fail(PPN_E_UNSUPPORTED, "stem3x3 (16 -> 16 / 32 channels, 3x3, pad 1) runs as PPN_F32 or PPN_BF16 only");
        if (!d->src || !d->weight) return ppn::fail(PPN_E_INVALID, "NULL src/weight");
        if ((d->scale1 == nullptr) != (d->shift1 == nullptr) || (!d->out_raw && !d->out_act))
            return ppn::fail(PPN_E_INVALID, "stem3x3: bad arguments");
        s->kernel = Kernel::Stem3x3;
        s->bc = d->cout; s->bp = d->stride;
        return PPN_OK;
    }
    const bool smallc = (d->cin % bk) != 0;
    if (smallc && ilog2_exact(d->cin) < 0) return ppn::fail(PPN_E_UNSUPPORTED, "cin %d < K step must be a power of two", d->cin);
    const int kreal = d->ksize * d->ksize * d->cin;
    int kpad = ((kreal + bk - 1) / bk) * bk;
    if (x3) {
        if (smallc || d->cout < 64 || d->src2 || d->limb_edge_pad)
            return ppn::fail(PPN_E_UNSUPPORTED, "PPN_F16X3: cin %% 64 == 0, cout >= 64, no fused shortcut, no edge tile");
        kpad *= 3;                                                    // three virtual slabs per real one
    }
    const int kmain = kpad;
    if (d->src2) {
        if (d->cin2 < bk || d->cin2 % bk != 0 || d->stride2 < 1 || d->in2_h < 1 || d->in2_w < 1 || d->scale1 ||
            d->out_nchw_f32 || smallc || (d->out_h - 1) * d->stride2 >= d->in2_h || (d->out_w - 1) * d->stride2 >= d->in2_w)
            return ppn::fail(PPN_E_INVALID, "fused shortcut: cin2 must be a multiple of the K step, scale1 NULL, "
                                            "and (out-1)*stride2 inside the second source");
        kpad += d->cin2;
    }
    if (d->k_total != kpad) return ppn::fail(PPN_E_INVALID, "k_total %d != %d", d->k_total, kpad);
    const long long m_all = s->m_hi;
    if (m_all > 0x7fffffffLL) return ppn::fail(PPN_E_UNSUPPORTED, "tensor too large for 32-bit indexing");
    long long m_lo = 0, m_hi = m_all;
    if (d->m_count != 0) {
        if (d->m_begin < 0 || d->m_count < 0 || (long long)d->m_begin + d->m_count > m_all)
            return ppn::fail(PPN_E_INVALID, "pixel range [%d, +%d) outside the %lld output pixels", d->m_begin, d->m_count, m_all);
        m_lo = d->m_begin; m_hi = m_lo + d->m_count;
        // The NCHW f32 epilogues store four consecutive pixels of one channel plane as a float4 when HoWo % 4 == 0:
        // a cut that is not a multiple of 4 would store misaligned, write up to 3 pixels of the neighbouring range
        // (a race with the launch that owns it) or run into the next channel plane.
        if (d->out_nchw_f32 && ((d->out_h * d->out_w) & 3) == 0 && ((m_lo & 3) != 0 || ((m_hi & 3) != 0 && m_hi != m_all)))
            return ppn::fail(PPN_E_INVALID, "NCHW output: pixel range [%d, +%d) must begin on a multiple of 4 and end on one "
                                            "(or at the last pixel)", d->m_begin, d->m_count);
    } else if (!smallc && d->stats_mode == 0) {
        // whole tensor: two launches with different tiles where that saves a round of workgroups (ppn_conv_split)
        const long long c = big_split_for(k, d->cout, m_all);
        if (c > 0 && c < m_all) { *cut = c; return PPN_OK; }
    }
    s->m_lo = m_lo; s->m_hi = m_hi;
    // the register-resident filter bank kernel, same results
    if (conv64_supported(k, d) && d->in_h == d->out_h && d->in_w == d->out_w && !(d->flags & PPN_CONV_OUT_BF16)) {
        if (!d->src || !d->weight || (!d->out_raw && !d->out_act)) return ppn::fail(PPN_E_INVALID, "conv64: NULL src/weight/output");
        if ((size_t)d->batch * d->in_h * d->in_w * 64 * 2 >= 0x7fffff00ull)
            return ppn::fail(PPN_E_UNSUPPORTED, "tensor too large for the buffer-addressed conv kernel");
        s->kernel = Kernel::Conv64;
        return PPN_OK;
    }
    const long long m = m_hi - m_lo;                                  // pixels of THIS launch: the tile is chosen for them
    const BigTile tc = choose_tile(d->cout);
    BigTile bt{0, 0};
    const bool big = !smallc && big_tile_for(k, d->cout, m, &bt, kpad / bk, (d->flags & PPN_CONV_SHARED_GPU) != 0);
    if (d->limb_edge_pad != 0) {
        // edge-aligned limb tile (conv_head.hip): rows [e * limb_edge_pad, +limb_window) of the packed weight / shift1
        // hold edge e's window, the rest of each edge's rows are padding
        if (d->limb_edge_pad != kEdgeTileBC || smallc || d->src2 || !d->argmax_keys || !d->out_nchw_f32 || d->out_raw ||
            d->unary_out || d->unary_channels != 0 || d->residual || d->out_act || d->limb_window < 1 ||
            d->limb_window > d->limb_edge_pad || d->cout % d->limb_window != 0 ||
            d->cout_pad != d->cout / d->limb_window * d->limb_edge_pad || d->act1 != PPN_ACT_SIGMOID)
            return ppn::fail(PPN_E_INVALID, "limb_edge_pad: needs %d rows per edge (window <= that), cout = E * window, "
                                            "cout_pad = E * limb_edge_pad, sigmoid, argmax_keys only (no out_raw / unary_out)",
                             kEdgeTileBC);
        // the kernel's epilogue masks the rows past the window in the LAST 16-row channel tile of its last wave only: a pad row
        // below that tile would compete (with zero weights and bias it wins every window whose scores are all below 0.5)
        if (d->limb_window <= d->limb_edge_pad - 16)
            return ppn::fail(PPN_E_UNSUPPORTED, "limb_edge_pad: limb_window %d is outside %d..%d (the edge tile masks pad rows in its "
                                                "last 16 rows only; smaller windows take the atomic-key epilogue, limb_edge_pad = 0)",
                             d->limb_window, d->limb_edge_pad - 15, d->limb_edge_pad);
        if (!d->src || !d->weight) return ppn::fail(PPN_E_INVALID, "NULL src/weight");
        if (d->ksize != 1 || d->stride != 1 || d->pad != 0 || d->scale1)
            return ppn::fail(PPN_E_UNSUPPORTED, "limb_edge_pad: the head conv is 1x1, stride 1, no padding, bias only (scale1 NULL)");
        if (d->k_total % (2 * bk) != 0)
            return ppn::fail(PPN_E_UNSUPPORTED, "limb_edge_pad: k_total must be a multiple of %d (an even number of K steps)", 2 * bk);
        const size_t es = d->dtype == PPN_F32 ? 4 : 2;
        if ((size_t)m_all * d->cin * es >= 0x7fffff00ull || (size_t)d->cout_pad * d->k_total * es >= 0x7fffff00ull)
            return ppn::fail(PPN_E_UNSUPPORTED, "tensor too large for the buffer-addressed head kernel");
        s->kernel = Kernel::HeadLimb;
        s->bp = kEdgeTileBP; s->bc = kEdgeTileBC;
        return PPN_OK;
    }
    const int bc = big ? bt.bc : tc.bc, bp = big ? bt.bp : tc.bp;
    if (d->cout_pad % bc != 0 || d->cout_pad < d->cout)
        return ppn::fail(PPN_E_INVALID, "cout_pad %d must be a multiple of %d and >= cout", d->cout_pad, bc);
    if (!d->src || !d->weight || !d->zero_page) return ppn::fail(PPN_E_INVALID, "NULL src/weight/zero_page");
    if (!d->out_raw && !d->out_act && !d->argmax_keys) return ppn::fail(PPN_E_INVALID, "conv has no output");
    if (d->argmax_keys && !d->limb_edge_pad &&
        (!d->out_nchw_f32 || !d->unary_out || d->unary_channels < 0 || d->limb_window < 1 ||
         d->unary_channels > d->cout || (d->cout - d->unary_channels) % d->limb_window != 0))
        return ppn::fail(PPN_E_INVALID, "fused arg-max needs the NCHW head mode, unary_out and cout = unary + E*window");
    if (d->argmax_keys && d->act1 != PPN_ACT_SIGMOID)
        return ppn::fail(PPN_E_INVALID, "fused arg-max keys assume non-negative (sigmoid) outputs");
    if (!d->out_nchw_f32 && (d->act1 == PPN_ACT_SIGMOID || d->act2 == PPN_ACT_SIGMOID))
        return ppn::fail(PPN_E_UNSUPPORTED, "sigmoid is only implemented for the NCHW head output");
    if (d->out_nchw_f32) {
        if (d->residual || d->out_act || (!d->out_raw && !d->argmax_keys))
            return ppn::fail(PPN_E_UNSUPPORTED, "NCHW head output supports out_raw / fused arg-max only");
    } else if (d->cout % 8 != 0) {
        return ppn::fail(PPN_E_UNSUPPORTED, "NHWC output needs cout %% 8 == 0 (got %d)", d->cout);
    }
    const long long in_elems = (long long)d->batch * d->in_h * d->in_w * d->cin * (x3 ? 2 : 1);
    if (in_elems > 0x7fffffffLL) return ppn::fail(PPN_E_UNSUPPORTED, "tensor too large for 32-bit indexing");
    if (d->src2 && (size_t)d->batch * d->in2_h * d->in2_w * d->cin2 * 4 >= 0x7fffff00ull)
        return ppn::fail(PPN_E_UNSUPPORTED, "second source too large for the buffer-addressed conv kernel");
    // BatchNorm statistics from the epilogue: a request, not a demand.  Delivered under the conditions of the single-output 16-bit
    // epilogue (conv_big.hip `fast`) + one launch over the whole tensor + no more pixel tiles than a BatchNorm workspace has
    // partial blocks (train.hip kMaxBlocks)
    const long long n_ptiles = (m + bp - 1) / bp;
    s->stats = d->stats_mode != 0 && big && big_stats_ok(k, d->dtype, bt) && !d->out_nchw_f32 && !d->residual && !d->out_act &&
               d->out_raw && d->cout % 8 == 0 && !(d->flags & PPN_CONV_OUT_BF16) && !d->src2 && !d->argmax_keys && d->m_count == 0 &&
               n_ptiles <= 1024;
    s->stats_tiles = s->stats ? (int)n_ptiles : 0;
    ConvKArgs& a = s->args;
    fill_args(d, m_lo, m_hi, bp, bc, kmain / bk, s->stats, &a);
    if (a.out_plain && (!x3 || d->out_nchw_f32))
        return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_X3_PLAIN_OUT: a PPN_F16X3 launch with NHWC outputs");
    if (a.out_bf16 && (d->dtype != PPN_F16 || !big || d->out_nchw_f32))
        return ppn::fail(PPN_E_UNSUPPORTED, "PPN_CONV_OUT_BF16: a PPN_F16 launch of the large-tile kernel with NHWC outputs");
    if (x3 && !big) return ppn::fail(PPN_E_UNSUPPORTED, "PPN_F16X3 is implemented by the large-tile kernel only");
    s->bp = bp; s->bc = bc;
    s->smallc = smallc;
    if (!big) {
        if (d->argmax_keys) return ppn::fail(PPN_E_UNSUPPORTED, "fused arg-max is implemented by the large-tile kernel only");
        if (d->src2) return ppn::fail(PPN_E_UNSUPPORTED, "the fused shortcut is implemented by the large-tile kernel only");
        s->kernel = Kernel::Generic;
        s->nw = 4;
        return PPN_OK;
    }
    s->kernel = Kernel::Big;
    // buffer descriptors address up to 2 GiB with the out-of-range marker used for padding
    const size_t es = d->dtype == PPN_F32 ? 4 : 2;
    if ((size_t)a.B * a.H * a.W * a.Cin * es >= 0x7fffff00ull || (size_t)a.n_ctiles * bt.bc * a.Ktot * es >= 0x7fffff00ull)
        return ppn::fail(PPN_E_UNSUPPORTED, "tensor too large for the buffer-addressed conv kernel");
    s->x3 = x3;
    s->shortcut = d->src2 != nullptr;
    s->nw = 8;
    if (!x3 && k.waves == 4 && bt.bp != 144) {
        s->nw = 4;
        // there is no 4-wave 64-channel instantiation: as before, such a launch runs the 128-channel one (PPN_CONV_WAVES=4 is a
        // tuning knob for the 128 / 256-channel tiles)
        if (s->bc == 64) s->bc = 128;
    }
    if (s->shortcut && !(s->nw == 8 && s->bc >= 128))
        return ppn::fail(PPN_E_UNSUPPORTED, "fused shortcut needs the 8-wave 128/256-channel tiles");
    if (!x3 && d->dtype != PPN_F32 && strip_eligible(k, a, d->dtype, bt, &a.sp_rows, &a.sp_pitch)) {
        a.sp_div = make_fastdiv((unsigned)a.sp_pitch);
        s->strip = true;
    }
    if (a.pf_lines) {                                                 // prefetch hint: lines per workgroup, at most two per thread
        const unsigned nwg = (unsigned)(a.n_ctiles * a.n_ptiles);
        a.pf_per_wg = std::min<unsigned>((a.pf_lines + nwg - 1) / nwg, 2u * 64 * s->nw);
    }
    return PPN_OK;
}

}  // namespace

int conv_route(const ppn_conv_desc* d, const RouteKnobs& k, ConvRoute* out) {
    *out = ConvRoute{};
    out->n = 1;
    if (!d) return ppn::fail(PPN_E_INVALID, "conv desc is NULL");
    if (d->flags & PPN_CONV_SPLIT_K) {
        out->seg[0].dtype = d->dtype;
        return route_splitk(d, &out->seg[0]);
    }
    if (d->stats_mode != 0) {
        if (d->stats_mode < 1 || d->stats_mode > 2 || !d->stats_partial || !d->stats_tiles)
            return ppn::fail(PPN_E_INVALID, "stats_mode 1 or 2 needs stats_partial and stats_tiles");
        if (d->stats_mode == 2 && (!d->stats_x || !d->stats_gamma || !d->stats_beta || !d->stats_mean || !d->stats_rstd ||
                                   d->stats_act < PPN_ACT_NONE || d->stats_act > PPN_ACT_LRELU))
            return ppn::fail(PPN_E_INVALID, "stats_mode 2 needs stats_x, gamma, beta, mean, rstd and act none / relu / lrelu");
        out->stats_asked = true;
    }
    if (!dtype_ok(d->dtype)) return ppn::fail(PPN_E_INVALID, "bad dtype %d", d->dtype);
    long long cut = 0;
    if (const int rc = route_segment(d, k, &out->seg[0], &cut)) return rc;
    if (cut == 0) return PPN_OK;
    const long long m_all = out->seg[0].m_hi;
    ppn_conv_desc part = *d;
    for (int i = 0; i < 2; ++i) {
        part.m_begin = (int32_t)(i ? cut : 0); part.m_count = (int32_t)(i ? m_all - cut : cut);
        out->seg[i] = ConvSegment{};
        long long none = 0;
        if (const int rc = route_segment(&part, k, &out->seg[i], &none)) return rc;
    }
    out->n = 2;
    return PPN_OK;
}

int route_strip(const ConvRoute& r) {
    int strip = 0;
    for (int i = 0; i < r.n; ++i)
        if (r.seg[i].kernel == Kernel::Big && (r.seg[i].dtype == PPN_BF16 || r.seg[i].dtype == PPN_F16)) strip = r.seg[i].strip ? 1 : 0;
    return strip;
}

const char* kernel_name(const ConvSegment& s) {
    // interned by what the name is made of; a few dozen instantiations exist
    struct Entry { unsigned key; char name[96]; };
    static Entry table[256];
    static int n = 0;
    static std::mutex mu;
    const bool f32 = s.dtype == PPN_F32;
    const char* elem = f32 ? "float" : ((s.dtype == PPN_F16 || s.dtype == PPN_F16X3) ? "_Float16" : "__bf16");
    const unsigned variant = s.kernel == Kernel::Generic ? (s.smallc ? 1u : 0u)
                           : s.kernel == Kernel::Big ? (s.shortcut ? 1u : 0u) | (s.x3 ? 2u : 0u) | (s.stats ? 4u : 0u) : 0u;
    const unsigned key = 1u + (unsigned)s.kernel + 8u * ((unsigned)s.dtype & 3u) + 32u * ((unsigned)s.bp & 511u) +
                         (32u << 9) * ((unsigned)s.bc & 511u) + (32u << 18) * ((unsigned)s.nw & 15u) + (32u << 22) * variant;
    std::lock_guard<std::mutex> lock(mu);
    for (int i = 0; i < n; ++i)
        if (table[i].key == key) return table[i].name;
    if (n == 256) return "?";                          // cannot happen with the instantiations that exist; never reuse a slot
    Entry& e = table[n++];
    e.key = key;
    switch (s.kernel) {
        case Kernel::Stem3x3: snprintf(e.name, sizeof(e.name), "stem3x3_kernel<%s, %d, %d>", f32 ? "float" : "__bf16", s.bc, s.bp); break;
        case Kernel::Conv64: snprintf(e.name, sizeof(e.name), "conv64_kernel<%s>", elem); break;
        case Kernel::HeadLimb: snprintf(e.name, sizeof(e.name), "head_limb_argmax_kernel<%s>", elem); break;
        case Kernel::SplitK: snprintf(e.name, sizeof(e.name), "conv_splitk_partial_kernel<%s, %d, %d, 2, 2>", elem, s.bp, s.bc); break;
        case Kernel::Generic:
            snprintf(e.name, sizeof(e.name), "conv_igemm_kernel<%s, %d, %d, %d, %d, %s>", elem, s.bp, s.bc, s.bc <= 32 ? 4 : 2,
                     s.bc <= 32 ? 1 : 2, s.smallc ? "true" : "false");
            break;
        case Kernel::Big:
            snprintf(e.name, sizeof(e.name), "conv_igemm_big_kernel<%s, %d, %d, %d, %s%s>", elem, s.bp, s.bc, s.nw,
                     s.shortcut ? "true" : "false", s.x3 ? ", true" : (s.stats ? ", false, true" : ""));
            break;
    }
    return e.name;
}

}  // namespace ppnconv

// ---- host-only entry points ---------------------------------------------------------------------------------------------------
using namespace ppnconv;

extern "C" int ppn_conv_tiling(int32_t dtype, int32_t cin, int32_t cout, int32_t ksize, int32_t* k_step,
                               int32_t* cout_tile, int32_t* k_order) {
    if (!dtype_ok(dtype)) return ppn::fail(PPN_E_INVALID, "bad dtype %d", dtype);
    if (cin < 1 || cout < 1 || ksize < 1) return ppn::fail(PPN_E_INVALID, "bad conv shape");
    const int bk = dtype == PPN_F32 ? 32 : 64;
    if (dtype == PPN_F16X3 && (cin % bk != 0 || cout < 64))
        return ppn::fail(PPN_E_UNSUPPORTED, "PPN_F16X3 needs cin %% 64 == 0 and cout >= 64 (run the layer as PPN_F32)");
    if (cin == 16 && (cout == 16 || cout == 32) && ksize == 3) {
        // direct small-channel kernel (stem3x3.hip): weights stay in the reference layout, f32, unpadded
        if (k_step) *k_step = 144;
        if (cout_tile) *cout_tile = cout;
        if (k_order) *k_order = 2;
        return PPN_OK;
    }
    if (k_step) *k_step = bk;
    const bool big = (cin % bk == 0) && cout >= 64;                   // the layers big_tile_for() finds a tile for
    if (cout_tile) *cout_tile = big ? pad_tile_for(cout) : choose_tile(cout).bc;
    if (k_order) *k_order = big ? 1 : 0;
    return PPN_OK;
}

extern "C" int ppn_conv_split(int32_t dtype, int32_t cin, int32_t cout, int64_t m, int64_t* m_split) {
    if (!dtype_ok(dtype)) return ppn::fail(PPN_E_INVALID, "bad dtype %d", dtype);
    if (cin < 1 || cout < 1 || m < 1 || !m_split) return ppn::fail(PPN_E_INVALID, "ppn_conv_split: bad arguments");
    const int bk = dtype == PPN_F32 ? 32 : 64;
    const long long cut = (cin % bk == 0) ? big_split_for(knobs(), cout, m) : 0;
    *m_split = (cut > 0 && cut < m) ? cut : 0;
    return PPN_OK;
}

extern "C" int ppn_conv_splitk_workspace(const ppn_conv_desc* d, int64_t* bytes, int32_t* slabs) {
    ppnsplitk::Partition p;
    if (const int rc = splitk_check(d, &p)) return rc;
    if (bytes) *bytes = p.ws_bytes;
    if (slabs) *slabs = p.slabs;
    return PPN_OK;
}

extern "C" int ppn_set_conv_tile_override(int32_t bp, int32_t bc) {
    if (!(bp == 0 && bc == 0) && !tile_shape_ok(bp, bc))
        return ppn::fail(PPN_E_INVALID, "ppn_set_conv_tile_override: bp in {128,192,256}, bc in {64,128,256}, not 192x64; or 144x256");
    knobs().ov_bp = bp; knobs().ov_bc = bc;
    return PPN_OK;
}

extern "C" int ppn_set_conv_strip_enabled(int32_t on) {
    knobs().strip_on = on ? 1 : 0;
    return PPN_OK;
}

extern "C" int ppn_set_conv64_enabled(int32_t on) {
    knobs().conv64_on = on ? 1 : 0;
    return PPN_OK;
}

extern "C" int ppn_set_conv_tile_policy(int32_t policy) {
    if (policy < 0 || policy > 2) return ppn::fail(PPN_E_INVALID, "ppn_set_conv_tile_policy: 0, 1 or 2");
    knobs().tile_policy = policy;
    return PPN_OK;
}
