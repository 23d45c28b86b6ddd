// Stand-alone driver of the conv dispatch (csrc/conv_route.cpp) for tests/test_conv_route_cpu.py: reads descriptors and knob states
// as text, routes each and prints what the route says.  No GPU, no HIP; built with the host sanitizers.
//
// stdin, one entry per line:   NULL   |   <the 53 fields of ppn_conv_desc in declaration order> <policy ov_bp ov_bc conv64 strip>
//   (pointer fields: 0 = NULL, 1 = some address, 2 = an address that is not 16-byte aligned)
// stdout, one line per entry, tab-separated:
//   rc  error-text  n  split  { kind  name  m_lo  m_hi  strip  stats_tiles  bp  bc  n_ptiles  n_ctiles } x n   route_strip
//   (split: ppn_conv_split's cut for the descriptor's shape under the same policy, through the ppn_set_conv_* entry points)
#include <cstdint>
#include <cstdio>
#include <sstream>
#include <string>
#include <iostream>

#include "conv_route.h"

namespace ppn {
char* error_buffer() {
    static thread_local char buf[512];
    return buf;
}
}  // namespace ppn

extern "C" const char* ppn_last_error(void) { return ppn::error_buffer(); }

static void* ptr(long long v) { return v == 0 ? nullptr : reinterpret_cast<void*>(static_cast<uintptr_t>(v == 2 ? 0x1004 : 0x1000)); }

int main() {
    using namespace ppnconv;
    static const char* kinds[] = {"stem3x3", "conv64", "head_limb", "big", "generic", "splitk"};
    std::string line;
    int32_t tiles_slot = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        ppn::error_buffer()[0] = 0;
        RouteKnobs k = knobs();                       // the defaults (no PPN_* variable is set in the test's environment)
        ConvRoute r;
        int rc;
        long long split = 0;
        if (line == "NULL") {
            rc = conv_route(nullptr, k, &r);
        } else {
            std::istringstream in(line);
            long long v[58];
            for (int i = 0; i < 58; ++i)
                if (!(in >> v[i])) { fprintf(stderr, "bad input line: %s\n", line.c_str()); return 2; }
            ppn_conv_desc d{};
            int i = 0;
            d.dtype = (int32_t)v[i++]; d.batch = (int32_t)v[i++]; d.in_h = (int32_t)v[i++]; d.in_w = (int32_t)v[i++];
            d.cin = (int32_t)v[i++]; d.out_h = (int32_t)v[i++]; d.out_w = (int32_t)v[i++]; d.cout = (int32_t)v[i++];
            d.ksize = (int32_t)v[i++]; d.stride = (int32_t)v[i++]; d.dilation = (int32_t)v[i++]; d.pad = (int32_t)v[i++];
            d.k_total = (int32_t)v[i++]; d.cout_pad = (int32_t)v[i++]; d.act1 = (int32_t)v[i++]; d.act2 = (int32_t)v[i++];
            d.out_nchw_f32 = (int32_t)v[i++];
            d.src = ptr(v[i++]); d.weight = ptr(v[i++]);
            d.scale1 = static_cast<const float*>(ptr(v[i++])); d.shift1 = static_cast<const float*>(ptr(v[i++]));
            d.residual = ptr(v[i++]); d.out_raw = ptr(v[i++]);
            d.scale2 = static_cast<const float*>(ptr(v[i++])); d.shift2 = static_cast<const float*>(ptr(v[i++]));
            d.out_act = ptr(v[i++]); d.zero_page = ptr(v[i++]);
            d.src2 = ptr(v[i++]); d.in2_h = (int32_t)v[i++]; d.in2_w = (int32_t)v[i++]; d.cin2 = (int32_t)v[i++];
            d.stride2 = (int32_t)v[i++];
            d.unary_out = static_cast<float*>(ptr(v[i++])); d.argmax_keys = static_cast<decltype(d.argmax_keys)>(ptr(v[i++]));
            d.unary_channels = (int32_t)v[i++]; d.limb_window = (int32_t)v[i++]; d.m_begin = (int32_t)v[i++];
            d.m_count = (int32_t)v[i++]; d.limb_edge_pad = (int32_t)v[i++]; d.flags = (int32_t)v[i++];
            d.prefetch = ptr(v[i++]); d.prefetch_bytes = v[i++];
            d.stats_partial = ptr(v[i++]); d.stats_mode = (int32_t)v[i++]; d.stats_act = (int32_t)v[i++];
            d.stats_x = ptr(v[i++]);
            d.stats_gamma = static_cast<const float*>(ptr(v[i++])); d.stats_beta = static_cast<const float*>(ptr(v[i++]));
            d.stats_mean = static_cast<const float*>(ptr(v[i++])); d.stats_rstd = static_cast<const float*>(ptr(v[i++]));
            d.stats_tiles = v[i++] ? &tiles_slot : nullptr;
            d.splitk_ws = ptr(v[i++]); d.splitk_ws_bytes = v[i++];
            k.tile_policy = (int)v[i++]; k.ov_bp = (int)v[i++]; k.ov_bc = (int)v[i++]; k.conv64_on = (int)v[i++];
            k.strip_on = (int)v[i++];
            tiles_slot = -7;
            rc = conv_route(&d, k, &r);
            if (tiles_slot != -7) { fprintf(stderr, "conv_route wrote through the descriptor\n"); return 3; }
            // the same policy through the process-wide knobs and the public entry point
            if (ppn_set_conv_tile_policy(k.tile_policy) != PPN_OK || ppn_set_conv_tile_override(k.ov_bp, k.ov_bc) != PPN_OK ||
                ppn_set_conv64_enabled(k.conv64_on) != PPN_OK || ppn_set_conv_strip_enabled(k.strip_on) != PPN_OK)
                return 4;
            int64_t cut = 0;
            const long long m_all = (long long)d.batch * d.out_h * d.out_w;
            if (rc == PPN_OK && ppn_conv_split(d.dtype, d.cin, d.cout, m_all, &cut) == PPN_OK) split = cut;
        }
        printf("%d\t%s\t%d\t%lld", rc, rc == PPN_OK ? "" : ppn::error_buffer(), rc == PPN_OK ? r.n : 0, split);
        for (int i = 0; rc == PPN_OK && i < r.n; ++i) {
            const ConvSegment& s = r.seg[i];
            const bool has_args = s.kernel == Kernel::Big || s.kernel == Kernel::Generic || s.kernel == Kernel::SplitK;
            printf("\t%s\t%s\t%lld\t%lld\t%d\t%d\t%d\t%d\t%d\t%d", kinds[(int)s.kernel], kernel_name(s), s.m_lo, s.m_hi, s.strip ? 1 : 0,
                   s.stats_tiles, s.bp, s.bc, has_args ? s.args.n_ptiles : 0, has_args ? s.args.n_ctiles : 0);
        }
        printf("\t%d\n", rc == PPN_OK ? route_strip(r) : 0);
    }
    return 0;
}
