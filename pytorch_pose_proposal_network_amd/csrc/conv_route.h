// Which kernel a ppn_conv_desc runs on, as data: conv_route() validates the descriptor, picks the kernel, the tile, the pixel
// segments, the strip loader and the BatchNorm-statistics epilogue, and fills the kernel arguments; the launchers (conv.hip and the
// kernels' own files) only launch what it says.  Host-only, no HIP types: the same functions are compiled into libppn.so and into
// tools/conv_route_check.cpp, a stand-alone program that runs under the host sanitizers (tests/test_conv_route_cpu.py).
#pragma once
#include "conv_args.h"
#include "error.h"
#include "splitk_partition.h"

namespace ppnconv {

// The process-wide tuning knobs of the dispatch.  knobs() reads the environment once, at its first use; the ppn_set_conv_* entry
// points change the one instance afterwards (or before: a setter's first use of knobs() reads the environment first).
struct RouteKnobs {
    int tile_policy;      // ppn_set_conv_tile_policy; PPN_CONV_CONT in the environment = 1
    int ov_bp, ov_bc;     // ppn_set_conv_tile_override / PPN_CONV_TILE="bp,bc": forced large tile, 0,0 = automatic
    int conv64_on;        // ppn_set_conv64_enabled / PPN_CONV64=0
    int strip_on;         // ppn_set_conv_strip_enabled / PPN_CONV_STRIP=0
    int waves;            // PPN_CONV_WAVES (8)
    int policy1_mask;     // PPN_POLICY1_MASK (7)
    double eff144;        // PPN_EFF144 (0.90)
};
RouteKnobs& knobs();

enum class Kernel { Stem3x3, Conv64, HeadLimb, Big, Generic, SplitK };

struct ConvSegment {      // one launch (SplitK: its pair of launches) over output pixels [m_lo, m_hi)
    Kernel kernel;
    int dtype;
    long long m_lo, m_hi;
    // what selects the template instantiation.  Generic / Big / SplitK: the pixel x channel tile; Stem3x3: bc = Cout, bp = stride
    int bp, bc, nw;
    bool smallc, shortcut, x3, stats, strip;
    int stats_tiles;                  // what *d->stats_tiles receives
    ConvKArgs args;                   // Big / Generic / SplitK, complete
    ppnsplitk::Partition splitk;      // SplitK
};

struct ConvRoute {
    int n;                            // segments; 2: the two-segment launch of tile policy 2
    bool stats_asked;                 // a valid stats_mode request: *d->stats_tiles is written, 0 unless seg[0].stats
    ConvSegment seg[2];
};

// PPN_OK, or the error (code and ppn_last_error text) the descriptor is rejected with.  Writes nothing through d.
int conv_route(const ppn_conv_desc* d, const RouteKnobs& k, ConvRoute* out);

// The kernel's name as rocprofv3 --kernel-trace prints it (a substring of the demangled symbol); the storage lives as long as
// the process.
const char* kernel_name(const ConvSegment& s);

// ppn_last_conv_strip of a route: the strip flag of its last 16-bit large-tile segment
int route_strip(const ConvRoute& r);

}  // namespace ppnconv
