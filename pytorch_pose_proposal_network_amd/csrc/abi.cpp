// libppn: error channel, version (see include/ppn.h) and the one process-wide switch read from the environment that belongs to no
// kernel family's dispatch (the conv knobs are in conv_route.cpp).
#include <cstdlib>

#include "common.h"

namespace ppn {
char* error_buffer() {
    static thread_local char buf[512] = {0};
    return buf;
}
// PPN_PACK_TILED=0: ppn_pack_table_build (conv.hip) leaves out the tiled 16-bit packs (A/B switch)
bool pack_tiled_enabled() {
    static const bool on = !(getenv("PPN_PACK_TILED") && atoi(getenv("PPN_PACK_TILED")) == 0);
    return on;
}
}  // namespace ppn

extern "C" const char* ppn_last_error(void) { return ppn::error_buffer(); }
extern "C" int ppn_version(void) { return 2; }
