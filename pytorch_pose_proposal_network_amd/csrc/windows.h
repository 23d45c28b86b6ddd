// The window layout's own refusals (include/ppn.h: ppn_window_layout), shared by ppn_ingest_windows and ppn_merge_windows.
// Host-only, no HIP types.
#pragma once
#include "error.h"

namespace ppn {

// PPN_OK, or PPN_E_INVALID with a message that starts with `who`.
inline int check_layout(const char* who, const ppn_window_layout* lay) {
    if (!lay) return fail(PPN_E_INVALID, "%s: NULL layout", who);
    if (lay->n < 1 || lay->n > PPN_MAX_WINDOWS)
        return fail(PPN_E_INVALID, "%s: %d windows outside 1..%d", who, lay->n, PPN_MAX_WINDOWS);
    for (int i = 0; i < lay->n; ++i) {
        const ppn_window& w = lay->win[i];
        if (w.h < 1 || w.w < 1 || w.y0 < 0 || w.x0 < 0)
            return fail(PPN_E_INVALID, "%s: window %d is (%d, %d) %dx%d", who, i, w.y0, w.x0, w.h, w.w);
    }
    return PPN_OK;
}

}  // namespace ppn
