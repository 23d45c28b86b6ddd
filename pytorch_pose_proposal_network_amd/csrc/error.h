// Error reporting of libppn: a return code plus a thread-local message (ppn_last_error).  Host-only, no HIP types.
#pragma once
#include <cstdarg>
#include <cstdio>

#include "../../include/ppn.h"

namespace ppn {

char* error_buffer();  // thread-local, 512 bytes (abi.cpp)

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace ppn
