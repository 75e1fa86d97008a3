// How the host side reports an error: fail() keeps the message hgs_last_error() returns (one per thread) and hands the
// code back; HIPCHK / LCHK turn a HIP status / a launcher's status into HGS_ERR_DEVICE with the place it happened.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/hgs.h"

namespace hgs {

inline thread_local std::string g_err;
inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

}  // namespace hgs

#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess)                                                                  \
            return fail(HGS_ERR_DEVICE, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define LCHK(x)                                                                                \
    do {                                                                                       \
        int e_ = (x);                                                                          \
        if (e_ != 0)                                                                           \
            return fail(HGS_ERR_DEVICE, "kernel launch failed: %s (%s:%d)",                    \
                        hipGetErrorString((hipError_t)e_), __FILE__, __LINE__);                \
    } while (0)
