// mcc_omnicalib_host.hpp -- host helpers shared by mcc_omnicalib_api.cpp and mcc_omnistereo_api.cpp:
// the error path of the C ABI and an owning device buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "mcc_omnicalib_internal.h"

namespace {

int oc_fail(int code, const std::string& msg) { return mcc_internal_fail(code, msg.c_str()); }

#define OCCHK(expr)                                                                          \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) return oc_fail(MCC_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T>
struct DBuf {
    T* p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
    hipError_t upload(const T* h, size_t n) {
        hipError_t e = alloc(n);
        if (e == hipSuccess && n) e = hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
};

// flags2idx (src/omnidir.cpp:2031-2076) for the 10 intrinsics: 1 = free, 0 = fixed.  The cascade
// of >= tests is the reference's (CALIB_USE_GUESS is not handled there either).  flags2idxStereo
// (:2078-2135) applies the same cascade to both cameras' intrinsics.
void intrinsic_mask(int flags, double* m) {
    for (int i = 0; i < 10; ++i) m[i] = 1.0;
    int f = flags;
    if (f >= MCC_OMNI_CALIB_FIX_CENTER) { m[3] = m[4] = 0; f -= MCC_OMNI_CALIB_FIX_CENTER; }
    if (f >= MCC_OMNI_CALIB_FIX_GAMMA) { m[0] = m[1] = 0; f -= MCC_OMNI_CALIB_FIX_GAMMA; }
    if (f >= MCC_OMNI_CALIB_FIX_XI) { m[5] = 0; f -= MCC_OMNI_CALIB_FIX_XI; }
    if (f >= MCC_OMNI_CALIB_FIX_P2) { m[9] = 0; f -= MCC_OMNI_CALIB_FIX_P2; }
    if (f >= MCC_OMNI_CALIB_FIX_P1) { m[8] = 0; f -= MCC_OMNI_CALIB_FIX_P1; }
    if (f >= MCC_OMNI_CALIB_FIX_K2) { m[7] = 0; f -= MCC_OMNI_CALIB_FIX_K2; }
    if (f >= MCC_OMNI_CALIB_FIX_K1) { m[6] = 0; f -= MCC_OMNI_CALIB_FIX_K1; }
    if (f >= MCC_OMNI_CALIB_FIX_SKEW) m[2] = 0;
}

}  // namespace
