// Stand-in for <hip/hip_runtime.h> when the device math of csrc/mcc_device.hpp and
// csrc/mcc_pnp_device.hpp is compiled for the host (tests/cpp/test_pnp_replay.cpp): the qualifiers
// vanish and the math functions are the C library's.  The two handle types are here for the launch
// declarations of the csrc/*_internal.h headers (tests/cpp/test_pinloop_policy.cpp); nothing calls them.
#pragma once
#include <cmath>
#include <cstddef>
#define __host__
#define __device__
#define __forceinline__ inline
typedef int hipError_t;
typedef struct ihipStream_t* hipStream_t;
