// Stand-in for <hip/hip_runtime.h> when the device math of csrc/mcc_device.hpp and
// csrc/mcc_pnp_device.hpp is compiled for the host (tests/cpp/test_pnp_replay.cpp): the qualifiers
// vanish and the math functions are the C library's.
#pragma once
#include <cmath>
#define __device__
#define __forceinline__ inline
