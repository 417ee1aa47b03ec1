// Stand-in for <hip/hip_runtime.h> where a device header is compiled as plain C++ on the CPU
// (tests/cpp/test_blockrun_first_pass_host.cpp puts this directory in front of the include path): just what
// zen_amd/csrc/fft_dev.h names outside the code that test instantiates.
#pragma once
#include <cmath>

#define __device__
#define __forceinline__ inline
#define __restrict__
struct float2 {
	float x, y;
};
static inline float2 make_float2(float x, float y) { return {x, y}; }
struct alignas(16) float4 { // zen_amd/addon/median_select.h (tests/cpp/test_addon_median_host.cpp)
	float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
// (named by functions of fft_dev.h the host test never calls)
#define __builtin_amdgcn_fence(order, scope) ((void)0)
#define __builtin_amdgcn_wave_barrier() ((void)0)
#define __builtin_amdgcn_rsq(x) (1.0 / std::sqrt(x))
static inline void __syncthreads() {}
