// pcm_kernels.h -- launchers of pcm_kernels.hip, for pcm_pipe.hip.  All asynchronous on `s`; n == 0 launches nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace zen_pcm {

hipError_t launch_to_float(const int16_t* src, int channels, size_t n_frames, float* dst, hipStream_t s);
hipError_t launch_peak(const float* src, size_t n, float* minmax, hipStream_t s);
// mode: ZEN_PCM_MODE_PEAK (divides by max(-minmax[0], minmax[1])) or ZEN_PCM_MODE_GAIN (multiplies by gain)
hipError_t launch_from_float(const float* src, size_t n, int mode, float gain, const float* minmax, int16_t* dst, hipStream_t s);
// `pairs` (<= 64) pairs of (+inf, -inf) at minmax
hipError_t launch_minmax_init(float* minmax, int pairs, hipStream_t s);

} // namespace zen_pcm
