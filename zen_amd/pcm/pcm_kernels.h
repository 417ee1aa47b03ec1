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
// the same two for packed 24-bit samples (three little-endian bytes each, no alignment asked of the packed side)
hipError_t launch_to_float24(const uint8_t* src, int channels, size_t n_frames, float* dst, hipStream_t s);
hipError_t launch_from_float24(const float* src, size_t n, int mode, float gain, const float* minmax, uint8_t* dst, hipStream_t s);
// by format (ZEN_PCM_FMT_I16 or ZEN_PCM_FMT_I24, checked by the caller): the pipeline's two launch sites
hipError_t launch_unpack(int fmt, const void* src, int channels, size_t n_frames, float* dst, hipStream_t s);
hipError_t launch_pack(int fmt, const float* src, size_t n, int mode, float gain, const float* minmax, void* dst, hipStream_t s);
// `pairs` (<= 64) pairs of (+inf, -inf) at minmax
hipError_t launch_minmax_init(float* minmax, int pairs, hipStream_t s);

} // namespace zen_pcm
