// multi_kernels.h -- launchers of the kernels of libzen_hip_multi.so (multi_kernels.hip), for multi.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

namespace zen_multi {

// the tile of split and join: TILE samples (frames x channels) in LDS, one pad word behind every 32
constexpr int TILE = 2048;
constexpr int TILE_WORDS = TILE + TILE / 32;

// fmt, mode: the values of zen_hip_multi.h.  Every launcher returns at once for n_frames == 0.
hipError_t launch_split(int fmt, const void* src, int channels, size_t n_frames, float* rows, size_t row_stride, hipStream_t s);
hipError_t launch_peak(const float* rows, int channels, size_t n_frames, size_t row_stride, float* minmax, hipStream_t s);
hipError_t launch_join(int fmt, const float* rows, int channels, size_t n_frames, size_t row_stride, int mode, float gain,
                       const float* minmax, void* dst, hipStream_t s);
// minmax[2 i] = +inf, minmax[2 i + 1] = -inf for i < pairs (at most 32)
hipError_t launch_minmax_init(float* minmax, int pairs, hipStream_t s);
// peaks[i] = pcm16_peak_of(minmax[2 i], minmax[2 i + 1]) where bit i of `active` is set and the pair saw a sample, else 0
hipError_t launch_peaks_of(const float* minmax, int pairs, unsigned active, float* peaks, hipStream_t s);

} // namespace zen_multi
