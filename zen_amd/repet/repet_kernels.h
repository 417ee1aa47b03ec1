// repet_kernels.h -- launch interface of the kernels of libzen_hip_repet.so (repet_kernels.hip).
// A call works on n_clips clips of n samples, m frames each.  The spectra are packed clip by clip: row c * m + k holds the N
// complex values of frame k of clip c, so one batched transform covers the call.  V holds the magnitudes of the bins 0..H,
// one row of v_stride floats (a multiple of 4: 16-byte loads) per frame, packed alike.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../addon/stft_args.h"

namespace zen_repet {

enum { MAX_SEGMENTS = 256, REGISTER_SEGMENTS = 32 }; // counts up to REGISTER_SEGMENTS are sorted in registers, the rest in LDS

using zen_addon::FrameArgs; // ../addon/stft_args.h, with the layout of a call's rows
using zen_addon::MagArgs;

struct LagArgs { // one clip: V (m rows) -> bins rows of L complex values (V^2, 0), zeros from m on
	const float* v;
	float* lag;
	size_t v_stride, m, L;
	int bins;
};

struct PowerArgs { // (re re + im im, 0) in place over count complex values
	float* z;
	size_t count;
};

struct BrawArgs { // braw[j] = sum over the bins in order of lag[f][j].re / (float)(m - j)
	const float* lag;
	float* braw;
	size_t m, L;
	int bins;
};

struct MedianArgs { // one clip or a caller's V
	const float* v;
	float* s; // period rows of s_stride floats
	size_t v_stride, s_stride, m, bins, period;
};

struct MaskArgs { // one clip, in place on its spectra
	float* rows;
	const float* v;
	const float* s;
	size_t v_stride, m, period;
	int N, kc;
};

struct OlaArgs { // one clip
	const float* rows; // inverse-transformed frames (NULL with period 0)
	const float* in;
	const float* div; // H floats
	float *background, *foreground; // either may be NULL
	size_t n, period; // period 0: background +0, foreground the input's bits
	int N;
};

// the first two are ../addon/stft_kernels.h's as this library compiled them; hidden: their names spell a type of zen_addon,
// and nothing of zen_amd/addon is among a library's dynamic symbols
__attribute__((visibility("hidden"))) hipError_t launch_frame(const FrameArgs& a, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_magnitude(const MagArgs& a, hipStream_t s);
hipError_t launch_lag_rows(const LagArgs& a, hipStream_t s);
hipError_t launch_power(const PowerArgs& a, hipStream_t s);
hipError_t launch_braw(const BrawArgs& a, hipStream_t s);
hipError_t launch_segment_median(const MedianArgs& a, hipStream_t s);
hipError_t launch_mask(const MaskArgs& a, hipStream_t s);
hipError_t launch_overlap_add(const OlaArgs& a, hipStream_t s);

} // namespace zen_repet
