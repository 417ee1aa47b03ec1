// stft_args.h -- the arguments of the two kernels every spectrogram add-on starts with (zen_amd/repet, repsim, nmf): what a
// library's host source (through stft_host.h) hands to its kernel source (through stft_kernels.h).
// A call works on n_clips clips of n samples, m frames each.  The spectra are packed clip by clip: row c * m + k holds the N
// complex values of frame k of clip c, so one batched transform covers the call.  V holds the magnitudes of the bins 0..H,
// one row of v_stride floats (a multiple of 4: 16-byte loads) per frame, packed alike.
#pragma once

#include <stddef.h>

namespace zen_addon {

struct FrameArgs {
	const float* in;  // clip c: in + c * in_stride, n samples
	const float* win; // N floats
	float* rows;      // n_clips * m rows of N complex values
	size_t in_stride, n, m, n_clips;
	int N;
};

struct MagArgs {
	const float* rows;
	float* v; // rows of v_stride floats; the floats behind bin H are written as +0
	size_t v_stride, frames; // frames = n_clips * m
	int N;
};

} // namespace zen_addon
