// pitch_kernels.h -- launch interface of the three kernels of libzen_hip_pitch.so (pitch_kernels.hip).
// A slice is `chunks` chunks of each of `n_streams` streams; its workspace rows are packed stream by stream: row w =
// s * chunks + c holds 2n complex values in z (the transforms run in place on it) and n + 1 doubles in prefix.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace zen_pitch {

struct PadArgs {
	const float* in; // chunk c of stream s of this slice: in + s * in_stride + (c0 + c) * step
	size_t in_stride, step, c0;
	float* z;       // 4n floats per row
	double* prefix; // n + 1 doubles per row
	size_t chunks, n_streams;
	int n;
};

struct PickArgs {
	const float* z; // after the inverse transform: r[t] = z[row][2t]
	const double* prefix;
	float *pitch, *period, *clarity, *nsdf; // any may be NULL; element (s, c0 + c) of rows out_stride apart (nsdf: times n)
	size_t out_stride, c0;
	size_t chunks, n_streams;
	int n;
	float fs;
};

size_t pick_lds_bytes(int n);
hipError_t prepare_pick(int n); // once per process and n: lets the kernel use the LDS a chunk of n needs
hipError_t launch_pad(const PadArgs& a, hipStream_t s);
hipError_t launch_power(float* z, size_t bins, hipStream_t s); // z[k] = (re^2 + im^2, 0) on `bins` complex values, bins % 2 == 0
hipError_t launch_pick(const PickArgs& a, hipStream_t s);

} // namespace zen_pitch
