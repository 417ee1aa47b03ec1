// tsm_kernels.h -- launch interface of the kernels of libzen_hip_tsm.so (tsm_kernels.hip).
// A call works on n_clips clips of n samples, M vocoder frames each.  The spectra are packed clip by clip: row c * M + m holds
// the N complex values of frame m of clip c, so one batched transform covers the call.  mag, theta, e and psi hold the bins
// 0..H of a frame in rows of `stride` words (a multiple of 4), packed alike; owner in rows of `stride` 16-bit words.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace zen_tsm {

enum { COARSE = 2048, FINE = 2048, ATAN_STEPS = 256 };

struct Framing { // one route: a_m = floor((double)((m - V / 2 + 1) Hs) / alpha)
	double alpha;
	int N, Hs, V;
};

struct FrameArgs {
	const float* in;  // clip c: in + c * in_stride, n samples
	const float* win; // N floats
	float* rows;      // n_clips * M rows of N complex values
	size_t in_stride, n, M, n_clips;
	Framing fr;
};

struct AnalysisArgs {
	const float* rows;
	float* mag;      // the words behind bin H of a row are written as 0, as theta's
	uint32_t* theta;
	size_t stride, frames; // frames = n_clips * M
	int N;
};

struct PeakArgs { // own_m[k], and e_m[k] = inc_m[own] + theta_m[k] - theta_m[own] (theta_0[k] for the first frame of a clip)
	const float* mag;
	const uint32_t* theta;
	uint16_t* owner;
	uint32_t* e;
	size_t stride, M, frames;
	Framing fr;
};

struct WalkArgs { // psi_m[k] = psi_{m-1}[own_m[k]] + e_m[k], psi_{-1} = 0: one workgroup per clip
	const uint16_t* owner;
	const uint32_t* e;
	uint32_t* psi;
	size_t stride, M, n_clips;
	int bins;
};

struct SpectrumArgs {
	float* rows;
	const float* mag;
	const uint32_t* psi;
	size_t stride, frames;
	int N;
};

struct OutputArgs { // out[t] = pv[t], ola[t] or pv[t] + ola[t], t < n_out, for every clip
	const float* rows; // inverse-transformed frames; NULL: no vocoder term
	const float* win;  // N floats
	const float* div;  // D: N / 4 floats
	size_t M;
	int N;
	const float* perc; // NULL: no overlap-add term
	const float* resid; // may be NULL
	const float* win_ola; // Np floats
	const float* div_ola; // d2: Np / 2 floats
	size_t in_stride, n;
	Framing ola;
	float* out;
	size_t out_stride, n_out, n_clips;
};

// the three trigonometric tables of the library's code object on the current device
hipError_t upload_tables(const uint32_t* atan_t, const float* coarse, const float* fine, float c3, float k);

hipError_t launch_frame(const FrameArgs& a, hipStream_t s);
hipError_t launch_analysis(const AnalysisArgs& a, hipStream_t s);
hipError_t launch_peaks(const PeakArgs& a, hipStream_t s);
hipError_t launch_walk(const WalkArgs& a, hipStream_t s);
hipError_t launch_spectrum(const SpectrumArgs& a, hipStream_t s);
hipError_t launch_output(const OutputArgs& a, hipStream_t s);
hipError_t launch_phase(const float* re_im, size_t count, uint32_t* theta, hipStream_t s);
hipError_t launch_cs(const uint32_t* psi, size_t count, float* cos_sin, hipStream_t s);

} // namespace zen_tsm
