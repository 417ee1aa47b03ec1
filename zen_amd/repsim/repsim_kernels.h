// repsim_kernels.h -- launch interface of the kernels of libzen_hip_repsim.so (repsim_kernels.hip).
// A call works on n_clips clips of n samples, m frames each.  The spectra are packed clip by clip: row c * m + a holds the N
// complex values of frame a of clip c, so one batched transform covers the call.  V holds the magnitudes of the bins 0..H,
// one row of v_stride floats (a multiple of 4: 16-byte loads) per frame, packed alike.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../addon/stft_args.h"

namespace zen_repsim {

enum { MAX_NEIGHBOURS = 256, REGISTER_NEIGHBOURS = 32, MAX_FRAMES = 16384 }; // counts up to REGISTER_NEIGHBOURS are sorted in registers
enum { SIM_TILE = 128 }; // similarity: rows and columns of S per workgroup

using zen_addon::FrameArgs; // ../addon/stft_args.h, with the layout of a call's rows
using zen_addon::MagArgs;

struct SimArgs { // S[a][b] for the ma rows of va against the mb rows of vb (both rows of `bins` floats, v_stride apart)
	const float* va;
	const float* vb;
	float* s; // ma rows of mb floats, s_stride apart
	size_t v_stride, s_stride, ma, mb, bins;
};

struct SelectArgs { // `rows` rows of S, each of m candidates -> idx (rows of k), counts
	const float* s;
	int* idx;
	int* counts;
	size_t s_stride, rows, m;
	float t;
	int dd, k; // 1 <= dd <= m, 1 <= k <= MAX_NEIGHBOURS
};

struct GatherArgs { // U[a][f] = the median of V[idx[a][q]][f], q < counts[a]
	const float* v; // m rows
	const int* idx; // `rows` rows of k
	const int* counts;
	float* u; // `rows` rows of u_stride floats
	size_t v_stride, u_stride, m, rows, bins;
	int k;
};

struct MaskArgs { // one clip, in place on its spectra
	float* rows;
	const float* v;
	const float* u; // m rows of v_stride floats
	size_t v_stride, m;
	int N, kc;
};

struct OlaArgs { // one clip
	const float* rows; // inverse-transformed frames
	const float* in;
	const float* div; // H floats
	float *background, *foreground; // either may be NULL
	size_t n;
	int N;
};

// the first two are ../addon/stft_kernels.h's as this library compiled them; hidden: their names spell a type of zen_addon,
// and nothing of zen_amd/addon is among a library's dynamic symbols
__attribute__((visibility("hidden"))) hipError_t launch_frame(const FrameArgs& a, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_magnitude(const MagArgs& a, hipStream_t s);
hipError_t launch_similarity(const SimArgs& a, bool mfma, hipStream_t s);
hipError_t launch_select(const SelectArgs& a, hipStream_t s);
hipError_t launch_gather_median(const GatherArgs& a, hipStream_t s);
hipError_t launch_mask(const MaskArgs& a, hipStream_t s);
hipError_t launch_overlap_add(const OlaArgs& a, hipStream_t s);

} // namespace zen_repsim
