// cqt_kernels.h -- launch interface of the kernels of libzen_hip_cqt.so (cqt_kernels.hip).
// A clip of n samples is cut into ns slices of Ls = 2 N samples at hop N.  The slice spectra are rows of Ls complex values,
// packed clip by clip (row c * ns + q), so one batched transform covers a call; the coefficients are rows of M complex values,
// row (c * ns + q) * nb + k for band k of slice q.  V, H and P are matrices of one clip: T = (ns + 1) M / 2 rows of nb floats.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace zen_cqt {

struct Tables { // device copies of the host tables (zen_hip_cqt_table)
	const int* kb;      // N + 1: the lower band of a bin
	const int* centres; // nb
	const float *gL, *gU, *gdL, *gdU; // N + 1 each
	const float *h, *s; // Ls each
};

struct SliceArgs { // step 1: (xp h, 0) of every slice of every clip
	const float* in; // clip c: in + c * in_stride, n samples
	const float* h;
	float* rows; // n_clips * ns rows of Ls complex values
	size_t in_stride, n, ns, n_clips;
	int Ls;
};

struct FoldArgs { // step 2: the half spectrum of every row folded into its nb rows of M values, zeros included
	const float* rows;
	float* coef;
	Tables t;
	size_t n_rows; // n_clips * ns
	int Ls, nb, M;
};

struct OverlapArgs { // step 3, one clip: halves of neighbouring slices added, the magnitude, band-major -> time-major
	const float* coef; // ns * nb rows of M complex values
	float* v;          // T rows of nb floats, v_stride floats apart
	size_t v_stride, ns;
	int nb, M;
};

enum { STEM_HARMONIC = 0, STEM_PERCUSSIVE = 1, STEM_RESIDUAL = 2 };

struct MaskArgs { // steps 5-6, slices q0 .. q0 + run of one clip: the stem's mask from H and P, applied to the coefficients
	const float* coef; // the clip's coefficients
	const float *hm, *pm; // T rows of nb floats
	float* out;        // run * nb rows of M complex values
	size_t q0, run;
	float beta;
	int nb, M, stem, soft;
};

struct GatherArgs { // step 6, slices q0 .. q0 + run of one clip: Y_q from the transformed rows, mirrored half included
	const float* g; // run * nb rows of M complex values
	float* rows;    // the clip's ns rows of Ls complex values
	Tables t;
	size_t q0, run;
	int Ls, nb, M;
};

struct OlaArgs { // step 7: every clip
	const float* rows; // n_clips * ns rows of Ls complex values, inverse-transformed
	const float* s;
	float* out; // clip c: out + c * out_stride
	size_t out_stride, n, ns, n_clips;
	int Ls;
};

hipError_t launch_slice(const SliceArgs& a, hipStream_t s);
hipError_t launch_fold(const FoldArgs& a, hipStream_t s);
hipError_t launch_overlap(const OverlapArgs& a, hipStream_t s);
hipError_t launch_mask(const MaskArgs& a, hipStream_t s);
hipError_t launch_gather(const GatherArgs& a, hipStream_t s);
hipError_t launch_overlap_add(const OlaArgs& a, hipStream_t s);

} // namespace zen_cqt
