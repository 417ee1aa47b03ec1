// nmf_kernels.h -- launch interface of the kernels of libzen_hip_nmf.so (nmf_kernels.hip).
// A call works on n_clips clips of n samples, m frames each.  The spectra are packed clip by clip: row c * m + a holds the N
// complex values of frame a of clip c, so one batched transform covers the call.  V holds the magnitudes of the bins 0..H,
// one row of v_stride floats (a multiple of 4: 16-byte loads) per frame, packed alike.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../addon/stft_args.h"

namespace zen_nmf {

enum { MAX_COMPONENTS = 256, MAX_FRAMES = 16384, SEGMENT = 256 };
enum { TILE = 128 }; // rows and columns of a product per workgroup
enum Product { RATIO = 0, UPDATE_H = 1, UPDATE_W = 2 };

using zen_addon::FrameArgs; // ../addon/stft_args.h, with the layout of a call's rows
using zen_addon::MagArgs;

// out[i][j] = epilogue(sdot over l < L of (A(i, l), B(l, j))), i < I, j < J.  An operand is reduction-minor (A(i, l) =
// a[i * a_stride + l]) or reduction-major (A(i, l) = a[l * a_stride + i]) as its product has it:
//   RATIO     A = H (major), B = W (major); I = m, J = F, L = K <= 256; out = e[i][j] / max(sum, eps) with e = V; `lam`
//             receives the sums where it is not null
//   UPDATE_H  A = W (minor), B = Q (minor); I = K, J = m, L = F; out = (e[i][j] * sum) / max(rowsum(A)[i], eps) with e = H
//   UPDATE_W  A = H (minor), B = Q (major); I = K - fixed (the launcher's caller shifts a, e and out), J = F, L = m; e = W
// out may be e.
//
// The two updates may be split by segments over workgroups (launch_product_split): workgroup z of a tile then carries
// segment z alone and leaves its raw sums in part[(z * I + i) * J + j] and its share of the row sums in part_rs[z * I + i];
// a second kernel adds the segments in rising order and applies the epilogue.  The bits are those of the kernel that walks the
// segments in sequence.
struct ProductArgs {
	const float* a;
	const float* b;
	const float* e;
	float* out;
	float* lam;
	size_t a_stride, b_stride, e_stride, out_stride, lam_stride, I, J, L;
	float* part;    // split only: ceil(L / SEGMENT) * I * J floats
	float* part_rs; // split only: ceil(L / SEGMENT) * I floats
};

struct StemArgs { // one clip, one group: y = x through the mask L_g / L
	const float* x; // m rows of N complex values
	float* y;
	const float* w; // K rows, w_stride apart
	const float* h; // K rows, h_stride apart
	size_t w_stride, h_stride, m;
	int N, K;
	unsigned member[MAX_COMPONENTS / 32]; // bit k: component k is of the group
};

struct OlaArgs { // one clip
	const float* rows; // inverse-transformed frames
	const float* div;  // H floats
	float* out;
	size_t n;
	int N;
};

// the first two are ../addon/stft_kernels.h's as this library compiled them; hidden: their names spell a type of zen_addon,
// and nothing of zen_amd/addon is among a library's dynamic symbols
__attribute__((visibility("hidden"))) hipError_t launch_frame(const FrameArgs& a, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_magnitude(const MagArgs& a, hipStream_t s);
hipError_t launch_product(Product which, const ProductArgs& a, bool mfma, hipStream_t s); // the segments in sequence
hipError_t launch_product_split(Product which, const ProductArgs& a, bool mfma, hipStream_t s); // UPDATE_H / UPDATE_W: partial sums, then combine
hipError_t launch_stem_mask(const StemArgs& a, hipStream_t s);
hipError_t launch_overlap_add(const OlaArgs& a, hipStream_t s);

} // namespace zen_nmf
