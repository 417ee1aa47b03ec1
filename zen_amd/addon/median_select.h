// median_select.h -- the median of up to 32 values per bin in registers, shared by the kernel sources of zen_amd/repet (over
// the frames one period apart) and zen_amd/repsim (over the frames a selection names): a bitonic network on a power of two
// of values padded with +inf, the pick of the middle one or two, and the body of a kernel around them.
//
// Header-only with internal linkage, as stft_kernels.h is.  A median is a selection: it is exact however it is found.
// Nothing here names the device beyond the words a stand-in header defines away, so it compiles as plain C++ as well
// (tests/cpp/test_addon_median_host.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stddef.h>

namespace zen_addon {
namespace {

__device__ __forceinline__ void cswap(float& a, float& b) // a permutation of (a, b) for every pair of non-NaN values
{
	const bool gt = a > b;
	const float lo = gt ? b : a, hi = gt ? a : b;
	a = lo;
	b = hi;
}

template <int P>
__device__ __forceinline__ void sort_network(float (&a)[P]) // the bitonic network on P values, ascending
{
#pragma unroll
	for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
		for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
			for (int i = 0; i < P; ++i) {
				const int l = i ^ j;
				if (l > i) {
					if ((i & k) == 0)
						cswap(a[i], a[l]);
					else
						cswap(a[l], a[i]);
				}
			}
		}
	}
}

template <int P>
__device__ __forceinline__ float pick_median(const float (&a)[P], int c) // c values sorted in front of P - c times +inf
{
	const int lo = (c - 1) >> 1, hi = c >> 1;
	float slo = a[0], shi = a[0];
#pragma unroll
	for (int i = 1; i < P; ++i) { // every index is a constant: the values stay in registers
		slo = i == lo ? a[i] : slo;
		shi = i == hi ? a[i] : shi;
	}
	return (c & 1) ? slo : (slo + shi) * 0.5f;
}

// The medians of the VEC adjacent bins f.. of a lane over up to P rows, into out[0..VEC).  The caller's RowOf states the rows:
// rows.present(q) whether there is a row q (at least one of q < P), rows.row(q) its bin 0.  row is asked for every q < P:
// what it answers for a row that is not present is never read through.  Every sweep q is a coalesced row read (16 bytes per
// lane for VEC = 4) and the VEC networks are independent of each other.  VEC = 4 wants the rows and out - f 16-byte aligned
// and their strides multiples of 4; the lanes at the end of a row fall back to single words.
template <int P, int VEC, class RowOf>
__device__ __forceinline__ void median_in_registers(const RowOf& rows, size_t f, size_t bins, float* __restrict__ out)
{
	float a[VEC][P];
	int c = 0;
	const bool whole = VEC == 1 || f + VEC <= bins;
#pragma unroll
	for (int q = 0; q < P; ++q) {
		const bool in = rows.present(q);
		c += in ? 1 : 0;
		const float* __restrict__ src = rows.row(q) + f;
		if (VEC == 4 && whole) {
			float4 x = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
			if (in)
				x = *reinterpret_cast<const float4*>(src);
			a[0][q] = x.x;
			a[1 % VEC][q] = x.y;
			a[2 % VEC][q] = x.z;
			a[3 % VEC][q] = x.w;
		} else {
#pragma unroll
			for (int e = 0; e < VEC; ++e)
				a[e][q] = in && f + e < bins ? src[e] : INFINITY;
		}
	}
	float r[VEC];
#pragma unroll
	for (int e = 0; e < VEC; ++e) {
		sort_network<P>(a[e]);
		r[e] = pick_median<P>(a[e], c);
	}
	if (VEC == 4 && whole) {
		*reinterpret_cast<float4*>(out) = make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
	} else {
#pragma unroll
		for (int e = 0; e < VEC; ++e)
			if (f + e < bins)
				out[e] = r[e];
	}
}

} // namespace
} // namespace zen_addon
