// row_walk.h -- the walk over a destination row that the streaming kernels of ragged_kernels.hip and live_kernels.hip share
// (gfx950), and the grid that goes with it.
//
// blockIdx.y walks the rows (clips, streams); the workgroups of a row walk it in a grid-stride loop over groups of 4 floats
// that start on a 16-byte boundary OF THE DESTINATION (global_store_dwordx4), with a scalar head in front of the first
// boundary and a scalar tail behind the last whole group: the caller's pointers and strides only promise 4-byte alignment.
// A group's source is read with one global_load_dwordx4 where its address happens to be 16-byte aligned too, with four
// dword loads otherwise.  What a group reads where it straddles a boundary of its source is the kernel's own business: its
// `four` assembles such a group sample by sample.  No LDS, no atomics.  The grid is capped at 8 workgroups of 256 threads
// per CU (32 wavefronts, the most a CU holds).
//
// Internal linkage throughout: every kernel file compiles its own copy, and none is visible outside its library.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace zen_addon {
namespace {

constexpr int TPB = 256;

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ float4 load4(const float* __restrict__ p)
{
	if (aligned16(p))
		return *reinterpret_cast<const float4*>(p);
	return make_float4(p[0], p[1], p[2], p[3]);
}

// The walk over one destination row of `len` floats: one(j) gives sample j, four(j0) the samples j0 .. j0+3 (all < len).
template <class One, class Four>
__device__ __forceinline__ void walk_row(float* __restrict__ dst, size_t len, size_t tid, size_t nthreads, One one, Four four)
{
	size_t head = ((16 - ((uintptr_t)dst & 15)) & 15) / 4; // floats in front of the first 16-byte boundary of dst
	if (head > len)
		head = len;
	const size_t n_groups = (len - head) / 4, tail = head + n_groups * 4;
	for (size_t j = tid; j < head; j += nthreads)
		dst[j] = one(j);
	for (size_t j = tail + tid; j < len; j += nthreads)
		dst[j] = one(j);
	for (size_t g = tid; g < n_groups; g += nthreads) {
		const size_t j0 = head + g * 4;
		*reinterpret_cast<float4*>(dst + j0) = four(j0);
	}
}

// gx workgroups per row x gy rows: enough to cover a row of `len` floats, at most 8 workgroups per CU over the grid
dim3 grid_for(size_t len, size_t n_rows)
{
	static unsigned cap = 0;
	if (!cap) {
		int dev = 0, cus = 0;
		if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
			cus = 256;
		(void)hipGetLastError();
		cap = 8u * (unsigned)cus;
	}
	const unsigned gy = (unsigned)(n_rows < 65535 ? n_rows : 65535);
	size_t gx = ((len + 3) / 4 + TPB - 1) / TPB;
	const size_t gx_cap = cap / gy > 0 ? cap / gy : 1;
	if (gx > gx_cap)
		gx = gx_cap;
	if (gx < 1)
		gx = 1;
	return dim3((unsigned)gx, gy, 1);
}

} // namespace
} // namespace zen_addon
