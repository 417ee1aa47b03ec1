// ragged_kernels.hip -- the three streaming kernels of libzen_hip_ragged.so (gfx950): pack (the caller's ragged rows into
// zero-padded rows), splice (pass 1's outputs into pass 2's input rows and the harmonic result rows) and trim (pass 2's
// output into the percussive result rows).
//
// Shape of all three: blockIdx.y walks the clips, the workgroups of a clip walk its destination row as ../addon/row_walk.h
// describes (16-byte stores on the destination's boundaries, a scalar head and tail).  A group's source is 16-byte aligned
// between the buffers of this library: their rows are multiples of the hop and so are the shifts.  A group that straddles
// one of the row's boundaries (the clip's end, the splice points) is assembled sample by sample, so nothing beyond a clip's
// own samples is ever read.
//
// The only arithmetic is Q = P1 + R1: one IEEE binary32 add, what the engine's `add` destination and the reference's
// sum_vectors_functor (libzen/hps.h:142-150) compute.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ragged_kernels.h"

#include "../addon/row_walk.h"

#pragma clang fp contract(off)

namespace zen_ragged {
namespace {

using namespace zen_addon;

// dst[j] = j < n ? src[j] : 0 for j < len (n <= len); src[n] and beyond is not read
__device__ __forceinline__ void copy_zero_tail(float* __restrict__ dst, const float* __restrict__ src, size_t n, size_t len,
                                               size_t tid, size_t nthreads)
{
	auto one = [=](size_t j) { return j < n ? src[j] : 0.0f; };
	auto four = [=](size_t j0) {
		if (j0 + 4 <= n)
			return load4(src + j0);
		if (j0 >= n)
			return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		return make_float4(one(j0), one(j0 + 1), one(j0 + 2), one(j0 + 3));
	};
	walk_row(dst, len, tid, nthreads, one, four);
}

__global__ __launch_bounds__(TPB) void pack_kernel(const float* __restrict__ audio, size_t stride, const tab_t* __restrict__ tab,
                                                   size_t n_clips, float* __restrict__ staged, size_t row)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	for (size_t c = blockIdx.y; c < n_clips; c += gridDim.y)
		copy_zero_tail(staged + c * row, audio + c * stride, (size_t)tab[c], row, tid, nthreads);
}

__global__ __launch_bounds__(TPB) void trim_kernel(const float* __restrict__ p2, size_t row2, size_t sh2, const tab_t* __restrict__ tab,
                                                   size_t n_clips, float* __restrict__ perc, size_t out_stride, size_t max_len)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	for (size_t c = blockIdx.y; c < n_clips; c += gridDim.y)
		copy_zero_tail(perc + c * out_stride, p2 + c * row2 + sh2, (size_t)tab[c], max_len, tid, nthreads);
}

__global__ __launch_bounds__(TPB) void splice_kernel(const float* __restrict__ h1, const float* __restrict__ p1,
                                                     const float* __restrict__ r1, size_t row1, size_t sh1,
                                                     const tab_t* __restrict__ tab, size_t n_clips, float* __restrict__ in2,
                                                     size_t row2, float* __restrict__ harm, size_t out_stride, size_t max_len)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	for (size_t c = blockIdx.y; c < n_clips; c += gridDim.y) {
		const size_t n = (size_t)tab[c], padded1 = (size_t)tab[n_clips + c];
		if (in2) {
			const float* __restrict__ p = p1 + c * row1;
			const float* __restrict__ r = r1 + c * row1;
			const size_t a = padded1 > sh1 ? padded1 - sh1 : 0; // [0, a): shifted; [a, padded1): what the in-place shift left behind
			auto one = [=](size_t j) {
				if (j >= padded1)
					return 0.0f;
				const size_t k = j < a ? j + sh1 : j;
				return p[k] + r[k];
			};
			auto four = [=](size_t j0) {
				if (j0 >= padded1)
					return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
				size_t k;
				if (j0 + 4 <= a)
					k = j0 + sh1;
				else if (j0 >= a && j0 + 4 <= padded1)
					k = j0;
				else
					return make_float4(one(j0), one(j0 + 1), one(j0 + 2), one(j0 + 3));
				const float4 x = load4(p + k), y = load4(r + k);
				return make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
			};
			walk_row(in2 + c * row2, row2, tid, nthreads, one, four);
		}
		if (harm)
			copy_zero_tail(harm + c * out_stride, h1 + c * row1 + sh1, n, max_len, tid, nthreads);
	}
}

} // namespace

hipError_t launch_pack(const float* audio, size_t stride, const tab_t* tab, size_t n_clips, float* staged, size_t row, hipStream_t s)
{
	if (n_clips == 0 || row == 0)
		return hipSuccess;
	pack_kernel<<<grid_for(row, n_clips), TPB, 0, s>>>(audio, stride, tab, n_clips, staged, row);
	return hipGetLastError();
}

hipError_t launch_splice(const float* h1, const float* p1, const float* r1, size_t row1, size_t sh1, const tab_t* tab,
                         size_t n_clips, float* in2, size_t row2, float* harm, size_t out_stride, size_t max_len, hipStream_t s)
{
	const size_t len = (in2 && row2 > max_len) || !harm ? row2 : max_len;
	if (n_clips == 0 || (!in2 && !harm) || len == 0)
		return hipSuccess;
	splice_kernel<<<grid_for(len, n_clips), TPB, 0, s>>>(h1, p1, r1, row1, sh1, tab, n_clips, in2, row2, harm, out_stride, max_len);
	return hipGetLastError();
}

hipError_t launch_trim(const float* p2, size_t row2, size_t sh2, const tab_t* tab, size_t n_clips, float* perc, size_t out_stride,
                       size_t max_len, hipStream_t s)
{
	if (n_clips == 0 || max_len == 0)
		return hipSuccess;
	trim_kernel<<<grid_for(max_len, n_clips), TPB, 0, s>>>(p2, row2, sh2, tab, n_clips, perc, out_stride, max_len);
	return hipGetLastError();
}

} // namespace zen_ragged
