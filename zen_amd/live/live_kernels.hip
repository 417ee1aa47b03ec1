// live_kernels.hip -- the three streaming kernels of libzen_hip_live.so (gfx950): feed (the carried partial block and the
// new samples into pass 1's input rows, the new carry, the dry ring), mid (pass 1's P1 + R1 into pass 2's input rows, the
// H1 delay) and out (pass 2's output, the delayed H1 and the delayed input into the caller's rows).
//
// Shape of all three: blockIdx.y walks the streams, the workgroups of a stream walk a destination row as
// ../addon/row_walk.h describes (16-byte stores on the destination's boundaries, a scalar head and tail).  A group that
// straddles a splice point (the end of the carry, the start of the stream's life, the end mapping of finish, the wrap of
// the dry ring) is assembled sample by sample, so nothing outside the source's own samples is ever read.
//
// The only arithmetic is Q = P1 + R1: one IEEE binary32 add, what the engine's `add` destination and the reference's
// sum_vectors_functor (libzen/hps.h:142-150) compute.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "live_kernels.h"

#include "../addon/row_walk.h"

#pragma clang fp contract(off)

namespace zen_live {
namespace {

using namespace zen_addon;

// X[x] of X = carry[0, c) ++ in[0, m) ++ zeros
__device__ __forceinline__ float concat1(const float* __restrict__ carry, size_t c, const float* __restrict__ in, size_t m, size_t x)
{
	if (x < c)
		return carry[x];
	return x - c < m ? in[x - c] : 0.0f;
}

// dst[i] = X[off + i], i < len
__device__ __forceinline__ void copy_concat(float* __restrict__ dst, size_t len, size_t off, const float* __restrict__ carry, size_t c,
                                            const float* __restrict__ in, size_t m, size_t tid, size_t nthreads)
{
	auto one = [=](size_t i) { return concat1(carry, c, in, m, off + i); };
	auto four = [=](size_t i0) {
		const size_t x = off + i0;
		if (x + 4 <= c)
			return load4(carry + x);
		if (x >= c && x - c + 4 <= m)
			return load4(in + (x - c));
		if (x >= c + m)
			return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		return make_float4(concat1(carry, c, in, m, x), concat1(carry, c, in, m, x + 1), concat1(carry, c, in, m, x + 2),
		                   concat1(carry, c, in, m, x + 3));
	};
	walk_row(dst, len, tid, nthreads, one, four);
}

__device__ __forceinline__ void copy_row(float* __restrict__ dst, const float* __restrict__ src, size_t len, size_t tid, size_t nthreads)
{
	walk_row(dst, len, tid, nthreads, [=](size_t j) { return src[j]; }, [=](size_t j0) { return load4(src + j0); });
}

// blockIdx.z picks one of the four destinations, so that each has workgroups of its own: 0 pass 1's input rows, 1 the new
// carry, 2 and 3 the dry ring up to its end and from its start on (at most one wrap: m < dry_len)
__global__ __launch_bounds__(TPB) void feed_kernel(FeedArgs a)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	const size_t first = a.m < a.dry_len - a.dry_pos ? a.m : a.dry_len - a.dry_pos;
	for (size_t s = blockIdx.y; s < a.n_streams; s += gridDim.y) {
		const float* __restrict__ in = a.in + s * a.in_stride; // (never dereferenced where m == 0)
		const float* __restrict__ carry = a.carry_cur + s * a.carry_stride;
		float* __restrict__ ring = a.dry + s * a.dry_stride;
		if (blockIdx.z == 0)
			copy_concat(a.in1 + s * a.in1_stride, a.len1, 0, carry, a.c, in, a.m, tid, nthreads);
		else if (blockIdx.z == 1)
			copy_concat(a.carry_next + s * a.carry_stride, a.c_next, a.len1, carry, a.c, in, a.m, tid, nthreads);
		else if (blockIdx.z == 2)
			copy_row(ring + a.dry_pos, in, first, tid, nthreads);
		else
			copy_row(ring, in + first, a.m - first, tid, nthreads);
	}
}

// one sample / four samples of a row read through the reference's shift, at stream position j
__device__ __forceinline__ float shifted1(const Shifted& q, const float* __restrict__ row, size_t j)
{
	if (j < q.shifted_end)
		return row[(long long)j + q.off_shifted];
	if (j < q.stale_end)
		return row[(long long)j + q.off_stale];
	return 0.0f;
}

// 0: the four samples from j0 on straddle a boundary; 1: *k is the index of the first of four consecutive ones; 2: zeros
__device__ __forceinline__ int shifted4(const Shifted& q, size_t j0, long long* k)
{
	if (j0 + 4 <= q.shifted_end) {
		*k = (long long)j0 + q.off_shifted;
		return 1;
	}
	if (j0 >= q.shifted_end && j0 + 4 <= q.stale_end) {
		*k = (long long)j0 + q.off_stale;
		return 1;
	}
	return j0 >= q.shifted_end && j0 >= q.stale_end ? 2 : 0;
}

__device__ __forceinline__ void copy_shifted(float* __restrict__ dst, size_t cnt, size_t d0, const Shifted q, size_t s, size_t tid,
                                             size_t nthreads)
{
	const float* __restrict__ row = q.row + s * q.stride;
	auto one = [=](size_t i) { return shifted1(q, row, d0 + i); };
	auto four = [=](size_t i0) {
		long long k;
		const int kind = shifted4(q, d0 + i0, &k);
		if (kind == 1)
			return load4(row + k);
		if (kind == 2)
			return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		return make_float4(one(i0), one(i0 + 1), one(i0 + 2), one(i0 + 3));
	};
	walk_row(dst, cnt, tid, nthreads, one, four);
}

__global__ __launch_bounds__(TPB) void mid_kernel(MidArgs a)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	for (size_t s = blockIdx.y; s < a.n_streams; s += gridDim.y) {
		if (a.len2) {
			const Shifted q = a.p;
			const float* __restrict__ p = q.row + s * q.stride;
			const float* __restrict__ r = a.r1 + s * q.stride;
			const size_t t0 = a.t0;
			auto one = [=](size_t j) { return shifted1(q, p, t0 + j) + shifted1(q, r, t0 + j); };
			auto four = [=](size_t j0) {
				long long k;
				const int kind = shifted4(q, t0 + j0, &k);
				if (kind == 1) {
					const float4 x = load4(p + k), y = load4(r + k);
					return make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
				}
				if (kind == 2)
					return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
				return make_float4(one(j0), one(j0 + 1), one(j0 + 2), one(j0 + 3));
			};
			walk_row(a.in2 + s * a.in2_stride, a.len2, tid, nthreads, one, four);
		}
		if (a.hist_len)
			copy_row(a.hist_next + s * a.hist_stride, a.hist_cur + s * a.hist_stride + a.hist_from, a.hist_len, tid, nthreads);
	}
}

__global__ __launch_bounds__(TPB) void out_kernel(OutArgs a)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	for (size_t s = blockIdx.y; s < a.n_streams; s += gridDim.y) {
		if (a.perc_out)
			copy_shifted(a.perc_out + s * a.out_stride, a.cnt, a.d0, a.p2, s, tid, nthreads);
		if (a.harm_out)
			copy_shifted(a.harm_out + s * a.out_stride, a.cnt, a.d0, a.h1, s, tid, nthreads);
		if (a.dry_out) {
			const float* __restrict__ ring = a.dry + s * a.dry_stride;
			const size_t len = a.dry_len, pos = a.dry_pos;
			auto at = [=](size_t i) { // the ring index of sample d0 + i (i < len)
				const size_t x = pos + i;
				return x < len ? x : x - len;
			};
			auto one = [=](size_t i) { return ring[at(i)]; };
			auto four = [=](size_t i0) {
				const size_t x = at(i0);
				if (x + 4 <= len)
					return load4(ring + x);
				return make_float4(one(i0), one(i0 + 1), one(i0 + 2), one(i0 + 3));
			};
			walk_row(a.dry_out + s * a.out_stride, a.cnt, tid, nthreads, one, four);
		}
	}
}

size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

} // namespace

hipError_t launch_feed(const FeedArgs& a, hipStream_t s)
{
	const size_t len = max3(a.len1, a.c_next, a.m);
	if (a.n_streams == 0 || len == 0)
		return hipSuccess;
	dim3 grid = grid_for(len, 4 * a.n_streams); // (the cap counts the four destinations of every stream)
	grid.y = (unsigned)(a.n_streams < 65535 ? a.n_streams : 65535);
	grid.z = 4;
	feed_kernel<<<grid, TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_mid(const MidArgs& a, hipStream_t s)
{
	const size_t len = a.len2 > a.hist_len ? a.len2 : a.hist_len;
	if (a.n_streams == 0 || len == 0)
		return hipSuccess;
	mid_kernel<<<grid_for(len, a.n_streams), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_out(const OutArgs& a, hipStream_t s)
{
	if (a.n_streams == 0 || a.cnt == 0 || (!a.harm_out && !a.perc_out && !a.dry_out))
		return hipSuccess;
	out_kernel<<<grid_for(a.cnt, a.n_streams), TPB, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace zen_live
