// multi_kernels.hip -- the three kernels of libzen_hip_multi.so (gfx950): split (interleaved frames -> planar float rows),
// join (planar rows -> interleaved frames, narrowed in PEAK or GAIN mode where the format is int16) and peak (accumulating
// min / max over the rows of one stem).  Sample arithmetic: ../pcm/pcm_convert.h, the functions the CPU tier tests.
//
// split and join are transposes of a [n_frames, C] matrix whose one side is C elements wide: memory-bound, 6 bytes per
// sample for int16 and 8 for float.  One shape for every C in 1..8, both formats and both directions:
//
//   A workgroup of 256 threads walks tiles of tf = (2048 / C) & ~3 frames, i.e. at most TILE = 2048 samples, through LDS.
//   The interleaved side of a tile is ONE contiguous run of nf * C samples and each planar side is C contiguous runs of nf
//   floats.  Every run is cut at its own 16-byte boundaries: whole 16-byte groups move with one dwordx4 access per lane,
//   consecutive lanes on consecutive groups; the elements in front of the first boundary and behind the last whole group
//   (at most 7 + 7 int16 or 3 + 3 floats per run) move one by one.  Nothing but the element size is assumed of a pointer
//   or of row_stride; a run whose address is 16-byte aligned has no scalar part at all.
//
//   LDS holds the tile in interleaved order as 32-bit words (float bits; int16 is widened before it goes in and narrowed
//   after it comes out), word e at e + e / 32.  Both phases use 4-byte LDS accesses, banked (address / 4) mod 32 over the
//   two 32-lane halves of a wavefront.  The interleaved side has lane l on words s + 4 l + k (float) or s + 8 l + k (int16),
//   the planar side on words (h + 4 l + j) C + c: without the pad word these are 8-way conflicts on the interleaved side and
//   up to 32-way (C = 8) on the planar side; with it every access of either phase is at most 2-way (3-way for C = 3 and 7
//   where a half straddles two channels), counted over every C, head and lane group by the arithmetic above.
//
//   Indices of samples in memory are size_t throughout (n_frames * C may pass 2^32); indices within a tile are ints < 2112.
//
// peak is the min / max kernel of the PCM library over C rows that are row_stride apart: 16-byte loads behind a scalar
// head per row, wavefront shuffle, LDS, one pair of integer atomics per workgroup.  min and max are exact and commute, so
// the result has the same bits in any order.  The grid of all three is capped at 8 workgroups per CU.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../pcm/pcm_convert.h"
#include "multi_kernels.h"
#include "zen_hip_multi.h"

#pragma clang fp contract(off)

namespace zen_multi {
namespace {

constexpr int TPB = 256;

__device__ __forceinline__ int lds_at(int e) { return e + (e >> 5); }

template <int FMT>
struct Sample;
template <>
struct Sample<ZEN_HIP_MULTI_I16> {
	typedef int16_t type;
};
template <>
struct Sample<ZEN_HIP_MULTI_F32> {
	typedef uint32_t type; // the bits: a copy keeps NaN payloads
};

// a run of `len` elements of `bytes` bytes at address a: [0, head) scalar, nvec groups of 16 bytes, [tail0, len) scalar
struct Run {
	int head, nvec, tail0, nscal;
	__device__ __forceinline__ Run(uintptr_t a, int len, int bytes)
	{
		const int per = 16 / bytes;
		head = (int)(((16 - (a & 15)) & 15) / bytes);
		if (head > len)
			head = len;
		nvec = (len - head) / per;
		tail0 = head + nvec * per;
		nscal = head + (len - tail0);
	}
	__device__ __forceinline__ int scalar(int i) const { return i < head ? i : tail0 + (i - head); } // i < nscal
};

__device__ __forceinline__ uint32_t widen(int16_t s) { return __float_as_uint(pcm16_to_float(s)); }
__device__ __forceinline__ uint32_t widen(uint32_t s) { return s; }

// the tile's frames: tf per tile, tile t holds frames [t tf, t tf + nf)
__device__ __forceinline__ int tile_frames(int C) { return (TILE / C) & ~3; }

template <int FMT>
__global__ __launch_bounds__(TPB) void split_kernel(const typename Sample<FMT>::type* __restrict__ src, int C, size_t n,
                                                    uint32_t* __restrict__ rows, size_t stride)
{
	typedef typename Sample<FMT>::type S;
	constexpr int PER = 16 / (int)sizeof(S);
	__shared__ uint32_t tile[TILE_WORDS];
	const int tf = tile_frames(C), nvmax = tf / 4;
	const size_t n_tiles = (n + (size_t)tf - 1) / (size_t)tf;
	for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const size_t f0 = t * (size_t)tf;
		const int nf = n - f0 < (size_t)tf ? (int)(n - f0) : tf, len = nf * C;
		// interleaved run -> LDS
		const S* p = src + f0 * (size_t)C;
		const Run in((uintptr_t)p, len, (int)sizeof(S));
		for (int i = threadIdx.x; i < in.nscal; i += TPB) {
			const int e = in.scalar(i);
			tile[lds_at(e)] = widen(p[e]);
		}
		for (int v = threadIdx.x; v < in.nvec; v += TPB) {
			const int e = in.head + v * PER; // e + PER <= len
			const int4 q = *reinterpret_cast<const int4*>(p + e);
			const int w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				if (FMT == ZEN_HIP_MULTI_I16) {
					tile[lds_at(e + 2 * k)] = widen((int16_t)(w[k] & 0xffff));
					tile[lds_at(e + 2 * k + 1)] = widen((int16_t)(w[k] >> 16));
				} else {
					tile[lds_at(e + k)] = (uint32_t)w[k];
				}
			}
		}
		__syncthreads();
		// LDS -> the C planar runs: item (c, v) = group v of row c, item (c, i) = scalar i of row c
		for (int it = threadIdx.x; it < C * nvmax; it += TPB) {
			const int c = it / nvmax, v = it - c * nvmax;
			uint32_t* r = rows + (size_t)c * stride + f0;
			const Run out((uintptr_t)r, nf, 4);
			if (v < out.nvec) {
				const int f = out.head + 4 * v; // f + 4 <= nf
				int4 q;
				q.x = (int)tile[lds_at(f * C + c)];
				q.y = (int)tile[lds_at((f + 1) * C + c)];
				q.z = (int)tile[lds_at((f + 2) * C + c)];
				q.w = (int)tile[lds_at((f + 3) * C + c)];
				*reinterpret_cast<int4*>(r + f) = q;
			}
		}
		for (int it = threadIdx.x; it < 8 * C; it += TPB) {
			const int c = it >> 3, i = it & 7;
			uint32_t* r = rows + (size_t)c * stride + f0;
			const Run out((uintptr_t)r, nf, 4);
			if (i < out.nscal) {
				const int f = out.scalar(i);
				r[f] = tile[lds_at(f * C + c)];
			}
		}
		__syncthreads(); // the next tile overwrites the words
	}
}

template <int FMT, int MODE>
__device__ __forceinline__ typename Sample<FMT>::type narrow(uint32_t w, float scale)
{
	if (FMT == ZEN_HIP_MULTI_F32)
		return (typename Sample<FMT>::type)w;
	const float y = __uint_as_float(w);
	return (typename Sample<FMT>::type)(MODE == ZEN_HIP_MULTI_PEAK ? float_to_pcm16_peak(y, scale) : float_to_pcm16_gain(y, scale));
}

// PEAK: scale = max(-minmax[0], minmax[1]), read here; GAIN: scale = gain; float: neither
template <int FMT, int MODE>
__global__ __launch_bounds__(TPB) void join_kernel(const uint32_t* __restrict__ rows, int C, size_t n, size_t stride, float gain,
                                                   const float* __restrict__ minmax, typename Sample<FMT>::type* __restrict__ dst)
{
	typedef typename Sample<FMT>::type S;
	constexpr int PER = 16 / (int)sizeof(S);
	__shared__ uint32_t tile[TILE_WORDS];
	float scale = gain;
	if (FMT == ZEN_HIP_MULTI_I16 && MODE == ZEN_HIP_MULTI_PEAK)
		scale = pcm16_peak_of(minmax[0], minmax[1]);
	const int tf = tile_frames(C), nvmax = tf / 4;
	const size_t n_tiles = (n + (size_t)tf - 1) / (size_t)tf;
	for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const size_t f0 = t * (size_t)tf;
		const int nf = n - f0 < (size_t)tf ? (int)(n - f0) : tf, len = nf * C;
		// the C planar runs -> LDS
		for (int it = threadIdx.x; it < C * nvmax; it += TPB) {
			const int c = it / nvmax, v = it - c * nvmax;
			const uint32_t* r = rows + (size_t)c * stride + f0;
			const Run in((uintptr_t)r, nf, 4);
			if (v < in.nvec) {
				const int f = in.head + 4 * v; // f + 4 <= nf
				const int4 q = *reinterpret_cast<const int4*>(r + f);
				tile[lds_at(f * C + c)] = (uint32_t)q.x;
				tile[lds_at((f + 1) * C + c)] = (uint32_t)q.y;
				tile[lds_at((f + 2) * C + c)] = (uint32_t)q.z;
				tile[lds_at((f + 3) * C + c)] = (uint32_t)q.w;
			}
		}
		for (int it = threadIdx.x; it < 8 * C; it += TPB) {
			const int c = it >> 3, i = it & 7;
			const uint32_t* r = rows + (size_t)c * stride + f0;
			const Run in((uintptr_t)r, nf, 4);
			if (i < in.nscal) {
				const int f = in.scalar(i);
				tile[lds_at(f * C + c)] = r[f];
			}
		}
		__syncthreads();
		// LDS -> interleaved run
		S* p = dst + f0 * (size_t)C;
		const Run out((uintptr_t)p, len, (int)sizeof(S));
		for (int i = threadIdx.x; i < out.nscal; i += TPB) {
			const int e = out.scalar(i);
			p[e] = narrow<FMT, MODE>(tile[lds_at(e)], scale);
		}
		for (int v = threadIdx.x; v < out.nvec; v += TPB) {
			const int e = out.head + v * PER; // e + PER <= len
			int w[4];
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				if (FMT == ZEN_HIP_MULTI_I16) {
					const unsigned lo = (uint16_t)narrow<FMT, MODE>(tile[lds_at(e + 2 * k)], scale);
					const unsigned hi = (uint16_t)narrow<FMT, MODE>(tile[lds_at(e + 2 * k + 1)], scale);
					w[k] = (int)(lo | (hi << 16));
				} else {
					w[k] = (int)tile[lds_at(e + k)];
				}
			}
			*reinterpret_cast<int4*>(p + e) = make_int4(w[0], w[1], w[2], w[3]);
		}
		__syncthreads();
	}
}

// float atomic min / max through the ordered-integer mapping: non-negative floats order like their bit patterns as signed
// integers, negative ones in reverse as unsigned integers.
__device__ __forceinline__ void atomic_min_float(float* addr, float v)
{
	if (!(__float_as_uint(v) >> 31))
		atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
	else
		atomicMax(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_float(float* addr, float v)
{
	if (!(__float_as_uint(v) >> 31))
		atomicMax(reinterpret_cast<int*>(addr), __float_as_int(v));
	else
		atomicMin(reinterpret_cast<unsigned*>(addr), __float_as_uint(v));
}

// minmax[0] = min(minmax[0], min over the C rows), minmax[1] likewise; fminf / fmaxf skip NaNs.  blockIdx.y: the row.
__global__ __launch_bounds__(TPB) void peak_kernel(const float* __restrict__ rows, size_t n, size_t stride, float* __restrict__ minmax)
{
	const float* src = rows + (size_t)blockIdx.y * stride;
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	float mn = INFINITY, mx = -INFINITY;
	size_t head = ((16 - ((uintptr_t)src & 15)) & 15) / 4;
	if (head > n)
		head = n;
	const size_t n_groups = (n - head) / 4, tail = head + n_groups * 4;
	for (size_t i = tid; i < head; i += nthreads) {
		mn = fminf(mn, src[i]);
		mx = fmaxf(mx, src[i]);
	}
	for (size_t i = tail + tid; i < n; i += nthreads) {
		mn = fminf(mn, src[i]);
		mx = fmaxf(mx, src[i]);
	}
	const float4* p = reinterpret_cast<const float4*>(src + head);
	size_t g = tid;
	for (; g + 3 * nthreads < n_groups; g += 4 * nthreads) { // four loads in flight per lane
		const float4 a = p[g], b = p[g + nthreads], c = p[g + 2 * nthreads], d = p[g + 3 * nthreads];
		const float lo = fminf(fminf(fminf(a.x, a.y), fminf(a.z, a.w)), fminf(fminf(b.x, b.y), fminf(b.z, b.w)));
		const float lo2 = fminf(fminf(fminf(c.x, c.y), fminf(c.z, c.w)), fminf(fminf(d.x, d.y), fminf(d.z, d.w)));
		const float hi = fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
		const float hi2 = fmaxf(fmaxf(fmaxf(c.x, c.y), fmaxf(c.z, c.w)), fmaxf(fmaxf(d.x, d.y), fmaxf(d.z, d.w)));
		mn = fminf(mn, fminf(lo, lo2));
		mx = fmaxf(mx, fmaxf(hi, hi2));
	}
	for (; g < n_groups; g += nthreads) {
		const float4 v = p[g];
		mn = fminf(fminf(mn, v.x), fminf(fminf(v.y, v.z), v.w));
		mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
	}
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) {
		mn = fminf(mn, __shfl_xor(mn, off, 64));
		mx = fmaxf(mx, __shfl_xor(mx, off, 64));
	}
	__shared__ float s_mn[TPB / 64], s_mx[TPB / 64];
	if ((threadIdx.x & 63) == 0) {
		s_mn[threadIdx.x >> 6] = mn;
		s_mx[threadIdx.x >> 6] = mx;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
#pragma unroll
		for (int w = 1; w < TPB / 64; ++w) {
			mn = fminf(mn, s_mn[w]);
			mx = fmaxf(mx, s_mx[w]);
		}
		if (mn <= mx) { // (a workgroup that saw nothing but NaNs has +inf / -inf: nothing to say)
			atomic_min_float(minmax, mn);
			atomic_max_float(minmax + 1, mx);
		}
	}
}

__global__ void minmax_init_kernel(float* minmax, int pairs)
{
	const int i = threadIdx.x;
	if (i < pairs) {
		minmax[2 * i] = INFINITY;
		minmax[2 * i + 1] = -INFINITY;
	}
}

__global__ void peaks_of_kernel(const float* minmax, int pairs, unsigned active, float* peaks)
{
	const int i = threadIdx.x;
	if (i < pairs) {
		const float mn = minmax[2 * i], mx = minmax[2 * i + 1];
		peaks[i] = ((active >> i) & 1u) && mn <= mx ? pcm16_peak_of(mn, mx) : 0.0f;
	}
}

// 8 workgroups per CU of the device that is current now (asked at every launch: a process may switch devices, and two host
// calls cost nothing beside a launch).  Where the question fails the launch that follows reports the error; 256 CUs until then.
unsigned grid_cap()
{
	int dev = 0, cus = 0;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
		(void)hipGetLastError(); // (not sticky: the launch's own hipGetLastError must speak of the launch)
		cus = 256;
	}
	return 8u * (unsigned)cus;
}

unsigned grid_for(size_t work_groups)
{
	const unsigned cap = grid_cap();
	if (work_groups < 1)
		work_groups = 1;
	return work_groups > cap ? cap : (unsigned)work_groups;
}

size_t tiles_of(size_t n, int C)
{
	const size_t tf = (size_t)((TILE / C) & ~3);
	return (n + tf - 1) / tf;
}

} // namespace

hipError_t launch_split(int fmt, const void* src, int C, size_t n, float* rows, size_t stride, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const unsigned grid = grid_for(tiles_of(n, C));
	if (fmt == ZEN_HIP_MULTI_I16)
		split_kernel<ZEN_HIP_MULTI_I16><<<grid, TPB, 0, s>>>((const int16_t*)src, C, n, (uint32_t*)rows, stride);
	else
		split_kernel<ZEN_HIP_MULTI_F32><<<grid, TPB, 0, s>>>((const uint32_t*)src, C, n, (uint32_t*)rows, stride);
	return hipGetLastError();
}

hipError_t launch_join(int fmt, const float* rows, int C, size_t n, size_t stride, int mode, float gain, const float* minmax, void* dst,
                       hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const unsigned grid = grid_for(tiles_of(n, C));
	const uint32_t* r = (const uint32_t*)rows;
	if (fmt == ZEN_HIP_MULTI_F32)
		join_kernel<ZEN_HIP_MULTI_F32, ZEN_HIP_MULTI_GAIN><<<grid, TPB, 0, s>>>(r, C, n, stride, gain, minmax, (uint32_t*)dst);
	else if (mode == ZEN_HIP_MULTI_PEAK)
		join_kernel<ZEN_HIP_MULTI_I16, ZEN_HIP_MULTI_PEAK><<<grid, TPB, 0, s>>>(r, C, n, stride, gain, minmax, (int16_t*)dst);
	else
		join_kernel<ZEN_HIP_MULTI_I16, ZEN_HIP_MULTI_GAIN><<<grid, TPB, 0, s>>>(r, C, n, stride, gain, minmax, (int16_t*)dst);
	return hipGetLastError();
}

hipError_t launch_peak(const float* rows, int C, size_t n, size_t stride, float* minmax, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const unsigned per_row = grid_for(((n + 3) / 4 + TPB - 1) / TPB) / (unsigned)C;
	peak_kernel<<<dim3(per_row ? per_row : 1, (unsigned)C), TPB, 0, s>>>(rows, n, stride, minmax);
	return hipGetLastError();
}

hipError_t launch_minmax_init(float* minmax, int pairs, hipStream_t s)
{
	minmax_init_kernel<<<1, 64, 0, s>>>(minmax, pairs);
	return hipGetLastError();
}

hipError_t launch_peaks_of(const float* minmax, int pairs, unsigned active, float* peaks, hipStream_t s)
{
	peaks_of_kernel<<<1, 64, 0, s>>>(minmax, pairs, active, peaks);
	return hipGetLastError();
}

} // namespace zen_multi
