// pcm_kernels.hip -- the streaming kernels of libzen_hip_pcm.so (gfx950): int16 -> float (with the stereo mix),
// min / max of an output, float -> int16 (PEAK or GAIN), and the two conversions again for packed 24-bit samples (their
// alignment scheme stands in front of them).  Arithmetic: pcm_convert.h, the same functions the CPU tier tests.
//
// Shape of the first three: a grid-stride loop over groups of 8 samples with 16-byte global accesses on the side that can be
// aligned (global_load_dwordx4 of 8 int16 / global_store_dwordx4 of 8 int16, two dwordx4 on the float side where that side
// happens to be 16-byte aligned as well), a scalar head up to the first 16-byte boundary and a scalar tail behind the last
// whole group: an int16_t* is only 2-byte aligned and the pieces of a pipeline start at arbitrary sample offsets.  The grid is
// capped at 8 workgroups of 256 threads per CU (32 wavefronts, the most a CU holds).  They move 6 bytes
// per sample (peak: 4) and run under host-link copies two orders of magnitude slower than HBM; nothing here is tuned past
// "not visible in the call's wall time".
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pcm_convert.h"
#include "pcm_kernels.h"

#pragma clang fp contract(off)

namespace zen_pcm {
namespace {

constexpr int TPB = 256;

__device__ __forceinline__ int16_t lo16(int w) { return (int16_t)(w & 0xffff); }
__device__ __forceinline__ int16_t hi16(int w) { return (int16_t)(w >> 16); }

template <int CH>
__device__ __forceinline__ float widen_frame(const int16_t* __restrict__ src, size_t i)
{
	if (CH == 1)
		return pcm16_to_float(src[i]);
	return stereo_to_mono(src[2 * i], src[2 * i + 1]);
}

// n frames of CH interleaved int16 -> n floats
template <int CH>
__global__ __launch_bounds__(TPB) void pcm16_to_float_kernel(const int16_t* __restrict__ src, size_t n, float* __restrict__ dst)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	constexpr size_t FRAME_BYTES = 2 * CH;
	const uintptr_t a = (uintptr_t)src;
	// frames in front of the first 16-byte boundary of src; stereo frames that straddle every boundary (src 2 mod 4): all scalar
	size_t head = n;
	if (a % FRAME_BYTES == 0) {
		head = ((16 - (a & 15)) & 15) / FRAME_BYTES;
		if (head > n)
			head = n;
	}
	const size_t n_groups = (n - head) / 8, tail = head + n_groups * 8;
	for (size_t i = tid; i < head; i += nthreads)
		dst[i] = widen_frame<CH>(src, i);
	for (size_t i = tail + tid; i < n; i += nthreads)
		dst[i] = widen_frame<CH>(src, i);
	const bool dst_vec = ((uintptr_t)(dst + head) & 15) == 0;
	for (size_t g = tid; g < n_groups; g += nthreads) {
		const size_t f0 = head + g * 8; // first frame of the group, < n - 7
		const int4* p = reinterpret_cast<const int4*>(src + f0 * CH);
		float o[8];
		if (CH == 1) {
			const int4 v = p[0];
			const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				o[2 * k] = pcm16_to_float(lo16(w[k]));
				o[2 * k + 1] = pcm16_to_float(hi16(w[k]));
			}
		}
		else {
			const int4 v0 = p[0], v1 = p[1];
			const int w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
			for (int k = 0; k < 8; ++k)
				o[k] = stereo_to_mono(lo16(w[k]), hi16(w[k]));
		}
		if (dst_vec) {
			float4* q = reinterpret_cast<float4*>(dst + f0);
			q[0] = make_float4(o[0], o[1], o[2], o[3]);
			q[1] = make_float4(o[4], o[5], o[6], o[7]);
		}
		else {
#pragma unroll
			for (int k = 0; k < 8; ++k)
				dst[f0 + k] = o[k];
		}
	}
}

template <int MODE>
__device__ __forceinline__ int16_t narrow(float y, float scale)
{
	return MODE == ZEN_PCM_MODE_PEAK ? float_to_pcm16_peak(y, scale) : float_to_pcm16_gain(y, scale);
}

// n floats -> n int16; PEAK: scale = max(-minmax[0], minmax[1]) read here, GAIN: scale = gain
template <int MODE>
__global__ __launch_bounds__(TPB) void float_to_pcm16_kernel(const float* __restrict__ src, size_t n, float gain,
                                                             const float* __restrict__ minmax, int16_t* __restrict__ dst)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	const float scale = MODE == ZEN_PCM_MODE_PEAK ? pcm16_peak_of(minmax[0], minmax[1]) : gain;
	size_t head = ((16 - ((uintptr_t)dst & 15)) & 15) / 2; // samples in front of the first 16-byte boundary of dst
	if (head > n)
		head = n;
	const size_t n_groups = (n - head) / 8, tail = head + n_groups * 8;
	for (size_t i = tid; i < head; i += nthreads)
		dst[i] = narrow<MODE>(src[i], scale);
	for (size_t i = tail + tid; i < n; i += nthreads)
		dst[i] = narrow<MODE>(src[i], scale);
	const bool src_vec = ((uintptr_t)(src + head) & 15) == 0;
	for (size_t g = tid; g < n_groups; g += nthreads) {
		const size_t s0 = head + g * 8; // first sample of the group, < n - 7
		float y[8];
		if (src_vec) {
			const float4* p = reinterpret_cast<const float4*>(src + s0);
			const float4 a = p[0], b = p[1];
			y[0] = a.x, y[1] = a.y, y[2] = a.z, y[3] = a.w, y[4] = b.x, y[5] = b.y, y[6] = b.z, y[7] = b.w;
		}
		else {
#pragma unroll
			for (int k = 0; k < 8; ++k)
				y[k] = src[s0 + k];
		}
		int w[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const unsigned lo = (uint16_t)narrow<MODE>(y[2 * k], scale), hi = (uint16_t)narrow<MODE>(y[2 * k + 1], scale);
			w[k] = (int)(lo | (hi << 16));
		}
		*reinterpret_cast<int4*>(dst + s0) = make_int4(w[0], w[1], w[2], w[3]);
	}
}

// ---- packed 24-bit samples ---------------------------------------------------------------------------------------------------
// A 24-bit buffer is only byte-aligned.  3 is coprime to 16, so from any address one of the next 16 samples starts on a
// 16-byte boundary: a byte-wise head of at most 15 samples, then groups of 16 samples = 48 bytes = three 16-byte accesses
// per lane, then a byte-wise tail.  A lane keeps its 48 bytes contiguous (lanes 48 bytes apart; the three accesses of a
// wavefront cover the same 3 KiB of whole cache lines between them), so the re-slicing into samples is shifts of twelve
// registers with constant counts and needs no LDS; the float side of a group is four 16-byte accesses where it is aligned.
// Stereo frames are 6 bytes: an even address reaches a boundary within 7 frames, an odd one never does (every frame
// straddles) and is converted byte-wise throughout -- the pipeline's staging never asks for that.

// sample k (0 .. NW * 4 / 3 - 1) of the little-endian words w: three bytes from byte 3k on, sign-extended
template <int NW>
__device__ __forceinline__ int32_t sample24(const uint32_t (&w)[NW], int k)
{
	const int word = (3 * k) >> 2, sh = ((3 * k) & 3) * 8; // sh <= 8: the sample lies within one word
	uint32_t u = w[word] >> sh;
	if (sh > 8)
		u |= w[word + 1] << (32 - sh); // word + 1 < NW: the last sample of the words has sh == 8
	u &= 0xffffffu;
	return (int32_t)(u ^ 0x800000u) - 0x800000;
}

template <int CH>
__device__ __forceinline__ float widen_frame24(const uint8_t* __restrict__ src, size_t i)
{
	if (CH == 1)
		return pcm24_to_float(pcm24_load(src + 3 * i));
	return pcm24_stereo_to_mono(pcm24_load(src + 6 * i), pcm24_load(src + 6 * i + 3));
}

// n frames of CH interleaved packed 24-bit samples -> n floats
template <int CH>
__global__ __launch_bounds__(TPB) void pcm24_to_float_kernel(const uint8_t* __restrict__ src, size_t n, float* __restrict__ dst)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	const unsigned a = (unsigned)((uintptr_t)src & 15);
	// frames in front of the first frame on a 16-byte boundary: 3 h = -a (mod 16) <=> h = -11 a, as 3 * 11 = 1 (mod 16);
	// stereo: 6 h = -a (mod 16) <=> a even and 3 h = -a / 2 (mod 8) <=> h = -3 a / 2, as 3 * 3 = 1 (mod 8)
	size_t head = n;
	if (CH == 1)
		head = (11u * (16u - a)) & 15u;
	else if (!(a & 1))
		head = (3u * (8u - a / 2)) & 7u;
	if (head > n)
		head = n;
	const size_t n_groups = (n - head) / 16, tail = head + n_groups * 16;
	for (size_t i = tid; i < head; i += nthreads)
		dst[i] = widen_frame24<CH>(src, i);
	for (size_t i = tail + tid; i < n; i += nthreads)
		dst[i] = widen_frame24<CH>(src, i);
	const bool dst_vec = ((uintptr_t)(dst + head) & 15) == 0;
	for (size_t g = tid; g < n_groups; g += nthreads) {
		const size_t f0 = head + g * 16; // first frame of the group, < n - 15
		const uint4* p = reinterpret_cast<const uint4*>(src + f0 * 3 * CH);
		uint32_t w[12 * CH];
#pragma unroll
		for (int k = 0; k < 3 * CH; ++k) {
			const uint4 v = p[k];
			w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
		}
		float o[16];
#pragma unroll
		for (int k = 0; k < 16; ++k)
			o[k] = CH == 1 ? pcm24_to_float(sample24(w, k)) : pcm24_stereo_to_mono(sample24(w, 2 * k), sample24(w, 2 * k + 1));
		if (dst_vec) {
			float4* q = reinterpret_cast<float4*>(dst + f0);
#pragma unroll
			for (int k = 0; k < 4; ++k)
				q[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
		}
		else {
#pragma unroll
			for (int k = 0; k < 16; ++k)
				dst[f0 + k] = o[k];
		}
	}
}

template <int MODE>
__device__ __forceinline__ int32_t narrow24(float y, float scale)
{
	return MODE == ZEN_PCM_MODE_PEAK ? float_to_pcm24_peak(y, scale) : float_to_pcm24_gain(y, scale);
}

// n floats -> n packed 24-bit samples; PEAK: scale = max(-minmax[0], minmax[1]) read here, GAIN: scale = gain.  Head and tail
// are byte stores of their own three bytes: nothing beside the 3 n bytes is read or written (a neighbouring piece may be
// in flight).
template <int MODE>
__global__ __launch_bounds__(TPB) void float_to_pcm24_kernel(const float* __restrict__ src, size_t n, float gain,
                                                             const float* __restrict__ minmax, uint8_t* __restrict__ dst)
{
	const size_t tid = (size_t)blockIdx.x * TPB + threadIdx.x, nthreads = (size_t)gridDim.x * TPB;
	const float scale = MODE == ZEN_PCM_MODE_PEAK ? pcm16_peak_of(minmax[0], minmax[1]) : gain;
	size_t head = (11u * (16u - (unsigned)((uintptr_t)dst & 15))) & 15u; // samples in front of the first one on a 16-byte boundary
	if (head > n)
		head = n;
	const size_t n_groups = (n - head) / 16, tail = head + n_groups * 16;
	for (size_t i = tid; i < head; i += nthreads)
		pcm24_store(dst + 3 * i, narrow24<MODE>(src[i], scale));
	for (size_t i = tail + tid; i < n; i += nthreads)
		pcm24_store(dst + 3 * i, narrow24<MODE>(src[i], scale));
	const bool src_vec = ((uintptr_t)(src + head) & 15) == 0;
	for (size_t g = tid; g < n_groups; g += nthreads) {
		const size_t s0 = head + g * 16; // first sample of the group, < n - 15
		float y[16];
		if (src_vec) {
			const float4* p = reinterpret_cast<const float4*>(src + s0);
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const float4 v = p[k];
				y[4 * k] = v.x, y[4 * k + 1] = v.y, y[4 * k + 2] = v.z, y[4 * k + 3] = v.w;
			}
		}
		else {
#pragma unroll
			for (int k = 0; k < 16; ++k)
				y[k] = src[s0 + k];
		}
		uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
		for (int k = 0; k < 16; ++k) {
			const uint32_t u = (uint32_t)narrow24<MODE>(y[k], scale) & 0xffffffu;
			const int word = (3 * k) >> 2, sh = ((3 * k) & 3) * 8;
			w[word] |= u << sh;
			if (sh > 8)
				w[word + 1] |= u >> (32 - sh);
		}
		uint4* q = reinterpret_cast<uint4*>(dst + s0 * 3);
#pragma unroll
		for (int k = 0; k < 3; ++k)
			q[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
	}
}

// float atomic min / max through the ordered-integer mapping: non-negative floats order like their bit patterns as signed
// integers, negative ones in reverse as unsigned integers, and every negative pattern is above every non-negative one as
// unsigned and below it as signed.
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

// minmax[0] = min(minmax[0], min(src)), minmax[1] = max(minmax[1], max(src)); fminf / fmaxf skip NaNs
__global__ __launch_bounds__(TPB) void peak_kernel(const float* __restrict__ src, size_t n, float* __restrict__ minmax)
{
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
	for (size_t g = tid; g < n_groups; g += nthreads) {
		const float4 v = p[g];
		mn = fminf(fminf(mn, v.x), fminf(fminf(v.y, v.z), v.w));
		mx = fmaxf(fmaxf(mx, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
	}
	// wavefront (64 lanes), then the workgroup's wavefronts through LDS, then one pair of atomics per workgroup
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
		if (mn <= mx) { // (a workgroup that saw nothing but NaNs, or nothing at all, has +inf / -inf: nothing to say)
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

unsigned grid_for(size_t work_items)
{
	static unsigned cap = 0;
	if (!cap) {
		int dev = 0, cus = 0;
		if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
			cus = 256;
		(void)hipGetLastError();
		cap = 8u * (unsigned)cus;
	}
	size_t g = (work_items + TPB - 1) / TPB;
	if (g < 1)
		g = 1;
	return g > cap ? cap : (unsigned)g;
}

} // namespace

hipError_t launch_to_float(const int16_t* src, int channels, size_t n, float* dst, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const unsigned grid = grid_for((n + 7) / 8);
	if (channels == 1)
		pcm16_to_float_kernel<1><<<grid, TPB, 0, s>>>(src, n, dst);
	else
		pcm16_to_float_kernel<2><<<grid, TPB, 0, s>>>(src, n, dst);
	return hipGetLastError();
}

hipError_t launch_from_float(const float* src, size_t n, int mode, float gain, const float* minmax, int16_t* dst, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const unsigned grid = grid_for((n + 7) / 8);
	if (mode == ZEN_PCM_MODE_PEAK)
		float_to_pcm16_kernel<ZEN_PCM_MODE_PEAK><<<grid, TPB, 0, s>>>(src, n, gain, minmax, dst);
	else
		float_to_pcm16_kernel<ZEN_PCM_MODE_GAIN><<<grid, TPB, 0, s>>>(src, n, gain, minmax, dst);
	return hipGetLastError();
}

hipError_t launch_to_float24(const uint8_t* src, int channels, size_t n, float* dst, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const unsigned grid = grid_for((n + 15) / 16);
	if (channels == 1)
		pcm24_to_float_kernel<1><<<grid, TPB, 0, s>>>(src, n, dst);
	else
		pcm24_to_float_kernel<2><<<grid, TPB, 0, s>>>(src, n, dst);
	return hipGetLastError();
}

hipError_t launch_from_float24(const float* src, size_t n, int mode, float gain, const float* minmax, uint8_t* dst, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	const unsigned grid = grid_for((n + 15) / 16);
	if (mode == ZEN_PCM_MODE_PEAK)
		float_to_pcm24_kernel<ZEN_PCM_MODE_PEAK><<<grid, TPB, 0, s>>>(src, n, gain, minmax, dst);
	else
		float_to_pcm24_kernel<ZEN_PCM_MODE_GAIN><<<grid, TPB, 0, s>>>(src, n, gain, minmax, dst);
	return hipGetLastError();
}

hipError_t launch_unpack(int fmt, const void* src, int channels, size_t n, float* dst, hipStream_t s)
{
	return fmt == ZEN_PCM_FMT_I24 ? launch_to_float24(static_cast<const uint8_t*>(src), channels, n, dst, s)
	                              : launch_to_float(static_cast<const int16_t*>(src), channels, n, dst, s);
}

hipError_t launch_pack(int fmt, const float* src, size_t n, int mode, float gain, const float* minmax, void* dst, hipStream_t s)
{
	return fmt == ZEN_PCM_FMT_I24 ? launch_from_float24(src, n, mode, gain, minmax, static_cast<uint8_t*>(dst), s)
	                              : launch_from_float(src, n, mode, gain, minmax, static_cast<int16_t*>(dst), s);
}

hipError_t launch_peak(const float* src, size_t n, float* minmax, hipStream_t s)
{
	if (n == 0)
		return hipSuccess;
	peak_kernel<<<grid_for((n + 3) / 4), TPB, 0, s>>>(src, n, minmax);
	return hipGetLastError();
}

hipError_t launch_minmax_init(float* minmax, int pairs, hipStream_t s)
{
	minmax_init_kernel<<<1, 64, 0, s>>>(minmax, pairs);
	return hipGetLastError();
}

} // namespace zen_pcm
