// pitch_kernels.hip -- the three kernels of libzen_hip_pitch.so (gfx950) around the two public FFT calls: pad (the real chunk
// into a zero-padded complex row, and the double prefix of its squares), power (|Z|^2 in place) and pick (the NSDF, its key
// maxima and the chosen peak).  One workgroup of 256 threads per chunk in pad and pick; blockIdx.y walks the streams.
//
// The arithmetic is the contract of zen_hip_pitch.h / DESIGN.md section 13, one IEEE operation at a time (contraction off):
// tests/pitch_model.py gives the same bits.  Where the contract fixes an order of additions (the runs of the prefix and
// their totals) one thread adds in that order.  Everything else is order-free: the key maxima are a set, the highest peak is
// a maximum, the chosen peak is the lowest index that passes a test -- so pick needs no ordered walk (see pick_kernel).
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

#include "pitch_kernels.h"

#pragma clang fp contract(off)

namespace zen_pitch {
namespace {

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int RUN = 64; // samples per run of the prefix

// ------------------------------------------------------------------------------------------------ pad
__global__ __launch_bounds__(TPB) void pad_kernel(PadArgs k)
{
	__shared__ double tot[TPB]; // the runs' totals, then the sum of the totals before each run (n / RUN <= 256)
	const int n = k.n, t = threadIdx.x;
	const int L = n < RUN ? n : RUN, runs = n / L;
	const size_t c = blockIdx.x;
	for (size_t s = blockIdx.y; s < k.n_streams; s += gridDim.y) {
		const size_t w = s * k.chunks + c;
		const float* __restrict__ x = k.in + s * k.in_stride + (k.c0 + c) * k.step; // 4-byte alignment only
		float4* __restrict__ z = reinterpret_cast<float4*>(k.z + w * 4 * (size_t)n); // two complex values per 16-byte store
		double* __restrict__ P = k.prefix + w * ((size_t)n + 1);
		for (int g = t; g < n; g += TPB)
			z[g] = g < n / 2 ? make_float4(x[2 * g], 0.0f, x[2 * g + 1], 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		if (t < runs) { // one thread per run: P[run start + i] = the sum of the i samples before it, left to right
			const float* __restrict__ xr = x + (size_t)t * L;
			double* __restrict__ pr = P + (size_t)t * L;
			double acc = 0.0;
			for (int i = 0; i < L; ++i) {
				pr[i] = acc;
				const double v = (double)xr[i];
				acc = acc + v * v; // (the square of a float is exact in double)
			}
			tot[t] = acc;
		}
		__threadfence_block();
		__syncthreads();
		if (t == 0) { // the association of the totals is the contract: one thread, in order
			double base = 0.0;
			for (int r = 0; r < runs; ++r) {
				const double v = tot[r];
				tot[r] = base;
				base = base + v;
			}
			P[n] = base;
		}
		__syncthreads();
		for (int j = t; j < n; j += TPB)
			P[j] = tot[j / L] + P[j];
		__syncthreads(); // tot is reused by the next stream
	}
}

// ------------------------------------------------------------------------------------------------ power
__global__ __launch_bounds__(TPB) void power_kernel(float4* __restrict__ z, size_t groups)
{
	for (size_t g = (size_t)blockIdx.x * TPB + threadIdx.x; g < groups; g += (size_t)gridDim.x * TPB) {
		const float4 v = z[g];
		z[g] = make_float4(v.x * v.x + v.y * v.y, 0.0f, v.z * v.z + v.w * v.w, 0.0f);
	}
}

// ------------------------------------------------------------------------------------------------ pick
struct Piece { // what a thread's segment contributes to runs that cross its borders
	float head_v, tail_v; // the best candidate in front of the segment's first non-positive value / behind its last one
	int head_i, tail_i;   // -1: none
	int open;             // the segment has no non-positive value: all of it is `head`
};

__device__ __forceinline__ int block_min(int v, int* scratch)
{
	for (int o = 32; o; o >>= 1) {
		const int u = __shfl_xor(v, o);
		v = u < v ? u : v;
	}
	__syncthreads();
	if ((threadIdx.x & 63) == 0)
		scratch[threadIdx.x >> 6] = v;
	__syncthreads();
	int r = scratch[0];
	for (int w = 1; w < WAVES; ++w)
		r = scratch[w] < r ? scratch[w] : r;
	return r;
}

__device__ __forceinline__ float block_max(float v, float* scratch)
{
	for (int o = 32; o; o >>= 1) {
		const float u = __shfl_xor(v, o);
		v = u > v ? u : v;
	}
	__syncthreads();
	if ((threadIdx.x & 63) == 0)
		scratch[threadIdx.x >> 6] = v;
	__syncthreads();
	float r = scratch[0];
	for (int w = 1; w < WAVES; ++w)
		r = scratch[w] > r ? scratch[w] : r;
	return r;
}

// the parabola through (i-1, i, i+1), float32, in the order of the contract
__device__ __forceinline__ void refine(const float* a, int i, float* pos, float* val)
{
	const float den = (a[i + 1] + a[i - 1]) - 2.0f * a[i];
	const float delta = a[i - 1] - a[i + 1];
	if (den == 0.0f) {
		*pos = (float)i;
		*val = a[i];
	} else {
		*pos = (float)i + delta / (2.0f * den);
		*val = a[i] - (delta * delta) / (8.0f * den);
	}
}

__device__ __forceinline__ bool is_key(const unsigned* bits, int i) { return (bits[i >> 5] >> (i & 31)) & 1u; }

// LDS: a[n] | one bit per index: key maximum | one Piece per thread | 4 words for the reductions
//
// Thread t owns the segment [t*E, (t+1)*E), E = n / 256 (1 below n = 256).  A run of positive values that begins and ends
// inside a segment is settled by its thread.  A run that crosses borders is settled by the thread in whose segment it begins:
// it takes its own `tail`, then the `head` of each following segment up to and including the first that is not open.  In
// both, a later candidate replaces the best so far only where it is larger, so the earliest of equal values stays.  Segments
// outside [p, n-2] count as non-positive.
__global__ __launch_bounds__(TPB) void pick_kernel(PickArgs k)
{
	extern __shared__ float lds[];
	const int n = k.n, t = threadIdx.x;
	float* a = lds;
	unsigned* bits = reinterpret_cast<unsigned*>(a + n);
	Piece* piece = reinterpret_cast<Piece*>(bits + n / 32);
	int* scratch = reinterpret_cast<int*>(piece + TPB);
	const int E = n >= TPB ? n / TPB : 1, s0 = t * E, s1 = s0 + E;
	const size_t c = blockIdx.x;
	for (size_t s = blockIdx.y; s < k.n_streams; s += gridDim.y) {
		const size_t w = s * k.chunks + c;
		const float* __restrict__ z = k.z + w * 4 * (size_t)n;
		const double* __restrict__ P = k.prefix + w * ((size_t)n + 1);
		float* __restrict__ nsdf = k.nsdf ? k.nsdf + (s * k.out_stride + k.c0 + c) * (size_t)n : nullptr;
		// ---- the NSDF: one double division per element
		const double p0 = P[0], pn = P[n];
		for (int j = t; j < n; j += TPB) {
			const double m = (P[n - j] - p0) + (pn - P[j]);
			const float v = m > 0.0 ? (float)((double)z[2 * j] / ((double)n * m)) : 0.0f;
			a[j] = v;
			if (nsdf)
				nsdf[j] = v;
		}
		for (int j = t; j < n / 32; j += TPB)
			bits[j] = 0u;
		__syncthreads();
		// ---- p: the smaller of T and the first non-positive index, then on to the first positive one (at most n - 1)
		int mine = n;
		for (int j = t; j < n; j += TPB)
			if (a[j] <= 0.0f) {
				mine = j;
				break;
			}
		int p = block_min(mine, scratch);
		const int T = (n - 1) / 3;
		p = p < T ? p : T;
		mine = n - 1;
		for (int j = p + t; j < n - 1; j += TPB)
			if (a[j] > 0.0f) {
				mine = j;
				break;
			}
		p = block_min(mine, scratch);
		// ---- the segment
		{
			Piece q = {0.0f, 0.0f, -1, -1, 1};
			const int lo = s0 > p ? s0 : p, hi = s1 < n - 1 ? s1 : n - 1; // [lo, hi): the part of the segment in [p, n-2]
			if (lo >= hi) {
				q.open = 0;
			} else {
				if (s0 < p)
					q.open = 0; // what lies in front of p ends a run
				float bv = 0.0f;
				int bi = -1;
				for (int i = lo; i < hi; ++i) {
					const float v = a[i];
					if (v > 0.0f) {
						if (i >= 1 && v > a[i - 1] && v >= a[i + 1] && (bi < 0 || v > bv)) {
							bv = v;
							bi = i;
						}
					} else {
						if (q.open) {
							q.head_v = bv;
							q.head_i = bi;
							q.open = 0;
						} else if (bi >= 0) {
							atomicOr(&bits[bi >> 5], 1u << (bi & 31));
						}
						bv = 0.0f;
						bi = -1;
					}
				}
				if (q.open) {
					q.head_v = bv;
					q.head_i = bi;
				} else {
					q.tail_v = bv;
					q.tail_i = bi;
				}
			}
			piece[t] = q;
			__syncthreads();
			// ---- the runs that cross borders; thread 0 also settles the one that begins in front of segment 0
			for (int from = (t == 0 ? -1 : t); from <= t; ++from) {
				if (from >= 0 && q.open)
					break;
				float bv = from < 0 ? 0.0f : q.tail_v;
				int bi = from < 0 ? -1 : q.tail_i;
				for (int u = from + 1; u < TPB; ++u) {
					const Piece o = piece[u];
					if (o.head_i >= 0 && (bi < 0 || o.head_v > bv)) {
						bv = o.head_v;
						bi = o.head_i;
					}
					if (!o.open)
						break;
				}
				if (bi >= 0)
					atomicOr(&bits[bi >> 5], 1u << (bi & 31));
			}
			__syncthreads();
		}
		// ---- the highest value among the key maxima and the refined peaks (a maximum: no order needed)
		const int end = s1 < n ? s1 : n;
		float top = 0.0f;
		for (int i = s0; i < end; ++i)
			if (is_key(bits, i)) {
				top = a[i] > top ? a[i] : top;
				if (a[i] > 0.5f) {
					float pos, val;
					refine(a, i, &pos, &val);
					top = val > top ? val : top;
				}
			}
		top = block_max(top, reinterpret_cast<float*>(scratch));
		// ---- the first refined peak that reaches the cut
		const float cut = (float)(0.93 * (double)top);
		float pos = 0.0f, val = 0.0f;
		mine = INT_MAX;
		for (int i = s0; i < end; ++i)
			if (is_key(bits, i) && a[i] > 0.5f) {
				refine(a, i, &pos, &val);
				if (val >= cut) {
					mine = i;
					break;
				}
			}
		const int first = block_min(mine, scratch);
		const size_t o = s * k.out_stride + k.c0 + c;
		if (first == INT_MAX ? t == 0 : mine == first) {
			float pitch = -1.0f;
			if (first == INT_MAX) {
				pos = 0.0f;
				val = 0.0f;
			} else {
				const float f = k.fs / pos;
				pitch = f > 80.0f ? f : -1.0f;
			}
			if (k.pitch)
				k.pitch[o] = pitch;
			if (k.period)
				k.period[o] = pos;
			if (k.clarity)
				k.clarity[o] = val;
		}
		__syncthreads(); // the LDS is reused by the next stream
	}
}

unsigned stream_rows(size_t n_streams) { return (unsigned)(n_streams < 65535 ? n_streams : 65535); }

} // namespace

size_t pick_lds_bytes(int n) { return sizeof(float) * (size_t)n + sizeof(unsigned) * (size_t)(n / 32) + sizeof(Piece) * TPB + sizeof(int) * WAVES; }

hipError_t prepare_pick(int n)
{
	const size_t lds = pick_lds_bytes(n);
	if (lds > 64 * 1024)
		return hipFuncSetAttribute((const void*)pick_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
	return hipSuccess;
}

hipError_t launch_pad(const PadArgs& a, hipStream_t s)
{
	if (a.chunks == 0 || a.n_streams == 0)
		return hipSuccess;
	pad_kernel<<<dim3((unsigned)a.chunks, stream_rows(a.n_streams), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_power(float* z, size_t bins, hipStream_t s)
{
	const size_t groups = bins / 2;
	if (groups == 0)
		return hipSuccess;
	static unsigned cap = 0; // 8 workgroups of 256 threads per CU: the 32 wavefronts a CU holds
	if (!cap) {
		int dev = 0, cus = 0;
		if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
			cus = 256;
		(void)hipGetLastError();
		cap = 8u * (unsigned)cus;
	}
	size_t gx = (groups + TPB - 1) / TPB;
	if (gx > cap)
		gx = cap;
	power_kernel<<<dim3((unsigned)gx, 1, 1), TPB, 0, s>>>(reinterpret_cast<float4*>(z), groups);
	return hipGetLastError();
}

hipError_t launch_pick(const PickArgs& a, hipStream_t s)
{
	if (a.chunks == 0 || a.n_streams == 0)
		return hipSuccess;
	pick_kernel<<<dim3((unsigned)a.chunks, stream_rows(a.n_streams), 1), TPB, pick_lds_bytes(a.n), s>>>(a);
	return hipGetLastError();
}

} // namespace zen_pitch
