// repsim_kernels.hip -- the kernels of libzen_hip_repsim.so (gfx950) around the public FFT call: frame (the windowed frames as
// complex rows), magnitude, similarity (V V^T over the bins, divided by the rows' norms: the hot kernel, on the matrix cores
// or on the vector ALU), select (the k most similar frames of a frame, a minimum distance apart), gather_median (the median
// over the selected frames), mask (the soft mask applied to a frame's spectrum in place) and overlap_add.
//
// The arithmetic is the contract of zen_hip_repsim.h / DESIGN.md section 19, one IEEE float32 operation at a time (contraction
// off, hipcc's correctly rounded division and square root): tests/repsim_model.py gives the same bits.  The one sum whose
// order the contract fixes (D, over the bins) is an fma chain in that order on both routes: v_mfma_f32_32x32x2_f32 adds its
// two products in k order with one rounding each, and the K loop feeds it the bins in rising order.  A median is a selection:
// it is exact however it is found, so the two paths of gather_median (a sorting network in registers, a search by rank through
// lane-private columns in LDS) give the same values.  frame, magnitude, the body of mask, the sample of overlap_add and the
// loader of the similarity's LDS tiles are zen_amd/addon/stft_kernels.h's, the network and the register path of the median
// zen_amd/addon/median_select.h's: shared with zen_amd/repet and nmf.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../addon/median_select.h"
#include "../addon/stft_kernels.h"
#include "repsim_kernels.h"

#pragma clang fp contract(off)

namespace zen_repsim {
namespace {

using namespace zen_addon;

// ------------------------------------------------------------------------------------------------ similarity
// A workgroup of four waves computes a SIM_TILE x SIM_TILE block of S: wave w the 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2
// tiles of 32 x 32, 16 accumulators per tile and lane.  The bins go by in chunks of KC through two LDS tiles (the rows a of
// the block and its rows b; a row of KC + 1 words keeps the 64 lanes of an operand read on 64 banks).  Where a chunk runs
// past the bins the b side is padded with +0 and the a side with -0: the product is -0 and fma(-0, +0, acc) is acc for every
// acc, -0 included, so the chain ends at the last bin whatever V holds.  Rows past ma / mb are padding too and never stored.
//
// Both routes keep a result in the same lane and register (the matrix core's C/D map: column = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so they share the epilogue.  The norms of the block's 2 x 128 rows are the
// same chain with both factors one row, carried by one thread per row beside the products: 1/128 of the block's work.
typedef float f32x16 __attribute__((ext_vector_type(16)));

template <bool MFMA, bool VEC>
__global__ __launch_bounds__(TPB) void similarity_kernel(SimArgs k)
{
	__shared__ float As[SIM_TILE * LDK];
	__shared__ float Bs[SIM_TILE * LDK];
	__shared__ float nrm[2 * SIM_TILE];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int l31 = lane & 31, hi = lane >> 5;
	const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
	const size_t a0 = (size_t)blockIdx.y * SIM_TILE, b0 = (size_t)blockIdx.x * SIM_TILE;
	f32x16 acc[2][2];
#pragma unroll
	for (int ti = 0; ti < 2; ++ti)
#pragma unroll
		for (int tj = 0; tj < 2; ++tj)
#pragma unroll
			for (int r = 0; r < 16; ++r)
				acc[ti][tj][r] = 0.0f;
	float nn = 0.0f; // D[row][row] of row tid of the a side, tid - SIM_TILE of the b side
	const float* __restrict__ mine = tid < SIM_TILE ? As + tid * LDK : Bs + (tid - SIM_TILE) * LDK;
	for (size_t f0 = 0; f0 < k.bins; f0 += KC) {
		load_tile<SIM_TILE, VEC>(As, k.va, k.v_stride, a0, k.ma, f0, k.bins, -0.0f, tid);
		load_tile<SIM_TILE, VEC>(Bs, k.vb, k.v_stride, b0, k.mb, f0, k.bins, 0.0f, tid);
		__syncthreads();
#pragma unroll
		for (int kk = 0; kk < KC; ++kk)
			nn = __builtin_fmaf(mine[kk], mine[kk], nn);
		if (MFMA) {
#pragma unroll 4
			for (int kk = 0; kk < KC; kk += 2) { // lanes 0..31 bring bin kk, lanes 32..63 bin kk + 1: added in that order
				float a[2], b[2];
#pragma unroll
				for (int t = 0; t < 2; ++t) {
					a[t] = As[(wr + t * 32 + l31) * LDK + kk + hi];
					b[t] = Bs[(wc + t * 32 + l31) * LDK + kk + hi];
				}
#pragma unroll
				for (int ti = 0; ti < 2; ++ti)
#pragma unroll
					for (int tj = 0; tj < 2; ++tj)
						acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ti], b[tj], acc[ti][tj], 0, 0, 0);
			}
		} else {
#pragma unroll 2
			for (int kk = 0; kk < KC; ++kk) {
				float b[2];
#pragma unroll
				for (int t = 0; t < 2; ++t)
					b[t] = Bs[(wc + t * 32 + l31) * LDK + kk];
#pragma unroll
				for (int ti = 0; ti < 2; ++ti)
#pragma unroll
					for (int r = 0; r < 16; ++r) {
						const float a = As[(wr + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi) * LDK + kk];
#pragma unroll
						for (int tj = 0; tj < 2; ++tj)
							acc[ti][tj][r] = __builtin_fmaf(a, b[tj], acc[ti][tj][r]);
					}
			}
		}
		__syncthreads();
	}
	nrm[tid] = sqrtf(nn);
	__syncthreads();
#pragma unroll
	for (int ti = 0; ti < 2; ++ti)
#pragma unroll
		for (int tj = 0; tj < 2; ++tj) {
			const int col = wc + tj * 32 + l31;
			const size_t b = b0 + col;
			const float nb = nrm[SIM_TILE + col];
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int row = wr + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
				const size_t a = a0 + row;
				if (a < k.ma && b < k.mb) {
					const float den = nrm[row] * nb;
					k.s[a * k.s_stride + b] = den > 0.0f ? acc[ti][tj][r] / den : 0.0f;
				}
			}
		}
}

// ------------------------------------------------------------------------------------------------ select
// One workgroup per frame; its row of S sits in LDS with everything that is no candidate (not above t, a NaN, removed) as
// -inf.  A thread keeps the first index of the largest candidate among its own words (b = tid, tid + 256, ..), a round is a
// workgroup-wide argmax of those (the larger value, the smaller index among equals) and the clearing of the neighbourhood;
// only a thread whose own best was cleared looks through its words again.  Dynamic LDS: m floats.
__device__ __forceinline__ void better(float& v, int& i, float ov, int oi)
{
	if (ov > v || (ov == v && oi < i)) {
		v = ov;
		i = oi;
	}
}

__device__ __forceinline__ void rescan(const float* row, int m, int tid, float& bv, int& bi)
{
	bv = -INFINITY;
	bi = INT_MAX;
	for (int b = tid; b < m; b += TPB) {
		const float v = row[b];
		if (v > bv) {
			bv = v;
			bi = b;
		}
	}
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void select_kernel(SelectArgs k)
{
	extern __shared__ float row[];
	__shared__ float wv[TPB / 64];
	__shared__ int wi[TPB / 64];
	const size_t a = blockIdx.x;
	const int m = (int)k.m, tid = threadIdx.x;
	const float* __restrict__ s = k.s + a * k.s_stride;
	int* __restrict__ idx = k.idx + a * (size_t)k.k;
	if (VEC) { // s 16-byte aligned, s_stride a multiple of 4
		for (int b = tid * 4; b < m; b += TPB * 4) {
			if (b + 4 <= m) {
				const float4 x = *reinterpret_cast<const float4*>(s + b);
				row[b] = x.x > k.t ? x.x : -INFINITY;
				row[b + 1] = x.y > k.t ? x.y : -INFINITY;
				row[b + 2] = x.z > k.t ? x.z : -INFINITY;
				row[b + 3] = x.w > k.t ? x.w : -INFINITY;
			} else {
				for (int e = b; e < m; ++e) {
					const float v = s[e];
					row[e] = v > k.t ? v : -INFINITY;
				}
			}
		}
	} else {
		for (int b = tid; b < m; b += TPB) {
			const float v = s[b];
			row[b] = v > k.t ? v : -INFINITY;
		}
	}
	__syncthreads();
	float bv;
	int bi;
	rescan(row, m, tid, bv, bi);
	int c = 0;
	for (; c < k.k; ++c) {
		float v = bv;
		int i = bi;
#pragma unroll
		for (int off = 32; off > 0; off >>= 1) {
			const float ov = __shfl_xor(v, off, 64);
			const int oi = __shfl_xor(i, off, 64);
			better(v, i, ov, oi);
		}
		if ((tid & 63) == 0) {
			wv[tid >> 6] = v;
			wi[tid >> 6] = i;
		}
		__syncthreads();
		v = wv[0];
		i = wi[0];
#pragma unroll
		for (int w = 1; w < TPB / 64; ++w)
			better(v, i, wv[w], wi[w]);
		if (!(v > -INFINITY)) // no candidate is left: the same for every thread
			break;
		if (tid == 0)
			idx[c] = i;
		const int lo = i - k.dd + 1 > 0 ? i - k.dd + 1 : 0, hi = i + k.dd - 1 < m - 1 ? i + k.dd - 1 : m - 1;
		for (int b = lo + tid; b <= hi; b += TPB)
			row[b] = -INFINITY;
		__syncthreads();
		if (bi >= lo && bi <= hi)
			rescan(row, m, tid, bv, bi);
	}
	for (int q = c + tid; q < k.k; q += TPB)
		idx[q] = -1;
	if (tid == 0)
		k.counts[a] = c;
}

// ------------------------------------------------------------------------------------------------ gather median
__device__ __forceinline__ int clamp_count(int c, int k) { return c < 0 ? 0 : c > k ? k : c; }
__device__ __forceinline__ size_t clamp_frame(int j, size_t m) { return j < 0 ? 0 : (size_t)j >= m ? m - 1 : (size_t)j; }

struct GatheredRows { // row q of the median of a frame: the q-th frame its selection names, q < c
	const GatherArgs& k;
	const int* __restrict__ idx;
	int c;
	__device__ bool present(int q) const { return q < c; }
	__device__ const float* row(int q) const { return k.v + (q < c ? clamp_frame(idx[q], k.m) : 0) * k.v_stride; } // idx has c entries
};

// The frames of up to REGISTER_NEIGHBOURS neighbours: a wave per frame, a lane has VEC adjacent bins (median_select.h), the
// network picked by the frame's count (the same for the whole wave).  Frames with more leave at once: median_lds_kernel has
// them.  VEC = 4 wants v and u 16-byte aligned and both strides multiples of 4.
template <int VEC>
__global__ __launch_bounds__(TPB) void median_reg_kernel(GatherArgs k)
{
	const size_t f = ((size_t)blockIdx.x * 64 + (threadIdx.x & 63)) * VEC;
	const size_t a = (size_t)blockIdx.y * (TPB / 64) + threadIdx.x / 64;
	if (f >= k.bins || a >= k.rows)
		return;
	const int c = clamp_count(k.counts[a], k.k);
	if (c > REGISTER_NEIGHBOURS)
		return;
	const GatheredRows rows = {k, k.idx + a * (size_t)k.k, c};
	float* __restrict__ out = k.u + a * k.u_stride + f;
	if (c == 0) {
#pragma unroll
		for (int e = 0; e < VEC; ++e)
			if (f + e < k.bins)
				out[e] = 0.0f;
	} else if (c <= 2) {
		median_in_registers<2, VEC>(rows, f, k.bins, out);
	} else if (c <= 4) {
		median_in_registers<4, VEC>(rows, f, k.bins, out);
	} else if (c <= 8) {
		median_in_registers<8, VEC>(rows, f, k.bins, out);
	} else if (c <= 16) {
		median_in_registers<16, VEC>(rows, f, k.bins, out);
	} else {
		median_in_registers<REGISTER_NEIGHBOURS, VEC>(rows, f, k.bins, out);
	}
}

// The frames of 33..256 neighbours: a lane keeps its column in LDS (word q * 64 + lane: lane-private, every access of a wave
// on 64 different banks) as keys, unsigned words in the order of the floats, and finds the key of rank (c - 1) / 2 a bit at a
// time from the top: the largest word that fewer than rank + 1 keys lie below.  That is 32 counting passes over the column
// whatever it holds; an even count takes one more for the next key up.  A sort of the same column in LDS (the bitonic
// network, pair by pair) waits on LDS at every pair and took 21.9 ms where this takes a fraction.
// No lane reads another lane's words, so nothing is synchronised.  Dynamic LDS: 64 words per neighbour the launch's k allows.
__device__ __forceinline__ unsigned key_of(float x)
{
	const unsigned u = __float_as_uint(x);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float value_of(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

__global__ __launch_bounds__(64) void median_lds_kernel(GatherArgs k)
{
	extern __shared__ unsigned col[];
	const int lane = threadIdx.x;
	const size_t f = (size_t)blockIdx.x * 64 + lane, a = blockIdx.y;
	if (f >= k.bins || a >= k.rows)
		return;
	const int c = clamp_count(k.counts[a], k.k);
	if (c <= REGISTER_NEIGHBOURS)
		return;
	const int* __restrict__ idx = k.idx + a * (size_t)k.k;
	for (int q = 0; q < c; ++q)
		col[q * 64 + lane] = key_of(k.v[clamp_frame(idx[q], k.m) * k.v_stride + f]);
	const int lo = (c - 1) >> 1;
	unsigned ans = 0;
	for (int bit = 31; bit >= 0; --bit) {
		const unsigned cand = ans | (1u << bit);
		int below = 0;
#pragma unroll 8
		for (int q = 0; q < c; ++q)
			below += col[q * 64 + lane] < cand ? 1 : 0;
		if (below <= lo)
			ans = cand;
	}
	const float slo = value_of(ans);
	float shi = slo;
	if (!(c & 1)) { // the value of rank lo + 1: slo again where more than lo + 1 keys are at or below it, else the next key up
		int le = 0;
		unsigned next = 0xffffffffu;
#pragma unroll 8
		for (int q = 0; q < c; ++q) {
			const unsigned key = col[q * 64 + lane];
			le += key <= ans ? 1 : 0;
			next = key > ans && key < next ? key : next;
		}
		if (le <= lo + 1)
			shi = value_of(next);
	}
	k.u[a * k.u_stride + f] = (c & 1) ? slo : (slo + shi) * 0.5f;
}

// ------------------------------------------------------------------------------------------------ mask
__global__ __launch_bounds__(TPB) void mask_kernel(MaskArgs k)
{
	const size_t fr = blockIdx.x; // the model of a frame is its own row of U
	soft_mask_frame(reinterpret_cast<float2*>(k.rows) + fr * (size_t)k.N, k.v + fr * k.v_stride, k.u + fr * k.v_stride, k.N, k.kc);
}

// ------------------------------------------------------------------------------------------------ overlap-add
__global__ __launch_bounds__(TPB) void overlap_add_kernel(OlaArgs k)
{
	const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
	if (t >= k.n)
		return;
	const float x = k.in[t];
	const float bg = overlap_add_sample(k.rows, k.div, t, k.N);
	if (k.background)
		k.background[t] = bg;
	if (k.foreground)
		k.foreground[t] = x - bg;
}

} // namespace

hipError_t launch_frame(const FrameArgs& a, hipStream_t s) { return zen_addon::launch_frame(a, s); }
hipError_t launch_magnitude(const MagArgs& a, hipStream_t s) { return zen_addon::launch_magnitude(a, s); }

hipError_t launch_similarity(const SimArgs& a, bool mfma, hipStream_t s)
{
	if (a.ma == 0 || a.mb == 0 || a.bins == 0 || a.ma > MAX_FRAMES || a.mb > MAX_FRAMES || a.v_stride < a.bins || a.s_stride < a.mb)
		return hipErrorInvalidValue;
	const dim3 grid((unsigned)((a.mb + SIM_TILE - 1) / SIM_TILE), (unsigned)((a.ma + SIM_TILE - 1) / SIM_TILE), 1);
	const bool vec = aligned16(a.va) && aligned16(a.vb) && a.v_stride % 4 == 0;
	if (mfma && vec)
		similarity_kernel<true, true><<<grid, TPB, 0, s>>>(a);
	else if (mfma)
		similarity_kernel<true, false><<<grid, TPB, 0, s>>>(a);
	else if (vec)
		similarity_kernel<false, true><<<grid, TPB, 0, s>>>(a);
	else
		similarity_kernel<false, false><<<grid, TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_select(const SelectArgs& a, hipStream_t s)
{
	if (a.rows == 0 || a.m == 0 || a.m > MAX_FRAMES || a.rows > MAX_FRAMES || a.s_stride < a.m || a.k < 1 || a.k > MAX_NEIGHBOURS || a.dd < 1 ||
	    (size_t)a.dd > a.m)
		return hipErrorInvalidValue;
	const size_t lds = sizeof(float) * a.m;
	const bool vec = aligned16(a.s) && a.s_stride % 4 == 0;
	// the row of the longest clip and the four words of the argmax are a little over 64 KiB
	static const hipError_t raised[2] = {
	    hipFuncSetAttribute((const void*)select_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(float) * MAX_FRAMES),
	    hipFuncSetAttribute((const void*)select_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(float) * MAX_FRAMES)};
	if (lds + 64 > 64 * 1024 && raised[vec] != hipSuccess)
		return raised[vec];
	if (vec)
		select_kernel<true><<<dim3((unsigned)a.rows, 1, 1), TPB, lds, s>>>(a);
	else
		select_kernel<false><<<dim3((unsigned)a.rows, 1, 1), TPB, lds, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_gather_median(const GatherArgs& a, hipStream_t s)
{
	if (a.rows == 0 || a.rows > MAX_FRAMES || a.m == 0 || a.bins == 0 || a.bins > ((size_t)1 << 30) || a.k < 1 || a.k > MAX_NEIGHBOURS ||
	    a.v_stride < a.bins || a.u_stride < a.bins)
		return hipErrorInvalidValue;
	const bool vec = aligned16(a.v) && aligned16(a.u) && a.v_stride % 4 == 0 && a.u_stride % 4 == 0;
	const unsigned rows = (unsigned)((a.rows + TPB / 64 - 1) / (TPB / 64));
	if (vec)
		median_reg_kernel<4><<<dim3((unsigned)((a.bins + 255) / 256), rows, 1), TPB, 0, s>>>(a);
	else
		median_reg_kernel<1><<<dim3((unsigned)((a.bins + 63) / 64), rows, 1), TPB, 0, s>>>(a);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess || a.k <= REGISTER_NEIGHBOURS)
		return e;
	median_lds_kernel<<<dim3((unsigned)((a.bins + 63) / 64), (unsigned)a.rows, 1), 64, sizeof(unsigned) * 64 * a.k, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_mask(const MaskArgs& a, hipStream_t s)
{
	if (a.m == 0)
		return hipErrorInvalidValue;
	mask_kernel<<<dim3((unsigned)a.m, 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_overlap_add(const OlaArgs& a, hipStream_t s)
{
	if (a.n == 0)
		return hipSuccess;
	overlap_add_kernel<<<dim3((unsigned)((a.n + TPB - 1) / TPB), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace zen_repsim
