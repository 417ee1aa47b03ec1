// nmf_kernels.hip -- the kernels of libzen_hip_nmf.so (gfx950) around the public FFT call: frame (the windowed frames as
// complex rows), magnitude, product (the three matrix products of an iteration with their divisions as epilogues: the hot
// kernel, on the matrix cores or on the vector ALU), stem_mask (the chains L and L_g, one division, applied to a copy of a
// frame's spectrum) and overlap_add.
//
// The arithmetic is the contract of zen_hip_nmf.h / DESIGN.md section 20, one IEEE float32 operation at a time (contraction
// off, hipcc's correctly rounded division and square root): tests/nmf_model.py gives the same bits.  Every sum whose order the
// contract fixes is an fma chain in that order on both routes: v_mfma_f32_32x32x2_f32 adds its two products in k order with
// one rounding each, the reduction loop feeds it the indices in rising order, and at every 256th index the accumulators are
// added to the running totals (the first is taken as it is) and start again from +0 -- the segments of the contract.  frame,
// magnitude, the sample of overlap_add and the loader of a reduction-minor LDS tile are zen_amd/addon/stft_kernels.h's: shared
// with zen_amd/repet and repsim.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../addon/stft_kernels.h"
#include "nmf_kernels.h"

#pragma clang fp contract(off)

namespace zen_nmf {
namespace {

using namespace zen_addon;

constexpr float EPS = 0x1p-40f;

// ------------------------------------------------------------------------------------------------ product
// A workgroup of four waves computes a TILE x TILE block of a product: wave w the 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2
// tiles of 32 x 32, 16 accumulators per tile and lane.  The reduction goes by in chunks of KC through two LDS tiles, both held
// as [row or column of the output][index of the reduction]: a row of KC + 1 words keeps the 64 lanes of an operand read on 64
// banks.  A reduction-minor operand is read as it lies; a reduction-major one (H in H^T W, W in H^T W, Q in H Q) is read
// along its rows, which are the output's rows or columns, and turned on its way into LDS (word (i, r) is 33 i + r: 33 is odd,
// so a wave's 64 rows i are 64 banks).  Where a chunk runs past the reduction the B side is padded with +0 and the A side
// with -0: the product is -0 and fma(-0, +0, acc) is acc for every acc, -0 included, so the chain ends at the last index
// whatever the operands hold.  Rows and columns past I / J are padding too and never stored.
//
// Both routes keep a result in the same lane and register (the matrix core's C/D map: column = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so they share the epilogue.  The row sums s and t of the two updates are
// sums over the A operand's rows along the same reduction with the same segments: one thread per row of the block carries
// fma(A, 1, acc) beside the products, 1/128 of the block's work, and no launch or scratch of their own.  x + (-0) is x, so
// the padding leaves them alone as well.
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Rows r0.. of a reduction-minor operand go through stft_kernels.h's load_tile.  The other one, with the same arguments:
// T[r * LDK + q] = v[(l0 + q) * stride + r0 + r]: columns r0.. of a reduction-major operand
template <bool VEC>
__device__ __forceinline__ void load_major(float* __restrict__ T, const float* __restrict__ v, size_t stride, size_t r0, size_t rows, size_t l0,
                                           size_t L, float pad, int tid)
{
	if (VEC) { // v 16-byte aligned, stride a multiple of 4; r0 is a multiple of TILE
#pragma unroll
		for (int i = 0; i < TILE * KC / 4 / TPB; ++i) {
			const int s = tid + TPB * i, q = s >> 5, r = (s & 31) * 4;
			const size_t row = r0 + r, l = l0 + q;
			float4 x = make_float4(pad, pad, pad, pad);
			if (l < L) {
				const float* __restrict__ p = v + l * stride + row;
				if (row + 4 <= rows) {
					x = *reinterpret_cast<const float4*>(p);
				} else {
					x.x = row < rows ? p[0] : pad;
					x.y = row + 1 < rows ? p[1] : pad;
					x.z = row + 2 < rows ? p[2] : pad;
				}
			}
			float* __restrict__ d = T + r * LDK + q;
			d[0] = x.x;
			d[LDK] = x.y;
			d[2 * LDK] = x.z;
			d[3 * LDK] = x.w;
		}
	} else {
#pragma unroll
		for (int i = 0; i < TILE * KC / TPB; ++i) {
			const int e = tid + TPB * i, q = e >> 7, r = e & 127;
			const size_t row = r0 + r, l = l0 + q;
			T[r * LDK + q] = row < rows && l < L ? v[l * stride + row] : pad;
		}
	}
}

// PART: the workgroup carries segment blockIdx.z alone and stores its raw sums (ProductArgs::part); combine_kernel has the rest.
template <int WHICH, bool MFMA, bool VEC, bool PART>
__global__ __launch_bounds__(TPB) void product_kernel(ProductArgs k)
{
	constexpr bool A_MAJOR = WHICH == RATIO, B_MAJOR = WHICH != UPDATE_H, SEG = WHICH != RATIO; // RATIO: L <= 256, one segment
	static_assert(!PART || SEG, "only the updates have segments to split");
	__shared__ float As[TILE * LDK];
	__shared__ float Bs[TILE * LDK];
	__shared__ float rowsum[TILE];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int l31 = lane & 31, hi = lane >> 5;
	const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
	const size_t i0 = (size_t)blockIdx.y * TILE, j0 = (size_t)blockIdx.x * TILE;
	f32x16 acc[2][2], tot[2][2];
#pragma unroll
	for (int ti = 0; ti < 2; ++ti)
#pragma unroll
		for (int tj = 0; tj < 2; ++tj)
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				acc[ti][tj][r] = 0.0f;
				tot[ti][tj][r] = 0.0f;
			}
	float rs = 0.0f, rs_tot = 0.0f; // the sum of row tid of the A side, tid < TILE
	bool first = true;              // no segment is in the totals yet
	const float* __restrict__ mine = As + (tid & (TILE - 1)) * LDK;
	const size_t l_begin = PART ? (size_t)blockIdx.z * SEGMENT : 0, l_end = PART && l_begin + SEGMENT < k.L ? l_begin + SEGMENT : k.L;
	for (size_t l0 = l_begin; l0 < l_end; l0 += KC) {
		if (A_MAJOR)
			load_major<VEC>(As, k.a, k.a_stride, i0, k.I, l0, k.L, -0.0f, tid);
		else
			load_tile<TILE, VEC>(As, k.a, k.a_stride, i0, k.I, l0, k.L, -0.0f, tid);
		if (B_MAJOR)
			load_major<VEC>(Bs, k.b, k.b_stride, j0, k.J, l0, k.L, 0.0f, tid);
		else
			load_tile<TILE, VEC>(Bs, k.b, k.b_stride, j0, k.J, l0, k.L, 0.0f, tid);
		__syncthreads();
		if (SEG) {
#pragma unroll
			for (int kk = 0; kk < KC; ++kk)
				rs = __builtin_fmaf(mine[kk], 1.0f, rs);
		}
		if (MFMA) {
#pragma unroll 4
			for (int kk = 0; kk < KC; kk += 2) { // lanes 0..31 bring index kk, lanes 32..63 index kk + 1: added in that order
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
		// the end of a segment that is not the last: its sums join the totals, the accumulators start again from +0
		if (SEG && !PART && (l0 + KC) % SEGMENT == 0 && l0 + KC < k.L) {
#pragma unroll
			for (int ti = 0; ti < 2; ++ti)
#pragma unroll
				for (int tj = 0; tj < 2; ++tj)
#pragma unroll
					for (int r = 0; r < 16; ++r) {
						tot[ti][tj][r] = first ? acc[ti][tj][r] : tot[ti][tj][r] + acc[ti][tj][r];
						acc[ti][tj][r] = 0.0f;
					}
			rs_tot = first ? rs : rs_tot + rs;
			rs = 0.0f;
			first = false;
		}
	}
	if (PART) {
		const size_t z = blockIdx.z;
		if (blockIdx.x == 0 && tid < TILE && i0 + tid < k.I)
			k.part_rs[z * k.I + i0 + tid] = rs;
#pragma unroll
		for (int ti = 0; ti < 2; ++ti)
#pragma unroll
			for (int tj = 0; tj < 2; ++tj) {
				const size_t j = j0 + wc + tj * 32 + l31;
#pragma unroll
				for (int r = 0; r < 16; ++r) {
					const size_t i = i0 + wr + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
					if (i < k.I && j < k.J)
						k.part[(z * k.I + i) * k.J + j] = acc[ti][tj][r];
				}
			}
		return;
	}
	if (SEG) {
		if (!first) { // the last segment
#pragma unroll
			for (int ti = 0; ti < 2; ++ti)
#pragma unroll
				for (int tj = 0; tj < 2; ++tj)
#pragma unroll
					for (int r = 0; r < 16; ++r)
						acc[ti][tj][r] = tot[ti][tj][r] + acc[ti][tj][r];
			rs = rs_tot + rs;
		}
		if (tid < TILE)
			rowsum[tid] = rs;
		__syncthreads();
	}
#pragma unroll
	for (int ti = 0; ti < 2; ++ti)
#pragma unroll
		for (int tj = 0; tj < 2; ++tj) {
			const size_t j = j0 + wc + tj * 32 + l31;
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int row = wr + ti * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
				const size_t i = i0 + row;
				if (i < k.I && j < k.J) {
					const float sum = acc[ti][tj][r], e = k.e[i * k.e_stride + j];
					if (WHICH == RATIO) {
						if (k.lam)
							k.lam[i * k.lam_stride + j] = sum;
						k.out[i * k.out_stride + j] = e / fmaxf(sum, EPS);
					} else {
						const float prod = e * sum;
						k.out[i * k.out_stride + j] = prod / fmaxf(rowsum[row], EPS);
					}
				}
			}
		}
}

// The second half of a split update: the segments' sums in rising order (the first as it is), the row sum alike, the epilogue.
struct CombineArgs {
	const float* part;
	const float* part_rs;
	const float* e;
	float* out;
	size_t e_stride, out_stride, I, J, segments;
};

__global__ __launch_bounds__(TPB) void combine_kernel(CombineArgs k)
{
	const size_t j = (size_t)blockIdx.x * TPB + threadIdx.x, i = blockIdx.y;
	if (j >= k.J)
		return;
	float sum = k.part[i * k.J + j], rs = k.part_rs[i];
	for (size_t z = 1; z < k.segments; ++z) {
		sum = sum + k.part[(z * k.I + i) * k.J + j];
		rs = rs + k.part_rs[z * k.I + i];
	}
	const float prod = k.e[i * k.e_stride + j] * sum;
	k.out[i * k.out_stride + j] = prod / fmaxf(rs, EPS);
}

// ------------------------------------------------------------------------------------------------ stem mask
// One workgroup per frame, a thread per bin: the chains L (every component) and L_g (the group's) in rising k from +0, the
// mask L_g / L and the frame's spectrum through it into y, bin N - f with the mask of bin f.
__global__ __launch_bounds__(TPB) void stem_mask_kernel(StemArgs k)
{
	const int N = k.N, H = N / 2;
	const size_t fr = blockIdx.x;
	const float2* __restrict__ x = reinterpret_cast<const float2*>(k.x) + fr * (size_t)N;
	float2* __restrict__ y = reinterpret_cast<float2*>(k.y) + fr * (size_t)N;
	for (int f = threadIdx.x; f <= H; f += TPB) {
		float lam = 0.0f, lg = 0.0f;
		for (int c = 0; c < k.K; ++c) {
			const float hv = k.h[(size_t)c * k.h_stride + fr], wv = k.w[(size_t)c * k.w_stride + f];
			lam = __builtin_fmaf(hv, wv, lam);
			if ((k.member[c >> 5] >> (c & 31)) & 1u)
				lg = __builtin_fmaf(hv, wv, lg);
		}
		const float M = lam > 0.0f ? lg / lam : 0.0f;
		const float2 z = x[f];
		y[f] = make_float2(z.x * M, z.y * M);
		if (f > 0 && f < H) {
			const float2 u = x[N - f];
			y[N - f] = make_float2(u.x * M, u.y * M);
		}
	}
}

// ------------------------------------------------------------------------------------------------ overlap-add
__global__ __launch_bounds__(TPB) void overlap_add_kernel(OlaArgs k)
{
	const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
	if (t >= k.n)
		return;
	k.out[t] = overlap_add_sample(k.rows, k.div, t, k.N);
}

template <int WHICH, bool PART>
hipError_t launch_one(const ProductArgs& a, bool mfma, hipStream_t s)
{
	const dim3 grid((unsigned)((a.J + TILE - 1) / TILE), (unsigned)((a.I + TILE - 1) / TILE), PART ? (unsigned)((a.L + SEGMENT - 1) / SEGMENT) : 1);
	const bool vec = aligned16(a.a) && aligned16(a.b) && a.a_stride % 4 == 0 && a.b_stride % 4 == 0;
	if (mfma && vec)
		product_kernel<WHICH, true, true, PART><<<grid, TPB, 0, s>>>(a);
	else if (mfma)
		product_kernel<WHICH, true, false, PART><<<grid, TPB, 0, s>>>(a);
	else if (vec)
		product_kernel<WHICH, false, true, PART><<<grid, TPB, 0, s>>>(a);
	else
		product_kernel<WHICH, false, false, PART><<<grid, TPB, 0, s>>>(a);
	return hipGetLastError();
}

bool product_ok(Product which, const ProductArgs& a)
{
	// a row of the output is a frame, a bin or a component: none of them goes beyond 16384
	if (!a.a || !a.b || !a.e || !a.out || a.I == 0 || a.J == 0 || a.L == 0 || a.I > MAX_FRAMES || a.J > MAX_FRAMES || a.L > MAX_FRAMES ||
	    a.e_stride < a.J || a.out_stride < a.J || (a.lam && a.lam_stride < a.J))
		return false;
	const size_t a_row = which == RATIO ? a.I : a.L, b_row = which == UPDATE_H ? a.L : a.J;
	return a.a_stride >= a_row && a.b_stride >= b_row && !(which == RATIO && a.L > SEGMENT) && !(which != RATIO && a.lam);
}

} // namespace

hipError_t launch_frame(const FrameArgs& a, hipStream_t s) { return zen_addon::launch_frame(a, s); }
hipError_t launch_magnitude(const MagArgs& a, hipStream_t s) { return zen_addon::launch_magnitude(a, s); }

hipError_t launch_product(Product which, const ProductArgs& a, bool mfma, hipStream_t s)
{
	if (!product_ok(which, a))
		return hipErrorInvalidValue;
	switch (which) {
	case RATIO:
		return launch_one<RATIO, false>(a, mfma, s);
	case UPDATE_H:
		return launch_one<UPDATE_H, false>(a, mfma, s);
	case UPDATE_W:
		return launch_one<UPDATE_W, false>(a, mfma, s);
	}
	return hipErrorInvalidValue;
}

hipError_t launch_product_split(Product which, const ProductArgs& a, bool mfma, hipStream_t s)
{
	if (!product_ok(which, a) || which == RATIO || !a.part || !a.part_rs)
		return hipErrorInvalidValue;
	const hipError_t e = which == UPDATE_H ? launch_one<UPDATE_H, true>(a, mfma, s) : launch_one<UPDATE_W, true>(a, mfma, s);
	if (e != hipSuccess)
		return e;
	const CombineArgs c = {a.part, a.part_rs, a.e, a.out, a.e_stride, a.out_stride, a.I, a.J, (a.L + SEGMENT - 1) / SEGMENT};
	combine_kernel<<<dim3((unsigned)((a.J + TPB - 1) / TPB), (unsigned)a.I, 1), TPB, 0, s>>>(c);
	return hipGetLastError();
}

hipError_t launch_stem_mask(const StemArgs& a, hipStream_t s)
{
	if (a.m == 0 || a.K < 1 || a.K > MAX_COMPONENTS)
		return hipErrorInvalidValue;
	stem_mask_kernel<<<dim3((unsigned)a.m, 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_overlap_add(const OlaArgs& a, hipStream_t s)
{
	if (a.n == 0)
		return hipSuccess;
	overlap_add_kernel<<<dim3((unsigned)((a.n + TPB - 1) / TPB), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace zen_nmf
