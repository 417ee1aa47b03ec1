// resample_kernels.hip -- the two kernels of libzen_hip_resample.so: the expansion of the polyphase rows (once, at create) and
// the filter.  The arithmetic is the contract of zen_hip_resample.h: built with -ffp-contract=off and no fast-math flag, every
// float operation below is one IEEE float32 operation.
//
// fir: one workgroup makes a tile of TILE consecutive outputs of one row, one output per thread.  The workgroup's first output
// t0 has a0 = t0 den, i0 = a0 div num and rem0 = a0 mod num -- the one 64-bit division; thread k's position is
// rem0 + k den < 2^28 + 2^20, 32-bit arithmetic from there on.  The samples the tile needs, i0 - W + 1 up to the last thread's
// last tap, are staged once into LDS by coalesced loads, zeros where the row or the window of the call ends, and every
// thread runs its eight chains from there against its coefficient row, read in 16-byte pieces.
#include "resample_kernels.h"

namespace zen_resample {
namespace {

// (p, mu) of a remainder: f = (rem 2^32) div num by long division in 32 bits (rem < num <= 2^20: 12, 12 and 8 bits of the
// quotient), p = f >> 23, mu = float32(f & 0x7FFFFF) 2^-23
__device__ __forceinline__ void phase_of(uint32_t rem, uint32_t num, uint32_t& p, float& mu)
{
	uint32_t r = rem << 12;
	uint32_t q = r / num;
	r -= q * num;
	r <<= 12;
	uint32_t d = r / num;
	r -= d * num;
	q = (q << 12) | d;
	r <<= 8;
	q = (q << 8) | (r / num);
	p = q >> 23;
	mu = (float)(q & 0x7FFFFFu) * 0x1p-23f;
}

__device__ __forceinline__ float lerp3(float h0, float h1, float mu)
{
	const float diff = h1 - h0;
	const float step = mu * diff;
	return h0 + step;
}

__global__ __launch_bounds__(TILE) void expand_kernel(ExpandArgs a)
{
	const uint32_t idx = blockIdx.x * TILE + threadIdx.x;
	const uint32_t rem = idx / (uint32_t)a.Tp, j = idx - rem * (uint32_t)a.Tp;
	if (rem >= a.num)
		return;
	uint32_t p;
	float mu;
	phase_of(rem, a.num, p, mu);
	const float* h0 = a.table + (size_t)p * a.Tp;
	a.poly[idx] = lerp3(h0[j], h0[a.Tp + j], mu);
}

template <bool POLY>
__global__ __launch_bounds__(TILE) void fir_kernel(FirArgs a)
{
	__shared__ float xs[STAGE];
	const uint32_t tid = threadIdx.x;
	const uint64_t k0 = (uint64_t)blockIdx.x * TILE; // the tile's first output within the call
	const uint64_t left = a.out_count - k0;
	const uint32_t cnt = left < (uint64_t)TILE ? (uint32_t)left : (uint32_t)TILE;
	const uint64_t a0 = (a.out_first + k0) * a.den;
	const uint64_t i0 = a0 / a.num;
	const uint32_t rem0 = (uint32_t)(a0 - i0 * a.num);
	// what the tile reads of LDS: the last thread's offset plus a padded row of taps
	const uint32_t taps = 2u * (uint32_t)a.W;
	const uint32_t last_off = (rem0 + (cnt - 1) * a.den) / a.num;
	const uint32_t filled = last_off + taps, staged = last_off + (uint32_t)a.Tp;
	const int64_t base = (int64_t)i0 - a.W + 1;      // the virtual index of xs[0]
	const float* __restrict__ in_row = a.in + (uint64_t)blockIdx.y * a.in_stride;
	for (uint32_t s = tid; s < staged; s += TILE) {
		const int64_t g = base + (int64_t)s;
		float v = 0.0f;
		if (s < filled && g >= 0 && (uint64_t)g < a.n_total && (uint64_t)g >= a.in_first && (uint64_t)g - a.in_first < a.in_count)
			v = in_row[(uint64_t)g - a.in_first];
		xs[s] = v;
	}
	__syncthreads();
	if (tid >= cnt)
		return;
	const uint32_t ak = rem0 + tid * a.den;
	const uint32_t off = ak / a.num, rem = ak - off * a.num;
	const float* x = xs + off;
	const float4* __restrict__ c0;
	const float4* __restrict__ c1 = nullptr;
	float mu = 0.0f;
	if (POLY) {
		c0 = reinterpret_cast<const float4*>(a.coef + (size_t)rem * a.Tp);
	} else {
		uint32_t p;
		phase_of(rem, a.num, p, mu);
		c0 = reinterpret_cast<const float4*>(a.coef + (size_t)p * a.Tp); // rows p and p + 1: one run of 2 Tp floats
		c1 = c0 + a.Tp / 4;
	}
	float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, s4 = 0.0f, s5 = 0.0f, s6 = 0.0f, s7 = 0.0f;
	const int groups = a.Tp / 8;
	for (int g = 0; g < groups; ++g) {
		float4 lo = c0[2 * g], hi = c0[2 * g + 1];
		if (!POLY) {
			const float4 lo1 = c1[2 * g], hi1 = c1[2 * g + 1];
			lo = make_float4(lerp3(lo.x, lo1.x, mu), lerp3(lo.y, lo1.y, mu), lerp3(lo.z, lo1.z, mu), lerp3(lo.w, lo1.w, mu));
			hi = make_float4(lerp3(hi.x, hi1.x, mu), lerp3(hi.y, hi1.y, mu), lerp3(hi.z, hi1.z, mu), lerp3(hi.w, hi1.w, mu));
		}
		const float* xg = x + 8 * g;
		const float p0 = xg[0] * lo.x, p1 = xg[1] * lo.y, p2 = xg[2] * lo.z, p3 = xg[3] * lo.w;
		const float p4 = xg[4] * hi.x, p5 = xg[5] * hi.y, p6 = xg[6] * hi.z, p7 = xg[7] * hi.w;
		s0 = s0 + p0;
		s1 = s1 + p1;
		s2 = s2 + p2;
		s3 = s3 + p3;
		s4 = s4 + p4;
		s5 = s5 + p5;
		s6 = s6 + p6;
		s7 = s7 + p7;
	}
	a.out[(uint64_t)blockIdx.y * a.out_stride + k0 + tid] = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
}

} // namespace

hipError_t launch_expand(const ExpandArgs& a, hipStream_t s)
{
	const uint32_t items = a.num * (uint32_t)a.Tp; // at most 4096 * 256
	expand_kernel<<<dim3((items + TILE - 1) / TILE, 1, 1), TILE, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_fir(const FirArgs& a, hipStream_t s)
{
	const dim3 grid(a.tiles, a.n_rows, 1);
	if (a.poly)
		fir_kernel<true><<<grid, TILE, 0, s>>>(a);
	else
		fir_kernel<false><<<grid, TILE, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace zen_resample
