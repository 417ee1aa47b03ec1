// repet_kernels.hip -- the kernels of libzen_hip_repet.so (gfx950) around the public FFT call: frame (the windowed frames as
// complex rows), magnitude, lag_rows (V^2 transposed from time-major to bin-major rows through an LDS tile), power, braw (the
// beat spectrum summed over the bins), segment_median (the median over frames one period apart: the hot kernel), mask (the
// soft mask applied to a frame's spectrum in place) and overlap_add.
//
// The arithmetic is the contract of zen_hip_repet.h / DESIGN.md section 17, one IEEE float32 operation at a time (contraction
// off, hipcc's correctly rounded division and square root): tests/repet_model.py gives the same bits.  The one sum whose
// order the contract fixes (braw, over the bins) is added by one thread in that order.  A median is a selection: it is exact
// however it is found, so the two paths of segment_median (a sorting network in registers, a sort of lane-private columns in
// LDS) give the same values.  frame, magnitude, the body of mask and the sample of overlap_add are zen_amd/addon/stft_kernels.h's,
// the sorting network and the pick of the median zen_amd/addon/median_select.h's: shared with zen_amd/repsim and nmf.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../addon/median_select.h"
#include "../addon/stft_kernels.h"
#include "repet_kernels.h"

#pragma clang fp contract(off)

namespace zen_repet {
namespace {

using namespace zen_addon;

constexpr int TILE = 64; // lag_rows: frames x bins per workgroup

// ------------------------------------------------------------------------------------------------ lag rows
// A tile of TILE frames x TILE bins: read along the bins, written along the frames, through LDS (a row of TILE + 1 words
// keeps both sides off each other's banks).  The grid covers L frames: from m on the rows are zeros.
__global__ __launch_bounds__(TPB) void lag_rows_kernel(LagArgs k)
{
	__shared__ float tile[TILE][TILE + 1];
	const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x / TILE;
	const size_t k0 = (size_t)blockIdx.x * TILE;
	const int f0 = blockIdx.y * TILE;
	for (int kk = ty; kk < TILE; kk += TPB / TILE) {
		const size_t fr = k0 + kk;
		const int f = f0 + tx;
		tile[kk][tx] = fr < k.m && f < k.bins ? k.v[fr * k.v_stride + f] : 0.0f;
	}
	__syncthreads();
	float2* __restrict__ lag = reinterpret_cast<float2*>(k.lag);
	for (int ff = ty; ff < TILE; ff += TPB / TILE) {
		const int f = f0 + ff;
		const size_t fr = k0 + tx;
		if (f < k.bins && fr < k.L) {
			const float v = tile[tx][ff];
			lag[(size_t)f * k.L + fr] = make_float2(v * v, 0.0f);
		}
	}
}

__global__ __launch_bounds__(TPB) void power_kernel(PowerArgs k)
{
	float2* __restrict__ z = reinterpret_cast<float2*>(k.z);
	for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < k.count; i += (size_t)gridDim.x * TPB) {
		const float2 a = z[i];
		z[i] = make_float2(a.x * a.x + a.y * a.y, 0.0f);
	}
}

// one thread per lag walks the bins in order; neighbouring lags read neighbouring words
__global__ __launch_bounds__(TPB) void braw_kernel(BrawArgs k)
{
	const size_t j = (size_t)blockIdx.x * TPB + threadIdx.x;
	if (j >= k.m)
		return;
	const float2* __restrict__ lag = reinterpret_cast<const float2*>(k.lag);
	const float den = (float)(k.m - j);
	float acc = 0.0f;
	for (int f = 0; f < k.bins; ++f)
		acc = acc + lag[(size_t)f * k.L + j].x / den;
	k.braw[j] = acc;
}

// ------------------------------------------------------------------------------------------------ segment median
// counts up to P in registers.  A lane has VEC adjacent bins of one row l of the segment: every sweep q is a coalesced row
// read (16 bytes per lane for VEC = 4) and the VEC networks are independent of each other.  VEC = 4 wants v and s 16-byte
// aligned and both strides multiples of 4; the lanes at the end of a row fall back to single words.
// The loop is this kernel's own and not median_select.h's median_in_registers, which zen_amd/repsim's gathered rows go
// through: through that body the 32-row kernel took 163 registers for 138 and 0.0222 ms for 0.0200 ms on 7753 frames of 1025
// bins (profiles/stft_shared_ab.json).
template <int P, int VEC>
__global__ __launch_bounds__(TPB) void median_reg_kernel(MedianArgs k)
{
	const size_t f = ((size_t)blockIdx.x * 64 + (threadIdx.x & 63)) * VEC;
	const size_t l = (size_t)blockIdx.y * (TPB / 64) + threadIdx.x / 64;
	if (f >= k.bins || l >= k.period)
		return;
	float a[VEC][P];
	int c = 0;
	const bool whole = VEC == 1 || f + VEC <= k.bins;
#pragma unroll
	for (int q = 0; q < P; ++q) {
		const size_t fr = l + (size_t)q * k.period;
		const bool in = fr < k.m;
		c += in ? 1 : 0;
		if (VEC == 4 && whole) {
			float4 x = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
			if (in)
				x = *reinterpret_cast<const float4*>(k.v + fr * k.v_stride + f);
			a[0][q] = x.x;
			a[1 % VEC][q] = x.y;
			a[2 % VEC][q] = x.z;
			a[3 % VEC][q] = x.w;
		} else {
#pragma unroll
			for (int e = 0; e < VEC; ++e)
				a[e][q] = in && f + e < k.bins ? k.v[fr * k.v_stride + f + e] : INFINITY;
		}
	}
	float r[VEC];
#pragma unroll
	for (int e = 0; e < VEC; ++e) {
		sort_network<P>(a[e]);
		r[e] = pick_median<P>(a[e], c);
	}
	float* __restrict__ out = k.s + l * k.s_stride + f;
	if (VEC == 4 && whole) {
		*reinterpret_cast<float4*>(out) = make_float4(r[0], r[1 % VEC], r[2 % VEC], r[3 % VEC]);
	} else {
#pragma unroll
		for (int e = 0; e < VEC; ++e)
			if (f + e < k.bins)
				out[e] = r[e];
	}
}

// counts up to 256: a lane keeps its column in LDS (word q * 64 + lane: lane-private, every access of a wave on 64 different
// banks), padded with +inf to P = 64, 128 or 256, and sorts it there with the same bitonic network, pair by pair.  No lane
// reads another lane's words, so nothing is synchronised.  Dynamic LDS: P * 64 floats.
__global__ __launch_bounds__(64) void median_lds_kernel(MedianArgs k, int P)
{
	extern __shared__ float col[];
	const int lane = threadIdx.x;
	const size_t f = (size_t)blockIdx.x * 64 + lane, l = blockIdx.y;
	if (f >= k.bins || l >= k.period)
		return;
	int c = 0;
	for (int q = 0; q < P; ++q) {
		const size_t fr = l + (size_t)q * k.period;
		const bool in = fr < k.m;
		c += in ? 1 : 0;
		col[q * 64 + lane] = in ? k.v[fr * k.v_stride + f] : INFINITY;
	}
	for (int kk = 2; kk <= P; kk <<= 1) {
		for (int j = kk >> 1; j > 0; j >>= 1) {
			for (int t = 0; t < P / 2; ++t) {
				const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p2 = i | j; // the pairs (i, i ^ j) with i < i ^ j
				float x = col[i * 64 + lane], y = col[p2 * 64 + lane];
				if ((i & kk) == 0)
					cswap(x, y);
				else
					cswap(y, x);
				col[i * 64 + lane] = x;
				col[p2 * 64 + lane] = y;
			}
		}
	}
	const float slo = col[((c - 1) >> 1) * 64 + lane], shi = col[(c >> 1) * 64 + lane];
	k.s[l * k.s_stride + f] = (c & 1) ? slo : (slo + shi) * 0.5f;
}

template <int P>
hipError_t launch_reg(const MedianArgs& a, bool vec, hipStream_t s)
{
	const unsigned rows = (unsigned)((a.period + TPB / 64 - 1) / (TPB / 64));
	if (vec)
		median_reg_kernel<P, 4><<<dim3((unsigned)((a.bins + 255) / 256), rows, 1), TPB, 0, s>>>(a);
	else
		median_reg_kernel<P, 1><<<dim3((unsigned)((a.bins + 63) / 64), rows, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ mask
__global__ __launch_bounds__(TPB) void mask_kernel(MaskArgs k)
{
	const size_t fr = blockIdx.x;
	float2* __restrict__ row = reinterpret_cast<float2*>(k.rows) + fr * (size_t)k.N;
	const float* __restrict__ s = k.s + (fr % k.period) * k.v_stride; // the model of a frame is its row of the segment
	soft_mask_frame(row, k.v + fr * k.v_stride, s, k.N, k.kc);
}

// ------------------------------------------------------------------------------------------------ overlap-add
__global__ __launch_bounds__(TPB) void overlap_add_kernel(OlaArgs k)
{
	const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
	if (t >= k.n)
		return;
	const float x = k.in[t];
	float bg = 0.0f, fg = x;
	if (k.period) {
		bg = overlap_add_sample(k.rows, k.div, t, k.N);
		fg = x - bg;
	}
	if (k.background)
		k.background[t] = bg;
	if (k.foreground)
		k.foreground[t] = fg;
}

} // namespace

hipError_t launch_frame(const FrameArgs& a, hipStream_t s) { return zen_addon::launch_frame(a, s); }
hipError_t launch_magnitude(const MagArgs& a, hipStream_t s) { return zen_addon::launch_magnitude(a, s); }

hipError_t launch_lag_rows(const LagArgs& a, hipStream_t s)
{
	if (a.L % TILE || a.m > a.L || a.bins <= 0)
		return hipErrorInvalidValue;
	lag_rows_kernel<<<dim3((unsigned)(a.L / TILE), (unsigned)((a.bins + TILE - 1) / TILE), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_power(const PowerArgs& a, hipStream_t s)
{
	if (a.count == 0)
		return hipSuccess;
	const size_t blocks = (a.count + TPB - 1) / TPB;
	power_kernel<<<dim3((unsigned)(blocks < 65536 ? blocks : 65536), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_braw(const BrawArgs& a, hipStream_t s)
{
	if (a.m == 0 || a.m > a.L)
		return hipErrorInvalidValue;
	braw_kernel<<<dim3((unsigned)((a.m + TPB - 1) / TPB), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_segment_median(const MedianArgs& a, hipStream_t s)
{
	if (a.period == 0 || a.bins == 0 || a.period > 65535 * (size_t)(TPB / 64) || a.bins > ((size_t)1 << 30))
		return hipErrorInvalidValue;
	const size_t r = (a.m + a.period - 1) / a.period;
	if (r < 2 || r > MAX_SEGMENTS || a.v_stride < a.bins || a.s_stride < a.bins)
		return hipErrorInvalidValue;
	const bool vec = (((uintptr_t)a.v | (uintptr_t)a.s) & 15) == 0 && a.v_stride % 4 == 0 && a.s_stride % 4 == 0;
	if (r <= 2)
		return launch_reg<2>(a, vec, s);
	if (r <= 4)
		return launch_reg<4>(a, vec, s);
	if (r <= 8)
		return launch_reg<8>(a, vec, s);
	if (r <= 16)
		return launch_reg<16>(a, vec, s);
	if (r <= REGISTER_SEGMENTS)
		return launch_reg<REGISTER_SEGMENTS>(a, vec, s);
	const int P = r <= 64 ? 64 : r <= 128 ? 128 : 256;
	median_lds_kernel<<<dim3((unsigned)((a.bins + 63) / 64), (unsigned)a.period, 1), 64, sizeof(float) * 64 * P, s>>>(a, P);
	return hipGetLastError();
}

hipError_t launch_mask(const MaskArgs& a, hipStream_t s)
{
	if (a.m == 0 || a.period == 0)
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

} // namespace zen_repet
