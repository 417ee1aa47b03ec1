// cqt_kernels.hip -- the kernels of libzen_hip_cqt.so (gfx950) around the public FFT and median calls: slice (the windowed
// slices as complex rows), fold (the bins of every band at their absolute index mod M, zeros included), overlap (the halves of
// neighbouring slices added, the magnitude, band-major rows turned into the time-major matrix through an LDS tile), mask (the
// stem's mask from H and P, turned back through an LDS tile and applied to a run of slices), gather (Y_q from at most two
// transformed rows per bin, with its mirrored half) and overlap_add.
//
// The arithmetic is the contract of zen_hip_cqt.h / DESIGN.md section 18, one IEEE float32 operation at a time (contraction
// off, hipcc's correctly rounded division and square root): tests/cqt_model.py gives the same bits.  Every sum of the contract
// has two terms and a stated order, so no kernel reduces anything.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "cqt_kernels.h"

#pragma clang fp contract(off)

namespace zen_cqt {
namespace {

constexpr int TPB = 256;
constexpr int TILE = 32; // overlap, mask: columns of time x bands per workgroup

unsigned grid_rows(size_t rows) { return (unsigned)(rows < 65535 ? rows : 65535); }

// ------------------------------------------------------------------------------------------------ slice
// xp is N zeros, the clip, zeros: sample j of slice q is x[q N - N + j].  A workgroup has SLICE_CHUNK samples of one slice.
constexpr int SLICE_CHUNK = 4 * TPB;

__global__ __launch_bounds__(TPB) void slice_kernel(SliceArgs k)
{
	const int Ls = k.Ls, N = Ls / 2, chunks = (Ls + SLICE_CHUNK - 1) / SLICE_CHUNK;
	const size_t q = blockIdx.x / chunks;
	const int j0 = (int)(blockIdx.x % chunks) * SLICE_CHUNK, j1 = j0 + SLICE_CHUNK < Ls ? j0 + SLICE_CHUNK : Ls;
	for (size_t c = blockIdx.y; c < k.n_clips; c += gridDim.y) {
		const float* __restrict__ x = k.in + c * k.in_stride;
		float2* __restrict__ row = reinterpret_cast<float2*>(k.rows) + (c * k.ns + q) * (size_t)Ls;
		for (int j = j0 + threadIdx.x; j < j1; j += TPB) {
			const size_t pos = q * (size_t)N + (size_t)j; // index into xp
			const float v = pos >= (size_t)N && pos - N < k.n ? x[pos - N] : 0.0f;
			row[j] = make_float2(v * k.h[j], 0.0f);
		}
	}
}

// ------------------------------------------------------------------------------------------------ fold
// One thread per coefficient (k, j): band k holds the bins lo..hi, fewer than M + 1 of them, so at most one has b mod M == j.
// Neighbouring j are neighbouring bins (but for the one wrap of a band): the reads of the half spectrum and the writes of the
// rows are both along the fast axis, and the entries no bin lands on are written as +0 here.
__global__ __launch_bounds__(TPB) void fold_kernel(FoldArgs k)
{
	const int M = k.M, N = k.Ls / 2;
	const size_t e = (size_t)blockIdx.x * TPB + threadIdx.x;
	if (e >= (size_t)k.nb * M)
		return;
	const int band = (int)(e / (size_t)M), j = (int)(e % (size_t)M);
	const int centre = k.t.centres[band];
	const int lo = band ? k.t.centres[band - 1] + 1 : 0, hi = band < k.nb - 1 ? k.t.centres[band + 1] - 1 : N;
	const int b = lo + ((j - lo) & (M - 1));
	const bool in = b <= hi;
	const float g = in ? (b >= centre ? k.t.gL[b] : k.t.gU[b]) : 0.0f;
	for (size_t r = blockIdx.y; r < k.n_rows; r += gridDim.y) {
		float2 z = make_float2(0.0f, 0.0f);
		if (in) {
			const float2 f = reinterpret_cast<const float2*>(k.rows)[r * (size_t)k.Ls + b];
			z = make_float2(f.x * g, f.y * g);
		}
		reinterpret_cast<float2*>(k.coef)[r * (size_t)k.nb * M + e] = z;
	}
}

// ------------------------------------------------------------------------------------------------ overlap
// A tile of TILE columns of time x TILE bands: read along time (the fast axis of a coefficient row), written along the bands
// (the fast axis of V), through LDS (a row of TILE + 1 words keeps both sides off each other's banks).
__global__ __launch_bounds__(TPB) void overlap_kernel(OverlapArgs k)
{
	__shared__ float tile[TILE][TILE + 1];
	const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x / TILE;
	const int M = k.M, half = M / 2;
	const size_t T = (k.ns + 1) * (size_t)half, t0 = (size_t)blockIdx.x * TILE;
	const int k0 = blockIdx.y * TILE;
	const float2* __restrict__ c = reinterpret_cast<const float2*>(k.coef);
	{
		const size_t t = t0 + tx, q = t / half;
		const int m = (int)(t % half);
		for (int kk = ty; kk < TILE; kk += TPB / TILE) {
			const int band = k0 + kk;
			float v = 0.0f;
			if (t < T && band < k.nb) {
				float2 a;
				if (q == 0) {
					a = c[(size_t)band * M + m];
				} else if (q == k.ns) {
					a = c[((q - 1) * k.nb + band) * (size_t)M + m + half];
				} else {
					const float2 e = c[((q - 1) * k.nb + band) * (size_t)M + m + half], l = c[(q * k.nb + band) * (size_t)M + m];
					a = make_float2(e.x + l.x, e.y + l.y); // the earlier slice first
				}
				v = sqrtf(a.x * a.x + a.y * a.y);
			}
			tile[kk][tx] = v;
		}
	}
	__syncthreads();
	for (int tt = ty; tt < TILE; tt += TPB / TILE) {
		const size_t t = t0 + tt;
		const int band = k0 + tx;
		if (t < T && band < k.nb)
			k.v[t * k.v_stride + band] = tile[tx][tt];
	}
}

// ------------------------------------------------------------------------------------------------ mask
__device__ __forceinline__ float stem_mask(float H, float P, float beta, int stem, int soft)
{
	if (soft) {
		const float hh = H * H, pp = P * P, d = hh + pp;
		if (!(d > 0.0f))
			return 0.0f;
		return stem == STEM_HARMONIC ? hh / d : pp / d;
	}
	const bool harm = H > beta * P;
	const bool perc = !harm && P >= beta * H;
	const bool on = stem == STEM_HARMONIC ? harm : stem == STEM_PERCUSSIVE ? perc : (!harm && !perc);
	return on ? 1.0f : 0.0f;
}

// A tile of TILE columns x TILE bands of one slice: H and P are read along the bands, the mask goes through LDS, and the
// coefficients are read and written along time.  Column m of slice q is row q M / 2 + m of the matrices.
__global__ __launch_bounds__(TPB) void mask_kernel(MaskArgs k)
{
	__shared__ float tile[TILE][TILE + 1];
	const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x / TILE;
	const int M = k.M, half = M / 2;
	const int m0 = blockIdx.x * TILE, k0 = blockIdx.y * TILE;
	const size_t q = k.q0 + blockIdx.z;
	for (int tt = ty; tt < TILE; tt += TPB / TILE) {
		const size_t t = q * half + m0 + tt; // below T: m0 + tt < M
		const int band = k0 + tx;
		float w = 0.0f;
		if (band < k.nb)
			w = stem_mask(k.hm[t * k.nb + band], k.pm[t * k.nb + band], k.beta, k.stem, k.soft);
		tile[tt][tx] = w;
	}
	__syncthreads();
	const float2* __restrict__ src = reinterpret_cast<const float2*>(k.coef) + q * k.nb * (size_t)M;
	float2* __restrict__ dst = reinterpret_cast<float2*>(k.out) + (size_t)blockIdx.z * k.nb * (size_t)M;
	for (int kk = ty; kk < TILE; kk += TPB / TILE) {
		const int band = k0 + kk;
		if (band < k.nb) {
			const float w = tile[tx][kk];
			const float2 z = src[(size_t)band * M + m0 + tx];
			dst[(size_t)band * M + m0 + tx] = make_float2(z.x * w, z.y * w);
		}
	}
}

// ------------------------------------------------------------------------------------------------ gather
// one thread per bin b <= N of one slice: at most two transformed rows meet there; it writes bin Ls - b as well
__global__ __launch_bounds__(TPB) void gather_kernel(GatherArgs k)
{
	const int Ls = k.Ls, N = Ls / 2, M = k.M;
	const int b = blockIdx.x * TPB + threadIdx.x;
	if (b > N)
		return;
	const int band = k.t.kb[b], j = b & (M - 1);
	const bool centre = k.t.centres[band] == b;
	const float gdl = k.t.gdL[b], gdu = k.t.gdU[b];
	for (size_t r = blockIdx.y; r < k.run; r += gridDim.y) {
		const float2* __restrict__ g = reinterpret_cast<const float2*>(k.g) + (r * k.nb + band) * (size_t)M;
		const float2 lo = g[j];
		float2 y = make_float2(lo.x * gdl, lo.y * gdl);
		if (!centre) {
			const float2 up = g[M + j]; // band + 1
			y = make_float2(y.x + up.x * gdu, y.y + up.y * gdu); // the lower band first
		}
		if (b == 0 || b == N)
			y.y = 0.0f;
		float2* __restrict__ row = reinterpret_cast<float2*>(k.rows) + (k.q0 + r) * (size_t)Ls;
		row[b] = y;
		if (b > 0 && b < N)
			row[Ls - b] = make_float2(y.x, -y.y);
	}
}

// ------------------------------------------------------------------------------------------------ overlap-add
__device__ __forceinline__ float ola_at(const float2* __restrict__ y, const float* __restrict__ s, size_t t, int N)
{
	const size_t q = t / N;
	const int i = (int)(t % N);
	return y[q * 2 * N + N + i].x * s[N + i] + y[(q + 1) * 2 * N + i].x * s[i]; // the earlier slice first
}

// VEC = 4: four samples per thread and one 16-byte store where all four are inside the clip; wants every row of out 16-byte
// aligned.  The values are those of VEC = 1.
template <int VEC>
__global__ __launch_bounds__(TPB) void overlap_add_kernel(OlaArgs k)
{
	const int N = k.Ls / 2;
	const size_t t = ((size_t)blockIdx.x * TPB + threadIdx.x) * VEC;
	if (t >= k.n)
		return;
	for (size_t c = blockIdx.y; c < k.n_clips; c += gridDim.y) {
		const float2* __restrict__ y = reinterpret_cast<const float2*>(k.rows) + c * k.ns * (size_t)k.Ls;
		float* __restrict__ out = k.out + c * k.out_stride + t;
		if (VEC == 4 && t + 4 <= k.n) {
			*reinterpret_cast<float4*>(out) = make_float4(ola_at(y, k.s, t, N), ola_at(y, k.s, t + 1, N), ola_at(y, k.s, t + 2, N), ola_at(y, k.s, t + 3, N));
		} else {
#pragma unroll
			for (int e = 0; e < VEC; ++e)
				if (t + e < k.n)
					out[e] = ola_at(y, k.s, t + e, N);
		}
	}
}

} // namespace

hipError_t launch_slice(const SliceArgs& a, hipStream_t s)
{
	if (a.ns == 0 || a.n_clips == 0)
		return hipSuccess;
	slice_kernel<<<dim3((unsigned)(a.ns * (size_t)((a.Ls + SLICE_CHUNK - 1) / SLICE_CHUNK)), grid_rows(a.n_clips), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_fold(const FoldArgs& a, hipStream_t s)
{
	if (a.n_rows == 0)
		return hipSuccess;
	if (a.nb < 3 || a.M < TILE || (a.M & (a.M - 1)))
		return hipErrorInvalidValue;
	fold_kernel<<<dim3((unsigned)(((size_t)a.nb * a.M + TPB - 1) / TPB), grid_rows(a.n_rows), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_overlap(const OverlapArgs& a, hipStream_t s)
{
	if (a.ns == 0 || a.nb <= 0 || a.M < TILE || a.v_stride < (size_t)a.nb)
		return hipErrorInvalidValue;
	const size_t T = (a.ns + 1) * (size_t)(a.M / 2);
	overlap_kernel<<<dim3((unsigned)((T + TILE - 1) / TILE), (unsigned)((a.nb + TILE - 1) / TILE), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_mask(const MaskArgs& a, hipStream_t s)
{
	if (a.run == 0)
		return hipSuccess;
	if (a.run > 65535 || a.nb <= 0 || a.M < TILE || a.M % TILE)
		return hipErrorInvalidValue;
	mask_kernel<<<dim3((unsigned)(a.M / TILE), (unsigned)((a.nb + TILE - 1) / TILE), (unsigned)a.run), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_gather(const GatherArgs& a, hipStream_t s)
{
	if (a.run == 0)
		return hipSuccess;
	gather_kernel<<<dim3((unsigned)((a.Ls / 2 + 1 + TPB - 1) / TPB), grid_rows(a.run), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_overlap_add(const OlaArgs& a, hipStream_t s)
{
	if (a.n == 0 || a.n_clips == 0)
		return hipSuccess;
	const bool vec = ((uintptr_t)a.out & 15) == 0 && (a.n_clips == 1 || a.out_stride % 4 == 0);
	if (vec)
		overlap_add_kernel<4><<<dim3((unsigned)((a.n + 4 * TPB - 1) / (4 * TPB)), grid_rows(a.n_clips), 1), TPB, 0, s>>>(a);
	else
		overlap_add_kernel<1><<<dim3((unsigned)((a.n + TPB - 1) / TPB), grid_rows(a.n_clips), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace zen_cqt
