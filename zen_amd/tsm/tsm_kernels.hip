// tsm_kernels.hip -- the kernels of libzen_hip_tsm.so (gfx950) around the public FFT call: frame (the windowed frames at their
// analysis positions as complex rows), analysis (magnitude and phase), peaks (peak flags as ballot words in LDS, the nearest
// peak of every bin by bit scans, and everything of the phase recurrence that does not depend on the frame before), walk (the
// recurrence itself: one workgroup per clip), spectrum (the synthesis spectrum from magnitude and phase), output (the two
// overlap-add gathers and their sum), and the two table functions alone (phase, cs).
//
// The arithmetic is the contract of zen_hip_tsm.h / DESIGN.md section 21, one IEEE float32 operation at a time (contraction
// off, hipcc's correctly rounded division and square root, rintf for the rounding to nearest even): tests/tsm_model.py gives
// the same bits.  Phases are u32 fractions of a turn; their sums wrap, so the walk may add them in any grouping.  The analysis
// positions are one correctly rounded double division per frame, the host's.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "tsm_kernels.h"

#pragma clang fp contract(off)

namespace zen_tsm {
namespace {

constexpr int TPB = 256;
constexpr int WALK_TPB = 1024;
constexpr int WALK_ITEMS = 5; // 4097 bins of the largest frame over 1024 threads
constexpr int WALK_DEPTH = 4; // frames whose owner and e words a thread holds ahead of the recurrence

__device__ uint32_t g_atan[ATAN_STEPS + 1];
__device__ float2 g_coarse[COARSE];
__device__ float2 g_fine[FINE];
__device__ float g_consts[2]; // c3, K

unsigned grid_rows(size_t n) { return (unsigned)(n < 65535 ? n : 65535); }

__device__ __forceinline__ long long position(long long m, const Framing& f)
{
	return (long long)floor((double)((m - f.V / 2 + 1) * (long long)f.Hs) / f.alpha);
}

__device__ __forceinline__ uint32_t atan2turns(float y, float x)
{
	const float ax = fabsf(x), ay = fabsf(y);
	if (ax == 0.0f && ay == 0.0f)
		return 0u;
	const float hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
	const float q = lo / hi;
	const float fi = rintf(q * 256.0f);
	const int i = (int)fi;
	const float qi = fi / 256.0f;
	const float t = (q - qi) / (1.0f + q * qi);
	const float s = t * t;
	const float u = t - (t * s) * g_consts[0];
	const int r = (int)rintf(u * g_consts[1]);
	uint32_t phi = g_atan[i] + (uint32_t)r;
	if (ay > ax)
		phi = 0x40000000u - phi;
	if (x < 0.0f)
		phi = 0x80000000u - phi;
	if (y < 0.0f)
		phi = 0u - phi;
	return phi;
}

__device__ __forceinline__ float2 cos_sin(uint32_t psi)
{
	const float2 a = g_coarse[psi >> 21], b = g_fine[(psi >> 10) & (FINE - 1)];
	return make_float2(a.x * b.x - a.y * b.y, a.y * b.x + a.x * b.y);
}

// ------------------------------------------------------------------------------------------------ frame
__global__ __launch_bounds__(TPB) void frame_kernel(FrameArgs k)
{
	const int N = k.fr.N;
	const size_t m = blockIdx.x;
	const long long first = position((long long)m, k.fr) - N / 2;
	for (size_t c = blockIdx.y; c < k.n_clips; c += gridDim.y) {
		const float* __restrict__ x = k.in + c * k.in_stride;
		float2* __restrict__ row = reinterpret_cast<float2*>(k.rows) + (c * k.M + m) * (size_t)N;
		for (int i = threadIdx.x; i < N; i += TPB) {
			const long long pos = first + i;
			const float v = pos >= 0 && pos < (long long)k.n ? x[pos] : 0.0f;
			row[i] = make_float2(v * k.win[i], 0.0f);
		}
	}
}

// ------------------------------------------------------------------------------------------------ analysis
__global__ __launch_bounds__(TPB) void analysis_kernel(AnalysisArgs k)
{
	const int N = k.N, H = N / 2;
	for (size_t f = blockIdx.x; f < k.frames; f += gridDim.x) {
		const float2* __restrict__ row = reinterpret_cast<const float2*>(k.rows) + f * (size_t)N;
		for (size_t i = threadIdx.x; i < k.stride; i += TPB) {
			float mg = 0.0f;
			uint32_t th = 0u;
			if (i <= (size_t)H) {
				const float2 z = row[i];
				mg = sqrtf(z.x * z.x + z.y * z.y);
				th = atan2turns(z.y, z.x);
			}
			k.mag[f * k.stride + i] = mg;
			k.theta[f * k.stride + i] = th;
		}
	}
}

// ------------------------------------------------------------------------------------------------ peaks
// One workgroup per frame.  The magnitudes of the row go to LDS; every wave turns 64 bins at a time into one ballot word of
// peak flags; the nearest peak below and above a bin is the highest set bit at or below it and the lowest at or above it,
// found a word at a time.  Then own and e, which need theta of this frame and of the one before at the owner only.
constexpr int MAX_BINS = 4097;
constexpr int MAX_WORDS = (MAX_BINS + 63) / 64;

__global__ __launch_bounds__(TPB) void peaks_kernel(PeakArgs k)
{
	__shared__ float smag[MAX_BINS + 3];
	__shared__ unsigned long long words[MAX_WORDS];
	const int N = k.fr.N, H = N / 2, bins = H + 1, nwords = (bins + 63) / 64;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (size_t f = blockIdx.x; f < k.frames; f += gridDim.x) {
		const size_t m = f % k.M;
		const float* __restrict__ mag = k.mag + f * k.stride;
		const uint32_t* __restrict__ th = k.theta + f * k.stride;
		__syncthreads(); // the frame before is done with LDS
		for (int i = threadIdx.x; i < bins; i += TPB)
			smag[i] = mag[i];
		__syncthreads();
		for (int w = wave; w < nwords; w += TPB / 64) { // uniform per wave: every lane takes part in the ballot
			const int b = w * 64 + lane;
			bool pk = b < bins;
			if (pk) {
				const float v = smag[b];
				pk = (b - 2 < 0 || v > smag[b - 2]) && (b - 1 < 0 || v > smag[b - 1]) && (b + 1 > H || v > smag[b + 1]) && (b + 2 > H || v > smag[b + 2]);
			}
			const unsigned long long word = __ballot(pk);
			if (lane == 0)
				words[w] = word;
		}
		__syncthreads();
		unsigned long long any = 0;
		for (int w = 0; w < nwords; ++w)
			any |= words[w];
		long long Ha = 1;
		if (m > 0)
			Ha = position((long long)m, k.fr) - position((long long)m - 1, k.fr);
		const uint32_t unit = (uint32_t)(0x100000000ull / (unsigned long long)N); // 2^32 / N
		for (int b = threadIdx.x; b < bins; b += TPB) {
			int own = b;
			if (any) {
				int wi = b >> 6;
				unsigned long long w = words[wi] & (~0ull >> (63 - (b & 63)));
				while (w == 0 && wi > 0)
					w = words[--wi];
				const int lo = w ? wi * 64 + 63 - __clzll((long long)w) : -1;
				wi = b >> 6;
				w = words[wi] & (~0ull << (b & 63));
				while (w == 0 && wi < nwords - 1)
					w = words[++wi];
				const int hi = w ? wi * 64 + __ffsll((unsigned long long)w) - 1 : -1;
				own = lo < 0 ? hi : hi < 0 ? lo : (b - lo <= hi - b ? lo : hi);
			}
			const uint32_t tb = th[b];
			uint32_t e = tb;
			if (m > 0) {
				const uint32_t tp = th[own], before = (th - k.stride)[own];
				const int32_t delta = (int32_t)(tp - before - (uint32_t)own * (uint32_t)Ha * unit);
				const uint32_t inc = (uint32_t)own * (uint32_t)k.fr.Hs * unit + (uint32_t)((long long)delta * (long long)k.fr.Hs / Ha);
				e = inc + tb - tp;
			}
			k.owner[f * k.stride + b] = (uint16_t)own;
			k.e[f * k.stride + b] = e;
		}
	}
}

// ------------------------------------------------------------------------------------------------ walk
// One workgroup per clip: two psi rows in LDS; per frame one LDS gather, one add, one barrier.  The owner and e words do not
// depend on the recurrence: a thread keeps those of the next WALK_DEPTH frames in registers, and the loads of frame m +
// WALK_DEPTH are issued ahead of frame m's barrier (every load has a valid address -- bin and frame are clamped -- so none of
// them hangs on a condition and each goes straight into its register).  The row written in frame m was last read in frame
// m - 1, before that frame's barrier, so one barrier per frame is enough.  ITEMS: the bins of a thread.
template <int ITEMS>
__global__ __launch_bounds__(WALK_TPB) void walk_kernel(WalkArgs k)
{
	extern __shared__ __attribute__((aligned(16))) uint32_t psi_rows[]; // 2 * stride words
	const int bins = k.bins, tpb = blockDim.x;
	const size_t S = k.stride, last = k.M - 1;
	int bin[ITEMS];
#pragma unroll
	for (int j = 0; j < ITEMS; ++j) {
		const int b = threadIdx.x + j * tpb;
		bin[j] = b < bins ? b : bins - 1;
	}
	for (size_t c = blockIdx.x; c < k.n_clips; c += gridDim.x) {
		const uint16_t* __restrict__ owner = k.owner + c * k.M * S;
		const uint32_t* __restrict__ e = k.e + c * k.M * S;
		uint32_t* __restrict__ psi = k.psi + c * k.M * S;
		__syncthreads();
		for (size_t i = threadIdx.x; i < 2 * S; i += tpb)
			psi_rows[i] = 0u;
		uint32_t own_q[WALK_DEPTH][ITEMS], e_q[WALK_DEPTH][ITEMS];
#pragma unroll
		for (int d = 0; d < WALK_DEPTH; ++d) {
			const size_t mm = (size_t)d < k.M ? (size_t)d : last;
#pragma unroll
			for (int j = 0; j < ITEMS; ++j) {
				own_q[d][j] = owner[mm * S + bin[j]];
				e_q[d][j] = e[mm * S + bin[j]];
			}
		}
		__syncthreads();
		// frame m with the words of slot d, then the loads of frame m + WALK_DEPTH into that slot, then the barrier
		const auto step = [&](size_t m, int d) {
			const uint32_t* before = psi_rows + (m & 1) * S;
			uint32_t* now = psi_rows + ((m + 1) & 1) * S;
#pragma unroll
			for (int j = 0; j < ITEMS; ++j) {
				const int b = threadIdx.x + j * tpb;
				if (b < bins) {
					const uint32_t v = before[own_q[d][j]] + e_q[d][j];
					now[b] = v;
					psi[m * S + b] = v;
				}
			}
			const size_t mm = m + WALK_DEPTH < k.M ? m + WALK_DEPTH : last;
#pragma unroll
			for (int j = 0; j < ITEMS; ++j) {
				own_q[d][j] = owner[mm * S + bin[j]];
				e_q[d][j] = e[mm * S + bin[j]];
			}
			__syncthreads();
		};
		size_t m = 0;
		for (; m + WALK_DEPTH <= k.M; m += WALK_DEPTH) { // whole groups: straight-line code, the slots are constants
#pragma unroll
			for (int d = 0; d < WALK_DEPTH; ++d)
				step(m + d, d);
		}
#pragma unroll
		for (int d = 0; d < WALK_DEPTH - 1; ++d)
			if (m + d < k.M)
				step(m + d, d);
	}
}

// ------------------------------------------------------------------------------------------------ spectrum
__global__ __launch_bounds__(TPB) void spectrum_kernel(SpectrumArgs k)
{
	const int N = k.N, H = N / 2;
	for (size_t f = blockIdx.x; f < k.frames; f += gridDim.x) {
		float2* __restrict__ row = reinterpret_cast<float2*>(k.rows) + f * (size_t)N;
		for (int b = threadIdx.x; b <= H; b += TPB) {
			const float mg = k.mag[f * k.stride + b];
			const float2 cs = cos_sin(k.psi[f * k.stride + b]);
			const float2 y = make_float2(mg * cs.x, mg * cs.y);
			row[b] = y;
			if (b > 0 && b < H)
				row[N - b] = make_float2(y.x, -y.y);
		}
	}
}

// ------------------------------------------------------------------------------------------------ output
__device__ __forceinline__ float stem_at(const OutputArgs& k, size_t c, long long pos)
{
	if (pos < 0 || pos >= (long long)k.n)
		return 0.0f;
	const float p = k.perc[c * k.in_stride + pos];
	return k.resid ? p + k.resid[c * k.in_stride + pos] : p;
}

__global__ __launch_bounds__(TPB) void output_kernel(OutputArgs k)
{
	const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
	if (t >= k.n_out)
		return;
	for (size_t c = blockIdx.y; c < k.n_clips; c += gridDim.y) {
		float pv = 0.0f, ola = 0.0f;
		if (k.rows) {
			const int N = k.N, Hs = N / 4;
			const size_t q = t / Hs;
			const int i = (int)(t % Hs);
			const float2* __restrict__ g = reinterpret_cast<const float2*>(k.rows) + (c * k.M + q) * (size_t)N;
			float acc = g[i + 3 * Hs].x * k.win[i + 3 * Hs];
#pragma unroll
			for (int j = 1; j < 4; ++j)
				acc = acc + g[(size_t)j * N + i + (3 - j) * Hs].x * k.win[i + (3 - j) * Hs];
			pv = acc / k.div[i];
		}
		if (k.perc) {
			const int Hs = k.ola.Hs;
			const long long q = (long long)(t / Hs);
			const int i = (int)(t % Hs);
			const float f0 = stem_at(k, c, position(q, k.ola) + i) * k.win_ola[i + Hs];
			const float f1 = stem_at(k, c, position(q + 1, k.ola) - Hs + i) * k.win_ola[i];
			ola = (f0 + f1) / k.div_ola[i];
		}
		k.out[c * k.out_stride + t] = k.rows && k.perc ? pv + ola : k.rows ? pv : ola;
	}
}

// ------------------------------------------------------------------------------------------------ the table functions alone
// the caller's pointers are 4-byte aligned only: single words
__global__ __launch_bounds__(TPB) void phase_kernel(const float* __restrict__ z, size_t count, uint32_t* __restrict__ theta)
{
	for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < count; i += (size_t)gridDim.x * TPB)
		theta[i] = atan2turns(z[2 * i + 1], z[2 * i]);
}

__global__ __launch_bounds__(TPB) void cs_kernel(const uint32_t* __restrict__ psi, size_t count, float* __restrict__ out)
{
	for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < count; i += (size_t)gridDim.x * TPB) {
		const float2 v = cos_sin(psi[i]);
		out[2 * i] = v.x;
		out[2 * i + 1] = v.y;
	}
}

unsigned flat_grid(size_t count)
{
	const size_t blocks = (count + TPB - 1) / TPB;
	return (unsigned)(blocks < 65536 ? blocks : 65536);
}

} // namespace

hipError_t upload_tables(const uint32_t* atan_t, const float* coarse, const float* fine, float c3, float k)
{
	const float consts[2] = {c3, k};
	hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_atan), atan_t, sizeof(uint32_t) * (ATAN_STEPS + 1));
	if (e == hipSuccess)
		e = hipMemcpyToSymbol(HIP_SYMBOL(g_coarse), coarse, sizeof(float2) * COARSE);
	if (e == hipSuccess)
		e = hipMemcpyToSymbol(HIP_SYMBOL(g_fine), fine, sizeof(float2) * FINE);
	if (e == hipSuccess)
		e = hipMemcpyToSymbol(HIP_SYMBOL(g_consts), consts, sizeof(consts));
	return e;
}

hipError_t launch_frame(const FrameArgs& a, hipStream_t s)
{
	if (a.M == 0 || a.n_clips == 0)
		return hipSuccess;
	frame_kernel<<<dim3((unsigned)a.M, grid_rows(a.n_clips), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_analysis(const AnalysisArgs& a, hipStream_t s)
{
	if (a.frames == 0)
		return hipSuccess;
	analysis_kernel<<<dim3((unsigned)(a.frames < (1u << 20) ? a.frames : (1u << 20)), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_peaks(const PeakArgs& a, hipStream_t s)
{
	if (a.frames == 0)
		return hipSuccess;
	if (a.fr.N / 2 + 1 > MAX_BINS || a.M == 0 || a.stride < (size_t)(a.fr.N / 2 + 1))
		return hipErrorInvalidValue;
	peaks_kernel<<<dim3((unsigned)(a.frames < (1u << 20) ? a.frames : (1u << 20)), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_walk(const WalkArgs& a, hipStream_t s)
{
	if (a.n_clips == 0 || a.M == 0)
		return hipSuccess;
	if (a.bins <= 0 || a.bins > WALK_TPB * WALK_ITEMS || a.stride < (size_t)a.bins)
		return hipErrorInvalidValue;
	const int tpb = a.bins >= WALK_TPB ? WALK_TPB : (a.bins + 63) / 64 * 64;
	const dim3 grid(grid_rows(a.n_clips), 1, 1);
	const size_t lds = sizeof(uint32_t) * 2 * a.stride;
	switch ((a.bins + tpb - 1) / tpb) {
	case 1:
		walk_kernel<1><<<grid, tpb, lds, s>>>(a);
		break;
	case 2:
		walk_kernel<2><<<grid, tpb, lds, s>>>(a);
		break;
	case 3:
		walk_kernel<3><<<grid, tpb, lds, s>>>(a);
		break;
	default:
		walk_kernel<WALK_ITEMS><<<grid, tpb, lds, s>>>(a);
	}
	return hipGetLastError();
}

hipError_t launch_spectrum(const SpectrumArgs& a, hipStream_t s)
{
	if (a.frames == 0)
		return hipSuccess;
	spectrum_kernel<<<dim3((unsigned)(a.frames < (1u << 20) ? a.frames : (1u << 20)), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_output(const OutputArgs& a, hipStream_t s)
{
	if (a.n_out == 0 || a.n_clips == 0)
		return hipSuccess;
	if (!a.rows && !a.perc)
		return hipErrorInvalidValue;
	output_kernel<<<dim3((unsigned)((a.n_out + TPB - 1) / TPB), grid_rows(a.n_clips), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_phase(const float* re_im, size_t count, uint32_t* theta, hipStream_t s)
{
	if (count == 0)
		return hipSuccess;
	phase_kernel<<<dim3(flat_grid(count), 1, 1), TPB, 0, s>>>(re_im, count, theta);
	return hipGetLastError();
}

hipError_t launch_cs(const uint32_t* psi, size_t count, float* cos_sin, hipStream_t s)
{
	if (count == 0)
		return hipSuccess;
	cs_kernel<<<dim3(flat_grid(count), 1, 1), TPB, 0, s>>>(psi, count, cos_sin);
	return hipGetLastError();
}

} // namespace zen_tsm
