// stft_kernels.h -- the device code the spectrogram add-ons share (zen_amd/repet, repsim, nmf), for their kernel sources:
// the kernels frame (the windowed frames as complex rows) and magnitude with their launchers, and as device functions the
// soft mask of one frame, the overlap-add of one sample and the loader of an LDS tile for the matrix kernels.
//
// Header-only, and everything in it has internal linkage (the anonymous namespace), as in addon_host.h: each library
// compiles a copy of its own into its own code object and launches that one, whichever libraries share the process.
//
// The arithmetic is one IEEE float32 operation at a time (contraction off, hipcc's correctly rounded division and square
// root): part of the contracts of zen_hip_repet.h, zen_hip_repsim.h and zen_hip_nmf.h, which tests/repet_model.py,
// repsim_model.py and nmf_model.py restate bit for bit.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "stft_args.h"

#pragma clang fp contract(off)

namespace zen_addon {
namespace {

constexpr int TPB = 256;

inline unsigned clip_rows(size_t n_clips) { return (unsigned)(n_clips < 65535 ? n_clips : 65535); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------ frame
// xp is H zeros, the clip, zeros: sample j of frame k is x[k H - H + j]
__global__ __launch_bounds__(TPB) void frame_kernel(FrameArgs k)
{
	const int N = k.N, H = N / 2;
	const size_t f = blockIdx.x;
	for (size_t c = blockIdx.y; c < k.n_clips; c += gridDim.y) {
		const float* __restrict__ x = k.in + c * k.in_stride;
		float2* __restrict__ row = reinterpret_cast<float2*>(k.rows) + (c * k.m + f) * (size_t)N;
		for (int j = threadIdx.x; j < N; j += TPB) {
			const size_t pos = f * (size_t)H + (size_t)j; // index into xp
			const float v = pos >= (size_t)H && pos - H < k.n ? x[pos - H] : 0.0f;
			row[j] = make_float2(v * k.win[j], 0.0f);
		}
	}
}

// ------------------------------------------------------------------------------------------------ magnitude
__global__ __launch_bounds__(TPB) void magnitude_kernel(MagArgs k)
{
	const int N = k.N, H = N / 2;
	const size_t f = blockIdx.x;
	const float2* __restrict__ row = reinterpret_cast<const float2*>(k.rows) + f * (size_t)N;
	float* __restrict__ v = k.v + f * k.v_stride;
	for (size_t i = threadIdx.x; i < k.v_stride; i += TPB) {
		float r = 0.0f;
		if (i <= (size_t)H) {
			const float2 z = row[i];
			r = sqrtf(z.x * z.x + z.y * z.y);
		}
		v[i] = r;
	}
}

inline hipError_t launch_frame(const FrameArgs& a, hipStream_t s)
{
	if (a.m == 0 || a.n_clips == 0)
		return hipSuccess;
	frame_kernel<<<dim3((unsigned)a.m, clip_rows(a.n_clips), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

inline hipError_t launch_magnitude(const MagArgs& a, hipStream_t s)
{
	if (a.frames == 0)
		return hipSuccess;
	magnitude_kernel<<<dim3((unsigned)a.frames, 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ soft mask
// A workgroup of TPB threads on one frame: its spectrum `row` (N complex values) in place through M = min(s, v) / v (0 where
// v is not above 0, 1 below bin kc), bin N - f with the mask of bin f.  v: the frame's magnitudes, s: the row of the model.
__device__ __forceinline__ void soft_mask_frame(float2* __restrict__ row, const float* __restrict__ v, const float* __restrict__ s, int N, int kc)
{
	const int H = N / 2;
	for (int f = threadIdx.x; f <= H; f += TPB) {
		const float V = v[f], S = s[f];
		const float W = S < V ? S : V;
		float M = V > 0.0f ? W / V : 0.0f;
		if (f < kc)
			M = 1.0f;
		const float2 z = row[f];
		row[f] = make_float2(z.x * M, z.y * M);
		if (f > 0 && f < H) {
			const float2 y = row[N - f];
			row[N - f] = make_float2(y.x * M, y.y * M);
		}
	}
}

// ------------------------------------------------------------------------------------------------ overlap-add
// sample t of a clip from its inverse-transformed frames (`rows`, N complex values each): the two frames that cover it, the
// earlier one first, over the divisor div[t mod H]
__device__ __forceinline__ float overlap_add_sample(const float* rows, const float* div, size_t t, int N)
{
	const int H = N / 2;
	const size_t fr = t / H;
	const int i = (int)(t % H);
	const float2* __restrict__ g = reinterpret_cast<const float2*>(rows);
	return (g[fr * N + H + i].x + g[(fr + 1) * N + i].x) / div[i];
}

// ------------------------------------------------------------------------------------------------ LDS tile
// The operand tile of a matrix kernel (repsim's similarity, nmf's product): ROWS rows of KC indices of the reduction, a row
// of KC + 1 words (the 64 lanes of an operand read on 64 banks).  T[r * LDK + q] = v[(r0 + r) * stride + l0 + q] for the TPB
// threads of a workgroup, `pad` past `rows` and past L.  VEC wants v 16-byte aligned and stride a multiple of 4.
constexpr int KC = 32;
constexpr int LDK = KC + 1;

template <int ROWS, bool VEC>
__device__ __forceinline__ void load_tile(float* __restrict__ T, const float* __restrict__ v, size_t stride, size_t r0, size_t rows, size_t l0,
                                          size_t L, float pad, int tid)
{
	if (VEC) {
#pragma unroll
		for (int i = 0; i < ROWS * KC / 4 / TPB; ++i) {
			const int s = tid + TPB * i, r = s >> 3, q = (s & 7) * 4;
			const size_t row = r0 + r, l = l0 + q;
			float4 x = make_float4(pad, pad, pad, pad);
			if (row < rows) {
				const float* __restrict__ p = v + row * stride + l;
				if (l + 4 <= L) {
					x = *reinterpret_cast<const float4*>(p);
				} else {
					x.x = l < L ? p[0] : pad;
					x.y = l + 1 < L ? p[1] : pad;
					x.z = l + 2 < L ? p[2] : pad;
				}
			}
			float* __restrict__ d = T + r * LDK + q;
			d[0] = x.x;
			d[1] = x.y;
			d[2] = x.z;
			d[3] = x.w;
		}
	} else {
#pragma unroll
		for (int i = 0; i < ROWS * KC / TPB; ++i) {
			const int e = tid + TPB * i, r = e >> 5, q = e & 31;
			const size_t row = r0 + r, l = l0 + q;
			T[r * LDK + q] = row < rows && l < L ? v[row * stride + l] : pad;
		}
	}
}

} // namespace
} // namespace zen_addon
