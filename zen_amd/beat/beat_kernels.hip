// beat_kernels.hip -- the three kernels of libzen_hip_beat.so (gfx950) around the public FFT call: frame (the windowed,
// rotated frame of every hop as a complex row), csd (the rectified complex spectral difference of three consecutive spectra,
// summed to one onset value per hop) and track (the cumulative score, the beat prediction and the tempo estimate, hop after
// hop).  One workgroup of 256 threads per hop and stream in frame and csd; one workgroup per stream in track, which walks
// the hops of the slice in order with its buffers in LDS.
//
// The arithmetic is the contract of zen_hip_beat.h / DESIGN.md section 15, one IEEE float32 operation at a time
// (contraction off, hipcc's correctly rounded division and square root): tests/beat_model.py gives the same bits.  Where
// the contract fixes an order of additions one thread adds in that order: a lane of csd over its column, a thread per
// window of thr, a thread per lag of the autocorrelation, every thread alike over the 41 tempo weights.  Maxima are exact
// in any order, so they are block reductions.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

#include "beat_kernels.h"
#include "beat_tables.h"

#pragma clang fp contract(off)

namespace zen_beat {
namespace {

constexpr int TPB = 256, WAVES = TPB / 64;
constexpr int MAX_N = 4096; // the frame of hop 2048
constexpr int BATCH = 256;  // hops whose onset values and results the track kernel holds in LDS at a time
constexpr int MASK = HISTORY - 1;

unsigned stream_rows(size_t n_streams) { return (unsigned)(n_streams < 65535 ? n_streams : 65535); }

// ------------------------------------------------------------------------------------------------ frame
__global__ __launch_bounds__(TPB) void frame_kernel(FrameArgs k)
{
	const int hop = k.hop, n = 2 * hop, t = threadIdx.x;
	const size_t c = blockIdx.x;
	for (size_t s = blockIdx.y; s < k.n_streams; s += gridDim.y) {
		const float* __restrict__ cur = k.in + s * k.in_stride + c * (size_t)hop; // 4-byte alignment only
		const float* __restrict__ old = c ? cur - hop : k.tail + s * (size_t)hop;
		float2* __restrict__ row = reinterpret_cast<float2*>(k.rows) + ((2 + c) * k.n_streams + s) * (size_t)n;
		// row[i] = z[(i + hop) mod N], z = frame * window: the new hop comes first, under the falling half of the window
		for (int i = t; i < n; i += TPB) {
			const float x = i < hop ? cur[i] * k.win[hop + i] : old[i - hop] * k.win[i - hop];
			row[i] = make_float2(x, 0.0f);
		}
	}
}

// ------------------------------------------------------------------------------------------------ csd
__device__ __forceinline__ void unit(float2 x, float* m, float* ur, float* ui)
{
	*m = sqrtf(x.x * x.x + x.y * x.y);
	if (*m == 0.0f) {
		*ur = 1.0f;
		*ui = 0.0f;
	} else {
		*ur = x.x / *m;
		*ui = x.y / *m;
	}
}

__global__ __launch_bounds__(TPB) void csd_kernel(CsdArgs k)
{
	__shared__ float v[MAX_N];
	const int n = 2 * k.hop, t = threadIdx.x;
	const size_t c = blockIdx.x, S = k.n_streams;
	for (size_t s = blockIdx.y; s < S; s += gridDim.y) {
		const float2* __restrict__ x2 = reinterpret_cast<const float2*>(k.rows) + (c * S + s) * (size_t)n;
		const float2* __restrict__ x1 = x2 + S * (size_t)n;
		const float2* __restrict__ x0 = x1 + S * (size_t)n;
		for (int i = t; i < n; i += TPB) {
			const float2 z = x0[i];
			float m, m1, m2, ur, ui, u1r, u1i, u2r, u2i;
			unit(z, &m, &ur, &ui);
			unit(x1[i], &m1, &u1r, &u1i);
			unit(x2[i], &m2, &u2r, &u2i);
			const float sr = u1r * u1r - u1i * u1i, si = u1r * u1i + u1r * u1i;
			const float dr = sr * u2r + si * u2i, di = si * u2r - sr * u2i;
			const float er = z.x - m1 * dr, ei = z.y - m1 * di;
			v[i] = m > m1 ? sqrtf(er * er + ei * ei) : 0.0f;
		}
		__syncthreads();
		if (t < 64) { // the association of the sum is the contract: lane l adds its column in order, then the halving tree
			float p = v[t];
			for (int i = 64 + t; i < n; i += 64)
				p = p + v[i];
			for (int o = 32; o; o >>= 1)
				p = p + __shfl_down(p, o);
			if (t == 0)
				k.odf[s * k.odf_stride + c] = p;
		}
		__syncthreads(); // v is reused by the next stream
	}
}

// ------------------------------------------------------------------------------------------------ track
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

// thr of the contract on x[0..len), element i; `at` maps a logical index to the LDS word
template <class At>
__device__ __forceinline__ float thr_at(const float* x, int len, int i, At at)
{
	const int lo = i - 8 > 0 ? i - 8 : 0, hi = i + 8 < len ? i + 8 : len;
	float acc = 0.0f;
	for (int q = lo; q < hi; ++q)
		acc = acc + x[at(q)];
	const float d = x[at(i)] - acc / (float)(hi - lo);
	return d > 0.0f ? d : 0.0f;
}

// df and cs are rings in LDS: the logical element i (0 the oldest, 511 the newest) is word (head + i) & 511.
__global__ __launch_bounds__(TPB) void track_kernel(TrackArgs k)
{
	__shared__ float df[HISTORY], cs[HISTORY], y[HISTORY], ac[HISTORY];
	__shared__ float fut[MAX_PERIOD], cr[128], ct[128], w1[W1_ROW], w2[W2_ROW];
	__shared__ float trans[TEMPI * TEMPI], tempo[TEMPI], prev[TEMPI], delta[TEMPI];
	__shared__ int bp[TEMPI];
	__shared__ float in_buf[BATCH], o_score[BATCH], o_beat[BATCH], o_tempo[BATCH];
	__shared__ float scratch[WAVES];
	int* iscratch = reinterpret_cast<int*>(scratch);
	const int t = threadIdx.x;
	const float* __restrict__ tab = k.tables;
	for (int i = t; i < TEMPI * TEMPI; i += TPB)
		trans[i] = tab[OFF_TRANS + i];
	if (t < TEMPI) {
		tempo[t] = tab[OFF_TEMPO + t];
		bp[t] = (int)tab[OFF_PERIOD + t];
	}
	for (size_t s = blockIdx.x; s < k.n_streams; s += gridDim.x) {
		float* __restrict__ st = k.state + s * STATE_WORDS;
		int* __restrict__ sti = reinterpret_cast<int*>(st + 2 * HISTORY + TEMPI);
		for (int i = t; i < HISTORY; i += TPB) {
			df[i] = st[i];
			cs[i] = st[HISTORY + i];
		}
		if (t < TEMPI)
			prev[t] = st[2 * HISTORY + t];
		int b = sti[0], m0 = sti[1], bc = sti[2], j = sti[3], head = sti[4] & MASK;
		// the state is the session's own, but an index into LDS is checked all the same
		b = b < 1 ? 1 : b > MAX_PERIOD ? MAX_PERIOD : b;
		j = j < 0 ? 0 : j >= TEMPI ? TEMPI - 1 : j;
		w1[t] = tab[OFF_PAST + (size_t)b * W1_ROW + t];
		if (t < W2_ROW)
			w2[t] = tab[OFF_FUTURE + (size_t)b * W2_ROW + t];
		__syncthreads();
		for (size_t base = 0; base < k.hops; base += BATCH) {
			const int cnt = k.hops - base < (size_t)BATCH ? (int)(k.hops - base) : BATCH;
			if (t < cnt)
				in_buf[t] = k.odf_ws[s * k.odf_stride + base + t];
			__syncthreads();
			for (int h = 0; h < cnt; ++h) {
				const float v = fabsf(in_buf[h]) + 1e-4f;
				m0 -= 1;
				bc -= 1;
				const int r2 = 2 * b, rh = (b + 1) >> 1, K = r2 - rh + 1;
				// ---- the score: the best of the past scores one period back, under the log-Gaussian window
				const float past = t < K ? cs[(head + HISTORY - r2 + t) & MASK] * w1[t] : 0.0f;
				const float M = block_max(past, scratch);
				const float score = (1.0f - 0.9f) * v + 0.9f * M;
				if (t == 0) { // the oldest word becomes the newest
					df[head] = v;
					cs[head] = score;
				}
				head = (head + 1) & MASK;
				__syncthreads();
				// ---- the next beat: the scores run on into the future over one period.  Element 512 + n reads nothing
				// newer than 512 + n - rh, so rh elements at a time are independent of each other: one thread each.
				if (m0 == 0) {
					for (int n0 = 0; n0 < b; n0 += rh) {
						const int n = n0 + t;
						if (t < rh && n < b) {
							float m = 0.0f;
							for (int q = 0; q < K; ++q) {
								const int idx = HISTORY + n - r2 + q;
								const float p = (idx < HISTORY ? cs[(head + idx) & MASK] : fut[idx - HISTORY]) * w1[q];
								m = p > m ? p : m;
							}
							fut[n] = m;
						}
						__syncthreads();
					}
					const float q = t < b ? fut[t] * w2[t] : 0.0f;
					const float top = block_max(q, scratch);
					int first = block_min(top > 0.0f && t < b && q == top ? t : INT_MAX, iscratch);
					if (first == INT_MAX)
						first = 0;
					bc = first;
					m0 = first + rh;
				}
				const bool beat = bc == 0;
				// ---- the tempo, at every beat
				if (beat) {
					const auto ring = [head](int i) { return (head + i) & MASK; };
					const auto plain = [](int i) { return i; };
					for (int i = t; i < HISTORY; i += TPB)
						y[i] = thr_at(df, HISTORY, i, ring);
					__syncthreads();
					for (int half = 0; half < 2; ++half) { // lags t and 511 - t: 513 terms per thread
						const int l = half ? HISTORY - 1 - t : t;
						float acc = 0.0f;
						for (int i = 0; i < HISTORY - l; ++i)
							acc = acc + y[i] * y[i + l];
						ac[l] = acc / (float)(HISTORY - l);
					}
					__syncthreads();
					if (t < 128) { // cr[i - 1] = C[i]
						const int i = t + 1;
						float c = 0.0f;
						if (i >= 2 && i <= 127) {
							const float R = tab[OFF_RAYLEIGH + i];
							for (int a = 1; a <= 4; ++a)
								for (int o = 1 - a; o <= a - 1; ++o)
									c = c + (ac[a * i + o - 1] * R) / (float)(2 * a - 1);
						}
						cr[t] = c;
					}
					__syncthreads();
					if (t < 128)
						ct[t] = thr_at(cr, 128, t, plain);
					__syncthreads();
					if (t < TEMPI) {
						const int p = bp[t];
						const float O = ct[p - 1] + ct[p / 2 - 1];
						float m = prev[0] * trans[t];
						for (int i = 1; i < TEMPI; ++i) {
							const float w = prev[i] * trans[i * TEMPI + t];
							m = w > m ? w : m;
						}
						delta[t] = m * O;
					}
					__syncthreads();
					float total = 0.0f;
					for (int i = 0; i < TEMPI; ++i) {
						const float d = delta[i];
						if (d > 0.0f)
							total = total + d;
					}
					__syncthreads();
					if (total > 0.0f && t < TEMPI)
						delta[t] = delta[t] / total;
					__syncthreads();
					j = 0;
					float best = delta[0];
					for (int i = 1; i < TEMPI; ++i)
						if (delta[i] > best) {
							best = delta[i];
							j = i;
						}
					b = bp[j];
					if (t < TEMPI)
						prev[t] = delta[t];
					w1[t] = tab[OFF_PAST + (size_t)b * W1_ROW + t];
					if (t < W2_ROW)
						w2[t] = tab[OFF_FUTURE + (size_t)b * W2_ROW + t];
					__syncthreads();
				}
				if (t == 0) {
					o_score[h] = score;
					o_beat[h] = beat ? 1.0f : 0.0f;
					o_tempo[h] = tempo[j];
				}
			}
			__syncthreads();
			if (t < cnt) {
				const size_t o = s * k.out_stride + k.c0 + base + t;
				if (k.odf)
					k.odf[o] = in_buf[t];
				if (k.score)
					k.score[o] = o_score[t];
				if (k.beat)
					k.beat[o] = o_beat[t];
				if (k.tempo)
					k.tempo[o] = o_tempo[t];
			}
			__syncthreads();
		}
		for (int i = t; i < HISTORY; i += TPB) {
			st[i] = df[i];
			st[HISTORY + i] = cs[i];
		}
		if (t < TEMPI)
			st[2 * HISTORY + t] = prev[t];
		if (t == 0) {
			sti[0] = b;
			sti[1] = m0;
			sti[2] = bc;
			sti[3] = j;
			sti[4] = head;
		}
		__syncthreads(); // the LDS is reused by the next stream
	}
}

} // namespace

hipError_t launch_frame(const FrameArgs& a, hipStream_t s)
{
	if (a.hops == 0 || a.n_streams == 0)
		return hipSuccess;
	frame_kernel<<<dim3((unsigned)a.hops, stream_rows(a.n_streams), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_csd(const CsdArgs& a, hipStream_t s)
{
	if (a.hops == 0 || a.n_streams == 0)
		return hipSuccess;
	if (2 * a.hop > MAX_N)
		return hipErrorInvalidValue;
	csd_kernel<<<dim3((unsigned)a.hops, stream_rows(a.n_streams), 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_track(const TrackArgs& a, hipStream_t s)
{
	if (a.hops == 0 || a.n_streams == 0)
		return hipSuccess;
	track_kernel<<<dim3(stream_rows(a.n_streams), 1, 1), TPB, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace zen_beat
