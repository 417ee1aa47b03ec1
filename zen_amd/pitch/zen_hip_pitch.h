/*
 * zen_hip_pitch.h -- pitch tracking on device rows: the McLeod pitch method (MPM) on chunks of a stream
 * (libzen_hip_pitch.so, linked against libzen_hip.so).
 *
 * The reference's second use of its separations (demos/pitch-tracking: "pitch tracking is improved with real-time harmonic
 * separation").  A session takes rows of samples that already are in device memory -- the harmonic rows a
 * zen_hip_hpr_process call has just written, for one -- cuts them into chunks of n samples and gives one pitch per chunk,
 * without a trip to the host.
 *
 * The arithmetic (tests/pitch_model.py computes the same bits).  Per chunk x[0..n) of float32:
 *   1. r = Re IFFT_2n( |FFT_2n(x ++ n zeros)|^2 )[0..n): the engine's transforms (zen_hip_fft_exec_batched, unnormalised),
 *      the power re*re + im*im in float32 (two multiplies, one add) on all 2n bins;
 *   2. P[k] = sum_{j<k} (double)x[j]^2 in runs of L = min(64, n) samples: each run summed left to right, the run totals
 *      summed left to right, P[k] = (totals of the earlier runs) + (the sum within k's run);
 *      m[t] = (P[n-t] - P[0]) + (P[n] - P[t]);
 *   3. the normalised square difference function a[t] = (float)((double)r[t] / ((double)n * m[t])) where m[t] > 0, else 0;
 *   4. key maxima: with T = (n-1)/3, p = min(T, first t with a[t] <= 0), advanced to the first t >= p with a[t] > 0 (at
 *      most n-1): per maximal run of positive values in [p, n-2], the largest a[i] among the i with a[i] > a[i-1] and
 *      a[i] >= a[i+1], the earliest on equal values;
 *   5. every key maximum above 0.5 is refined by a parabola through (i-1, i, i+1) in float32; hi = the largest value among
 *      all key maxima and all refined values; the first refined peak whose value reaches (float)(0.93 * (double)hi) gives
 *      `period` (in samples) and `clarity`; pitch = fs / period where that is above 80 Hz, else -1.  No such peak:
 *      pitch -1, period 0, clarity 0.
 * Samples are expected to be finite.
 *
 * Conventions: those of zen_hip.h and zen_hip_live.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_pitch_last_error() (this library's own thread-local message; failures of the library underneath are copied
 * into it).  All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  Everything
 * is allocated by zen_hip_pitch_create, sized by n, n_streams and max_chunks, never by the length of a call.
 */
#ifndef ZEN_HIP_PITCH_H
#define ZEN_HIP_PITCH_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_pitch* zen_hip_pitch_t;

typedef struct zen_hip_pitch_stats_t {
	unsigned long long chunks;       /* chunks analysed since create (all streams) */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the FFT handle's own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_pitch_stats_t;

enum { ZEN_HIP_PITCH_KERNELS = 5 }; /* pad, fft forward, power, fft inverse, pick */

const char* zen_hip_pitch_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_pitch_version(void);

/* fs: sample rate; n: chunk length, a power of two in 32..16384 (ZEN_HIP_E_BAD_ARG otherwise); n_streams >= 1 rows analysed
 * by every call.  max_chunks only sizes the workspace: calls with more chunks per stream run in slices of max_chunks.
 * 0 = default: 2^23 / (n * n_streams) chunks, clamped to 1..65536.  A slice takes 32 bytes of device memory per sample (the
 * complex rows 16, the prefix 8, the staging rows of the host calls 8; n = 16384 another 16 inside the transform), so the
 * default is 256 MiB unless one chunk of every stream already is more.  create allocates all of it, the transform's own
 * included (it runs its largest batch once, on zeros): afterwards no call of the session allocates. */
int zen_hip_pitch_create(float fs, size_t n, size_t n_streams, size_t max_chunks, zen_hip_pitch_t* h);
int zen_hip_pitch_destroy(zen_hip_pitch_t h);
int zen_hip_pitch_set_stream(zen_hip_pitch_t h, void* stream); /* waits for what the previous stream holds */

/* Chunk c of stream s is the n floats from in_dev + s * in_stride + c * step on; step >= 1, so chunks may overlap or leave
 * gaps.  Each non-NULL result receives n_streams rows of n_chunks floats, out_stride floats apart: pitch in Hz or -1,
 * period in samples or 0, clarity (the NSDF value of the chosen peak) or 0.  nsdf_dev (optional) receives the NSDF itself,
 * n floats per chunk: rows of n_chunks * n floats, out_stride * n floats apart.  n_chunks == 0 is legal and touches
 * nothing.  Nothing outside the named elements is written.  Pointers need 4-byte alignment only; out_stride >= n_chunks
 * where a result is asked for (ZEN_HIP_E_BAD_ARG otherwise, nothing is touched).  Asynchronous on the handle's stream;
 * calls may be queued back to back. */
int zen_hip_pitch_run_device(zen_hip_pitch_t h, const float* in_dev, size_t in_stride, size_t n_chunks, size_t step, float* pitch_dev,
                             float* period_dev, float* clarity_dev, float* nsdf_dev, size_t out_stride);
/* The same rows in host memory: plain copies up and down around the device call, slice by slice.  Synchronous. */
int zen_hip_pitch_run_host(zen_hip_pitch_t h, const float* in_host, size_t in_stride, size_t n_chunks, size_t step, float* pitch_host,
                           float* period_host, float* clarity_host, float* nsdf_host, size_t out_stride);

int zen_hip_pitch_stats(zen_hip_pitch_t h, zen_hip_pitch_stats_t* out);

/* Profiling hooks for the harness (tools/ab_pitch.py), as the live library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step ([0] pad, [1] forward FFT, [2] power,
 * [3] inverse FFT, [4] pick) milliseconds, bytes read + written, and launches. */
int zen_hip_pitch_profile(zen_hip_pitch_t h, int enable);
int zen_hip_pitch_profile_get(zen_hip_pitch_t h, double ms[ZEN_HIP_PITCH_KERNELS], unsigned long long bytes[ZEN_HIP_PITCH_KERNELS],
                              unsigned long long launches[ZEN_HIP_PITCH_KERNELS]);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_PITCH_H */
