/*
 * zen_hip_tsm.h -- time-scale modification on device rows: the harmonic stem through a phase-locked phase vocoder, the
 * percussive stem (and the residual) through plain overlap-add on short frames, and their sum
 * (libzen_hip_tsm.so, linked against libzen_hip.so).
 *
 * The method is Driedger, Mueller and Ewert, "Improving time-scale modification of music signals using harmonic-percussive
 * separation" (IEEE SPL 21(1), 2014); the vocoder's identity phase locking is Laroche and Dolson, "Improved phase vocoder
 * time-scale modification of audio" (IEEE TSAP 7(3), 1999).  DESIGN.md section 21 states it in full and says what was measured.
 *
 * The arithmetic (tests/tsm_model.py computes the same bits).  Phases are 32-bit unsigned fractions of a turn: one turn is
 * 2^32, u32 arithmetic wraps, so the principal-argument wrap is integer overflow and integer sums may be regrouped freely.
 * Every float operation on the device is one of + - * / sqrt rne compare in float32, one rounding each (rne: round to nearest
 * even of a float32 to an integer-valued float32); everything transcendental is a table computed on the host in double (libm
 * cos, sin, atan) and rounded once -- zen_hip_tsm_table hands them out.
 *
 *   Parameters: alpha, a finite double in [0.25, 4]; the vocoder's frame N, a power of two in 64..8192, Hs = N / 4, H = N / 2,
 *   overlap V = 4; the overlap-add frame Np, a power of two in 16..4096, Hs = Np / 2, V = 2; n_clips >= 1 rows of equal length
 *   n, stretched alike in one call.
 *   Tables: w[i] = 0.5 - 0.5 cos(2 pi i / N), the periodic Hann window (wp: the same of Np); D[i] = float32(N sum_{j<4}
 *   (double)w[i + j Hs]^2), i < Hs; d2[i] = float32((double)wp[i] + (double)wp[i + Np / 2]); A[a] = (cos, sin)(2 pi a / 2048),
 *   a < 2048; B[b] = (cos, sin)(2 pi b / 2^22), b < 2048; T[i] = (u32) llround(atan(i / 256) / (2 pi) 2^32), i <= 256;
 *   c3 = float32(1 / 3), K = float32(2^32 / (2 pi)).
 *
 *   Framing (both routes, each with its N, Hs, V): n_out = floor((double)n alpha); M = (n_out - 1) / Hs + V frames;
 *   a_m = floor((double)((m - V / 2 + 1) Hs) / alpha), one double division, floor towards minus infinity (a_0 may be negative);
 *   Ha_m = a_m - a_{m-1} >= 1; x[i] = 0 outside [0, n); element i of frame m is x[a_m - N / 2 + i] w[i].
 *
 *   atan2turns(y, x), a u32 phase: ax = |x|, ay = |y|; both zero: 0.  hi = max(ax, ay), lo = min(ax, ay), q = lo / hi;
 *   i = (int) rne(q 256), qi = i / 256; t = (q - qi) / (1 + q qi); s = t t; u = t - (t s) c3; r = (int) rne(u K);
 *   phi = T[i] + r; ay > ax: phi = 2^30 - phi; x < 0: phi = 2^31 - phi; y < 0: phi = -phi.  Plain float compares (-0 is
 *   not < 0); inputs are finite, denormals are kept.
 *   cs(psi) = (C, S): a = psi >> 21, b = (psi >> 10) & 2047; C = A[a].c B[b].c - A[a].s B[b].s; S = A[a].s B[b].c + A[a].c B[b].s.
 *
 *   The vocoder, per clip:
 *   1. The frame rows (x w, 0) through the forward N-point transform (zen_hip_fft_exec_batched).
 *   2. For the bins k <= H: mag = sqrt(re re + im im), theta_m[k] = atan2turns(im, re).
 *   3. k is a peak iff mag[k] > mag[j] for every j in {k - 2, k - 1, k + 1, k + 2} within [0, H]; a frame without a peak has
 *      every bin as a peak.  own_m[k] is the nearest peak, the lower one of two at the same distance.
 *   4. psi_0[k] = theta_0[k].  For m >= 1, with Omega(k, h) = ((k h) mod N) (2^32 / N): at a peak p,
 *      delta = (int32)(theta_m[p] - theta_{m-1}[p] - Omega(p, Ha_m)) and
 *      psi_m[p] = psi_{m-1}[p] + Omega(p, Hs) + (u32)((int64) delta Hs / Ha_m), the quotient rounded towards zero;
 *      elsewhere psi_m[k] = psi_m[own] + theta_m[k] - theta_m[own].
 *   5. Y_m[k] = (mag C, mag S), (C, S) = cs(psi_m[k]); Y_m[N - k] = (re, -im) of Y_m[k] for 0 < k < H.
 *   6. g_m = the real part of the unnormalised inverse transform.  For output t, q = t / Hs, i = t mod Hs,
 *      p_j = g_{q+j}[i + (3 - j) Hs] w[i + (3 - j) Hs]; pv[t] = (((p_0 + p_1) + p_2) + p_3) / D[i].
 *   Overlap-add (perc and optionally resid, added sample by sample): f_m[i] = (perc[.] (+ resid[.])) wp[i], the same framing
 *   with Np; ola[t] = (f_q[i + Np / 2] + f_{q+1}[i]) / d2[i].
 *   HP stretch: out[t] = pv(harm)[t] + ola(perc, resid)[t], one add.
 *   At alpha = 1, Ha_m = Hs and psi_m[k] == theta_m[k] for every m and k, exactly.
 *
 * Conventions: those of zen_hip.h and zen_hip_repet.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_tsm_last_error() (this library's own thread-local message; failures of the library underneath are copied into
 * it).  All device memory comes from zen_hip_malloc, all of it allocated by zen_hip_tsm_create, never by a call; the three
 * trigonometric tables are constants of the library's code object, written once per device.
 */
#ifndef ZEN_HIP_TSM_H
#define ZEN_HIP_TSM_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_tsm* zen_hip_tsm_t;

typedef struct zen_hip_tsm_stats_t {
	unsigned long long calls;        /* stretch and inspect calls since create, host calls included */
	unsigned long long clips;        /* clips stretched since create */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the FFT handle's own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_tsm_stats_t;

/* frame, fft, analysis, peaks, walk, spectrum, ifft, overlap_add */
enum { ZEN_HIP_TSM_KERNELS = 8 };
enum { ZEN_HIP_TSM_MAX_FRAMES = 16384 };
enum {
	ZEN_HIP_TSM_TABLE_WINDOW = 0,      /* nfft floats; nfft a power of two in 16..8192 */
	ZEN_HIP_TSM_TABLE_PV_DIVISOR = 1,  /* D: nfft / 4 floats; nfft in 64..8192 */
	ZEN_HIP_TSM_TABLE_OLA_DIVISOR = 2, /* d2: nfft / 2 floats; nfft in 16..4096 */
	ZEN_HIP_TSM_TABLE_COARSE = 3,      /* A: 2048 (cos, sin) pairs of floats; nfft is not looked at */
	ZEN_HIP_TSM_TABLE_FINE = 4,        /* B: 2048 (cos, sin) pairs of floats */
	ZEN_HIP_TSM_TABLE_ATAN = 5,        /* T: 257 unsigned 32-bit words */
	ZEN_HIP_TSM_TABLE_CONSTANTS = 6    /* c3, K: 2 floats */
};

const char* zen_hip_tsm_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_tsm_version(void);

/* fs > 0; nfft: the vocoder's frame, a power of two in 64..8192; nfft_ola: the overlap-add frame, a power of two in 16..4096;
 * n_clips >= 1 rows stretched by every call; max_samples >= 1: the longest clip a call may bring; max_alpha in [0.25, 4]: the
 * largest ratio a call may ask for at that length.  floor(max_samples max_alpha) output samples must make at most 16384
 * frames on either route (ZEN_HIP_E_BAD_ARG otherwise, before a device is touched).  create allocates everything, the
 * transform's own included (it runs its largest batch once, on zeros): afterwards no call of the session allocates.  With M
 * the vocoder's frames of the longest output that is n_clips M (8 nfft + 18 (nfft / 2 + 4)) bytes, 4 n_clips (3 max_samples +
 * the longest output) bytes for the host call and a little more. */
int zen_hip_tsm_create(float fs, size_t nfft, size_t nfft_ola, size_t n_clips, size_t max_samples, double max_alpha, zen_hip_tsm_t* h);
int zen_hip_tsm_destroy(zen_hip_tsm_t h);
int zen_hip_tsm_set_stream(zen_hip_tsm_t h, void* stream); /* waits for what the previous stream holds */

/* Clip c is the n floats from in + c * in_stride on, 1 <= n <= max_samples; row c of the output is the n_out = floor(n alpha)
 * floats from out + c * out_stride on.  Each call writes n_clips rows of n_out floats and nothing outside them, and is
 * asynchronous on the handle's stream.  Pointers need 4-byte alignment; in_stride >= n, out_stride >= n_out, alpha finite in
 * [0.25, 4], n_out >= 1 and within what create sized (ZEN_HIP_E_BAD_ARG otherwise, nothing is touched).  resid may be NULL. */
int zen_hip_tsm_stretch_pv_device(zen_hip_tsm_t h, const float* in_dev, size_t in_stride, size_t n, double alpha, float* out_dev, size_t out_stride);
int zen_hip_tsm_stretch_ola_device(zen_hip_tsm_t h, const float* perc_dev, const float* resid_dev, size_t in_stride, size_t n, double alpha,
                                   float* out_dev, size_t out_stride);
int zen_hip_tsm_stretch_hp_device(zen_hip_tsm_t h, const float* harm_dev, const float* perc_dev, const float* resid_dev, size_t in_stride, size_t n,
                                  double alpha, float* out_dev, size_t out_stride);
/* The same rows in host memory: plain copies up and down around the device call.  Synchronous. */
int zen_hip_tsm_stretch_hp_host(zen_hip_tsm_t h, const float* harm_host, const float* perc_host, const float* resid_host, size_t in_stride, size_t n,
                                double alpha, float* out_host, size_t out_stride);

/* Steps 1-4 of the vocoder, for the tests: each non-NULL output receives n_clips * M rows of nfft / 2 + 1 values in device
 * memory, packed (clip, frame, bin): mag floats, theta and psi unsigned 32-bit words, owner unsigned 16-bit words.
 * Asynchronous on the handle's stream. */
int zen_hip_tsm_inspect_device(zen_hip_tsm_t h, const float* in_dev, size_t in_stride, size_t n, double alpha, float* mag_dev, unsigned* theta_dev,
                               unsigned short* owner_dev, unsigned* psi_dev);

/* The two table functions alone, without a handle; asynchronous on `stream` (a hipStream_t as void*).  phase: `count` (re, im)
 * pairs of floats -> count phases atan2turns(im, re).  cs: count phases -> count (cos, sin) pairs of floats.  A null or
 * misaligned (4 bytes) pointer: ZEN_HIP_E_BAD_ARG, nothing is touched; count == 0 does nothing. */
int zen_hip_tsm_phase_device(const float* re_im_dev, size_t count, unsigned* theta_dev, void* stream);
int zen_hip_tsm_cs_device(const unsigned* psi_dev, size_t count, float* cos_sin_dev, void* stream);

int zen_hip_tsm_stats(zen_hip_tsm_t h, zen_hip_tsm_stats_t* out);

/* Profiling hooks for the harness (tools/ab_tsm.py), as the repet library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step (the order of ZEN_HIP_TSM_KERNELS'
 * comment) milliseconds, bytes read + written, and launches. */
int zen_hip_tsm_profile(zen_hip_tsm_t h, int enable);
int zen_hip_tsm_profile_get(zen_hip_tsm_t h, double ms[ZEN_HIP_TSM_KERNELS], unsigned long long bytes[ZEN_HIP_TSM_KERNELS],
                            unsigned long long launches[ZEN_HIP_TSM_KERNELS]);

/* The framing of either route on the host, without a device: n samples, a frame of `frame` samples (a power of two in
 * 16..8192), overlap 4 or 2, alpha -> *n_out, *frames (M) and, where a_out is not NULL, the M analysis positions a_m (cap, the
 * values a_out has room for, must be at least M).  n == 0, n_out == 0, alpha outside [0.25, 4] or not finite, another
 * overlap: ZEN_HIP_E_BAD_ARG. */
int zen_hip_tsm_positions(size_t n, size_t frame, size_t overlap, double alpha, size_t* n_out, size_t* frames, long long* a_out, size_t cap);
/* One host table, computed without a device: `which` is a ZEN_HIP_TSM_TABLE_* value.  out receives the table's 4-byte words;
 * cap, the words out has room for, must be at least its length (ZEN_HIP_E_BAD_ARG otherwise, as for an nfft outside the
 * table's range and an unknown table). */
int zen_hip_tsm_table(size_t nfft, int which, void* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_TSM_H */
