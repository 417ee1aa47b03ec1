/*
 * zen_hip_repet.h -- REPET on device rows: the repeating background of a recording against its foreground
 * (libzen_hip_repet.so, linked against libzen_hip.so).
 *
 * The separations of zen_hip.h are harmonic / percussive / residual.  This one gives the stem they do not: lead or voice
 * against accompaniment, by the published median-filtering method for it (Rafii and Pardo, "REpeating Pattern Extraction
 * Technique (REPET): A Simple Method for Music/Voice Separation", IEEE TASLP 21(1), 2013).  It finds the period of the
 * repeating accompaniment from the beat spectrum of the spectrogram, takes the median of the spectrogram over the
 * repetitions, builds a soft mask from that median and resynthesises through the mask.  DESIGN.md section 17 states it in
 * full and says what was measured.
 *
 * The arithmetic (tests/repet_model.py computes the same bits).  Every float operation on the device is one of + - * /
 * sqrt min max compare in float32, one rounding each; everything transcendental is a table computed on the host in double
 * (libm cos) and rounded once to float32 -- zen_hip_repet_table hands them out.
 *
 *   Parameters: fs; the frame N, a power of two in 64..8192, H = N / 2, bins = H + 1; n_clips >= 1 rows of equal length,
 *   each separated on its own with its own period.  A clip of n >= 1 samples has m = ceil(n / H) + 1 frames, m <= 16384.
 *   Tables: the periodic Hamming window w[i] = 0.54 - 0.46 cos(2 pi i / N); d[i] = float32(N ((double)w[i] + (double)w[i + H])).
 *
 *   1. xp = H zeros, the clip, zeros up to (m + 1) H samples.  Frame k is xp[k H .. k H + N); its row is (xp w, 0); X_k is
 *      the forward N-point transform of the row (zen_hip_fft_exec_batched).
 *   2. V[k][f] = sqrt(re re + im im), f < bins.
 *   3. L = the smallest power of two >= max(64, 2 m).  Per bin f the row (V[k][f] V[k][f], 0), k < m, zeros up to L; its
 *      forward L-point transform; (re re + im im, 0); the inverse transform; a[f][j] its real part, j < m.
 *      braw[j] = a[0][j] / (float)(m - j) + a[1][j] / (float)(m - j) + ..., the bins in order from +0.
 *   4. zen_hip_repet_find_period, on the host in double: b[j] = braw[j] / braw[0]; l = floor(3 m / 4); for every candidate j
 *      in [jmin, min(jmax, floor(l / 3))], jmin = max(2, ceil(tmin fs / H)), jmax = floor(tmax fs / H): D = floor(3 j / 4),
 *      I = 0; for i = j, 2 j, .. while i < l: h1 = the first index of the largest b in [max(1, i - 2), min(l - 1, i + 2)],
 *      h2 the same over [max(1, i - D), min(l - 1, i + D)]; where h1 == h2, I += b[h1] - (the sum of b over the D window,
 *      left to right from 0) / (its count).  J[j] = I / floor(l / j).  The period p is the first j with the largest J,
 *      provided J > 0.  No period (p = 0): an empty candidate range, no positive J, braw[0] zero or not finite.
 *   5. r = ceil(m / p), 2 <= r <= 256.  For l < p the column of the c values V[l + q p][f], l + q p < m (c = r or r - 1);
 *      S[l][f] = their median: sorted s[0..c), s[(c - 1) / 2] for odd c, (s[c / 2 - 1] + s[c / 2]) * 0.5f for even c.
 *   6. W = min(S[k mod p][f], V[k][f]); M = W / V where V > 0, else 0; with a high-pass cut-off fc > 0, kc = ceil(fc N / fs)
 *      in double and M = 1 for f < kc.  Y_k[f] = (re M, im M) for f <= H, Y_k[N - f] = (re_{N-f} M[f], im_{N-f} M[f]) for
 *      0 < f < H.
 *   7. g_k = the real part of the unnormalised inverse transform of Y_k.  For sample t, k = floor(t / H), i = t mod H:
 *      background[t] = (g_k[H + i] + g_{k+1}[i]) / d[i], the earlier frame first; foreground[t] = x[t] - background[t].
 *   8. No period: the background is +0 everywhere and the foreground is the input, bit for bit.
 * Samples are expected to be finite, a caller's V finite or +inf and not negative.
 *
 * Conventions: those of zen_hip.h and zen_hip_beat.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_repet_last_error() (this library's own thread-local message; failures of the library underneath are copied into
 * it).  All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  Everything is
 * allocated by zen_hip_repet_create, sized by the frame, n_clips and max_samples, never by a call.
 */
#ifndef ZEN_HIP_REPET_H
#define ZEN_HIP_REPET_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_repet* zen_hip_repet_t;

typedef struct zen_hip_repet_stats_t {
	unsigned long long calls;        /* separate and beat_spectrum calls since create, host calls included */
	unsigned long long clips;        /* clips separated since create */
	unsigned long long searches;     /* clips whose period was found by the call (one synchronisation per call that has any) */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the FFT handles' own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_repet_stats_t;

/* frame, fft, magnitude, lag_rows, lag_fft, power, braw, median, mask, ifft, overlap_add */
enum { ZEN_HIP_REPET_KERNELS = 11 };
/* counts up to REGISTER_SEGMENTS are sorted in registers, longer columns in LDS: the values are the same */
enum { ZEN_HIP_REPET_MAX_SEGMENTS = 256, ZEN_HIP_REPET_MAX_FRAMES = 16384, ZEN_HIP_REPET_REGISTER_SEGMENTS = 32 };
enum { ZEN_HIP_REPET_TABLE_WINDOW = 0 /* N values */, ZEN_HIP_REPET_TABLE_DIVISOR = 1 /* N / 2 values */ };

const char* zen_hip_repet_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_repet_version(void);

/* fs > 0; nfft: the frame N, a power of two in 64..8192; n_clips >= 1 rows separated by every call; max_samples >= 1: the
 * longest clip a call may bring, at most 16384 frames of it (ZEN_HIP_E_BAD_ARG otherwise, before a device is touched: the
 * lag transform of step 3 must fit the FFT wrapper's 32768 points).  create allocates everything, the transforms' own
 * included (each runs its largest batch once, on zeros): afterwards no call of the session allocates.  With m the frames
 * of max_samples and L its lag points that is n_clips m (8 N + 8 (N / 2 + 4)) + 8 (N / 2 + 1) L + 12 n_clips max_samples
 * bytes and a little more. */
int zen_hip_repet_create(float fs, size_t nfft, size_t n_clips, size_t max_samples, zen_hip_repet_t* h);
int zen_hip_repet_destroy(zen_hip_repet_t h);
int zen_hip_repet_set_stream(zen_hip_repet_t h, void* stream); /* waits for what the previous stream holds */
/* The period search looks at periods of tmin_s..tmax_s seconds (defaults 0.8 and 8); bins below highpass_hz go to the
 * background whole (default 100, 0 = off).  tmin_s > 0, tmax_s >= tmin_s, highpass_hz >= 0, all finite (ZEN_HIP_E_BAD_ARG). */
int zen_hip_repet_set_params(zen_hip_repet_t h, double tmin_s, double tmax_s, double highpass_hz);

/* Clip c is the n floats from in_dev + c * in_stride on, 1 <= n <= max_samples.  periods: NULL, or n_clips values in host
 * memory, the period of each clip in frames, 0 for "find it".  Each non-NULL output receives n_clips rows of n floats,
 * out_stride floats apart; either may be NULL.  periods_used: NULL, or room for n_clips values in host memory: the period
 * each clip was separated with, 0 where none was found (step 8).  braw_host: NULL, or host memory for n_clips rows of m
 * floats, braw_stride floats apart: the beat spectrum of every clip whose period the call found (the rows of the other
 * clips are left alone).
 * A period whose r = ceil(m / p) is outside 2..256, given or found: ZEN_HIP_E_UNSUPPORTED, and no output was touched.
 * Pointers need 4-byte alignment only; in_stride >= n, out_stride >= n where an output is asked for, braw_stride >= m
 * (ZEN_HIP_E_BAD_ARG otherwise, nothing is touched).  Nothing outside the named elements is written.  Asynchronous on the
 * handle's stream where every period is given; where one must be found the call waits for the beat spectra and returns
 * with the rest queued. */
int zen_hip_repet_separate_device(zen_hip_repet_t h, const float* in_dev, size_t in_stride, size_t n, const size_t* periods,
                                  float* background_dev, float* foreground_dev, size_t out_stride, size_t* periods_used, float* braw_host,
                                  size_t braw_stride);
/* The same rows in host memory: plain copies up and down around the device call.  Synchronous. */
int zen_hip_repet_separate_host(zen_hip_repet_t h, const float* in_host, size_t in_stride, size_t n, const size_t* periods,
                                float* background_host, float* foreground_host, size_t out_stride, size_t* periods_used, float* braw_host,
                                size_t braw_stride);
/* Steps 1-3 alone: braw_dev receives n_clips rows of m floats in device memory, braw_stride >= m floats apart.  Asynchronous. */
int zen_hip_repet_beat_spectrum_device(zen_hip_repet_t h, const float* in_dev, size_t in_stride, size_t n, float* braw_dev, size_t braw_stride);

/* The kernel of step 5 alone, on a caller's V: m rows of bins floats, v_stride floats apart, in device memory; s_dev receives
 * `period` rows of bins floats, s_stride floats apart.  No handle and no workspace; asynchronous on `stream` (a hipStream_t as
 * void*).  r = ceil(m / period) outside 2..256: ZEN_HIP_E_UNSUPPORTED; bins == 0, a stride below bins, a null or misaligned
 * (4 bytes) pointer: ZEN_HIP_E_BAD_ARG; nothing is touched either way.  16-byte accesses are used where both pointers are
 * 16-byte aligned and both strides multiples of 4, single words otherwise: the values are the same.  Nothing outside the
 * named elements is read or written. */
int zen_hip_repet_segment_median_device(const float* v_dev, size_t m, size_t bins, size_t v_stride, size_t period, float* s_dev, size_t s_stride,
                                        void* stream);

int zen_hip_repet_stats(zen_hip_repet_t h, zen_hip_repet_stats_t* out);

/* Profiling hooks for the harness (tools/ab_repet.py), as the beat library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step (the order of ZEN_HIP_REPET_KERNELS'
 * comment) milliseconds, bytes read + written, and launches. */
int zen_hip_repet_profile(zen_hip_repet_t h, int enable);
int zen_hip_repet_profile_get(zen_hip_repet_t h, double ms[ZEN_HIP_REPET_KERNELS], unsigned long long bytes[ZEN_HIP_REPET_KERNELS],
                              unsigned long long launches[ZEN_HIP_REPET_KERNELS]);

/* Step 4, on the host, without a device: braw of m lags -> *period in frames (0: none) and, where score is not NULL, its
 * J (0 where there is none).  braw NULL with m > 0 or period NULL: ZEN_HIP_E_BAD_ARG. */
int zen_hip_repet_find_period(const float* braw, size_t m, size_t jmin, size_t jmax, size_t* period, double* score);
/* One host table of the frame nfft, computed without a device: `which` is a ZEN_HIP_REPET_TABLE_* value.  out receives the
 * table's floats; cap, the floats out has room for, must be at least its length (ZEN_HIP_E_BAD_ARG otherwise, as for an
 * nfft create refuses and an unknown table). */
int zen_hip_repet_table(size_t nfft, int which, float* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_REPET_H */
