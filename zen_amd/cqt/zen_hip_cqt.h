/*
 * zen_hip_cqt.h -- an invertible constant-Q transform on device rows, and the harmonic / percussive / residual separation
 * in its domain (libzen_hip_cqt.so, linked against libzen_hip.so).
 *
 * The separations of zen_hip.h filter an STFT, whose bins are equally wide.  Here the bands are spaced geometrically, B to the
 * octave, as pitches are: the transform is a sliced non-stationary Gabor transform in matrix form (overlapping slices of the
 * signal; in each, raised-cosine bands on the spectrum; every band brought down to the same M coefficients per slice), built
 * from its definition and exactly invertible.  On top of it sits the single-pass median-filtering separation (Fitzgerald
 * 2010; Driedger, Mueller and Disch 2014 for the residual) in that domain.  DESIGN.md section 18 states the construction and
 * says what was measured.
 *
 * The arithmetic (tests/cqt_model.py computes the same bits).  Every float operation on the device is one of + - * / sqrt
 * compare in float32, one rounding each; everything transcendental is a table computed on the host in double (libm cos, pow)
 * and rounded once to float32 -- zen_hip_cqt_plan and zen_hip_cqt_table hand them out.  The transforms are
 * zen_hip_fft_exec_batched, the medians zen_hip_mfilt_run.
 *
 *   Parameters: fs > 0; the slice Ls, a power of two in 64..32768, N = Ls / 2; B bands per octave, 1..96; fmin > 0;
 *   n_clips >= 1 rows of exactly n_samples >= 1 samples each (fixed at create: the median handles are sized by it).
 *
 *   Band centres, in bins of the slice, integers from doubles: r = 2^(1/B), wmin = 4; p[0] = 0;
 *   p[1] = max(wmin, floor(fmin Ls / fs + 0.5)); p[k+1] = max(p[k] + wmin, floor(p[k] r + 0.5)) for as long as that is
 *   <= N - wmin; the last centre is N.  Constant-Q above the corner where a band is wmin bins wide, linear below it, with a DC
 *   band and a Nyquist band.  nb is the number of centres; fewer than 3 is ZEN_HIP_E_BAD_ARG.
 *
 *   Band windows: band k rises as 0.5 - 0.5 cos(pi (b - p[k-1]) / (p[k] - p[k-1])) on p[k-1] <= b <= p[k] and falls as
 *   0.5 + 0.5 cos(pi (b - p[k]) / (p[k+1] - p[k])) on p[k] <= b <= p[k+1]; band 0 only falls, the last band only rises.  Every
 *   bin 0 <= b <= N lies in at most two bands: the lower band kb[b] with p[kb] <= b < p[kb+1] (for b = N the last band) and
 *   the upper band kb + 1, absent at a centre.  The tables are per bin: kb[b], gL[b], gU[b] (float32, gU = 0 at centres) and
 *   the duals gdL, gdU: M = the smallest power of two >= max(32, max_k (p[k+1] - p[k-1] - 1)) (p[-1] = p[0], p[nb] = p[nb-1]),
 *   gd = float32(g / (M (gL gL + gU gU))) with the float32 g's taken to double.
 *
 *   Slice windows: h[i] = 0.5 - 0.5 cos(2 pi i / Ls) (it sums to 1 at hop N), rounded to float32;
 *   s[i] = float32((h[i] / (h[i] h[i] + h[(i + N) mod Ls] h[(i + N) mod Ls])) / Ls), all of it in double.
 *
 *   Per clip of n samples: ns = ceil(n / N) + 1 slices, ns <= 4096; T = (ns + 1) M / 2 columns.
 *   1. xp = N zeros, the clip, zeros up to (ns + 1) N samples.  Slice q is xp[q N .. q N + Ls); its row is (xp h, 0); F_q is
 *      the forward Ls-point transform.
 *   2. For band k the row of M complex values is +0 everywhere except: for every bin b of the band (p[k-1] < b < p[k+1],
 *      clipped to [0, N]), buf[b mod M] = (F.re g, F.im g), g band k's weight at b.  c_q[k] is the unnormalised inverse
 *      M-point transform of the row.  The index is the absolute bin mod M, not the bin relative to the centre: with a centred
 *      index neighbouring slices of an odd-centred band meet with opposite sign and cancel in step 3.
 *   3. Column t = q M / 2 + m of the clip's matrix: A[t][k] = c_{q-1}[k][m + M / 2] + c_q[k][m] per component, the earlier
 *      slice first; where only one slice exists its value alone.  V[t][k] = sqrt(re re + im im): T rows of nb floats.
 *   4. H = the median of V over lh columns of time (ZEN_HIP_TIME_ANTICAUSAL), P = the median over lp bands
 *      (ZEN_HIP_FREQUENCY); centred, odd, replicate border, as everywhere in zen_hip.h.  Default lh: 0.2 s of columns,
 *      floor(0.2 fs M / Ls), made odd upward, clamped to T; default lp: one octave of bands, B made odd upward, clamped to nb.
 *   5. Masks, beta in float32.  Hard (default, beta >= 1): harmonic where H > beta P; otherwise percussive where P >= beta H;
 *      otherwise residual; each mask 1.0f or 0.0f.  Soft: d = H H + P P; mh = H H / d and mp = P P / d where d > 0, both 0
 *      elsewhere; the residual stem is then +0.
 *   6. Per stem c'_q[k][m] = (re m_, im m_), m_ the mask at column q M / 2 + m, band k; G the forward M-point transform of each
 *      row.  For 0 <= b <= N: Y[b] = G_kb[b mod M] gdL[b] at a centre, otherwise G_kb[b mod M] gdL[b] + G_{kb+1}[b mod M] gdU[b]
 *      per component, the lower band first; the imaginary parts of Y[0] and Y[N] are +0; Y[Ls - b] = (re, -im) of Y[b] for
 *      0 < b < N.  y_q = the real part of the unnormalised inverse Ls-point transform.
 *   7. Sample t, q = floor(t / N), i = t mod N: out[t] = y_q[N + i] s[N + i] + y_{q+1}[i] s[i], the earlier slice first.
 * Samples are expected to be finite.
 *
 * Conventions: those of zen_hip.h and zen_hip_repet.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_cqt_last_error() (this library's own thread-local message; failures of the library underneath are copied into it).
 * All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  Everything is allocated by
 * zen_hip_cqt_create, never by a call.  The coefficients are the big object (ns nb M 8 bytes per clip) and are kept once: a
 * stem goes through a scratch of a bounded run of slices (32 MiB, one slice at the least), not through a copy of its own.
 */
#ifndef ZEN_HIP_CQT_H
#define ZEN_HIP_CQT_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_cqt* zen_hip_cqt_t;

typedef struct zen_hip_cqt_stats_t {
	unsigned long long calls;        /* forward, spectrogram, inverse and separate calls since create, host calls included */
	unsigned long long clips;        /* clips separated since create */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the FFT handles' own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_cqt_stats_t;

typedef struct zen_hip_cqt_shape_t {
	size_t slices;  /* ns */
	size_t bands;   /* nb */
	size_t m;       /* M: coefficients per band and slice */
	size_t columns; /* T */
	size_t run;     /* slices a stem's scratch holds */
	size_t lh, lp;  /* the median lengths in use */
} zen_hip_cqt_shape_t;

/* slice, slice_fft, fold, band_ifft, overlap, median_time, median_freq, mask, band_fft, gather, slice_ifft, overlap_add */
enum { ZEN_HIP_CQT_KERNELS = 12 };
enum { ZEN_HIP_CQT_MAX_SLICES = 4096, ZEN_HIP_CQT_MAX_BANDS_PER_OCTAVE = 96 };
/* KB: N + 1 ints; GL, GU, GDL, GDU: N + 1 floats; H, S: Ls floats */
enum { ZEN_HIP_CQT_TABLE_KB = 0, ZEN_HIP_CQT_TABLE_GL = 1, ZEN_HIP_CQT_TABLE_GU = 2, ZEN_HIP_CQT_TABLE_GDL = 3, ZEN_HIP_CQT_TABLE_GDU = 4,
       ZEN_HIP_CQT_TABLE_H = 5, ZEN_HIP_CQT_TABLE_S = 6 };

const char* zen_hip_cqt_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_cqt_version(void);

/* The plan of (fs, slice, bands_per_octave, fmin), on the host without a device: *nb and *m where not NULL, and where centres
 * is not NULL the nb centres (cap, the ints it has room for, must be at least nb).  A slice that is no power of two in
 * 64..32768, fs or fmin not positive and finite, bands_per_octave outside 1..96, fewer than 3 bands: ZEN_HIP_E_BAD_ARG. */
int zen_hip_cqt_plan(float fs, size_t slice, int bands_per_octave, double fmin, size_t* nb, size_t* m, int* centres, size_t cap);
/* One host table of that plan, computed without a device: `which` is a ZEN_HIP_CQT_TABLE_* value, cap the values out has
 * room for (at least the table's length; ZEN_HIP_E_BAD_ARG otherwise, as for a plan that is refused and an unknown table). */
int zen_hip_cqt_table(float fs, size_t slice, int bands_per_octave, double fmin, int which, void* out, size_t cap);

/* n_clips >= 1 rows of n_samples >= 1 samples, separated or transformed by every call.  Refused before a device is touched
 * (ZEN_HIP_E_BAD_ARG): what zen_hip_cqt_plan refuses, and a clip of more than 4096 slices; ZEN_HIP_E_UNSUPPORTED: T, nb or
 * T nb beyond the int of zen_hip_mfilt_create, n_clips ns nb beyond one batched transform.  create allocates everything, the
 * transforms' and medians' own included (each runs its largest batch once, on zeros): afterwards no call of the session
 * allocates.  With run = min(ns, max(1, 2^22 / (nb M))) that is
 *   n_clips ns (8 Ls + 8 nb M) + 8 run nb M + 12 T nb + 16 (N + 1) + 8 Ls + 4 (N + 1 + nb) + 16 n_clips n_samples
 * bytes in 12 allocations. */
int zen_hip_cqt_create(float fs, size_t slice, int bands_per_octave, double fmin, size_t n_clips, size_t n_samples, zen_hip_cqt_t* h);
int zen_hip_cqt_destroy(zen_hip_cqt_t h);
int zen_hip_cqt_set_stream(zen_hip_cqt_t h, void* stream); /* waits for what the previous stream holds */
/* beta: 0 for the default 2, else finite and >= 1; soft != 0: the soft masks; lh, lp: the median lengths in columns and in
 * bands, 0 for the defaults of step 4.  A length above its dimension: ZEN_HIP_E_FILTER_TOO_BIG; a negative one or a bad
 * beta: ZEN_HIP_E_BAD_ARG; the handle keeps what it had.  New lengths wait for the stream and replace the median handles. */
int zen_hip_cqt_set_params(zen_hip_cqt_t h, float beta, int soft, int lh, int lp);
int zen_hip_cqt_shape(zen_hip_cqt_t h, zen_hip_cqt_shape_t* out);
int zen_hip_cqt_stats(zen_hip_cqt_t h, zen_hip_cqt_stats_t* out);

/* Clip c is the n_samples floats from in_dev + c * in_stride on, in_stride >= n_samples.  Pointers need 4-byte alignment
 * only (the overlap-add of step 7 stores 16 bytes at a time where a row of the output is 16-byte aligned, single words
 * otherwise: the values are the same).  Nothing outside the named elements is read or written; a bad argument
 * (ZEN_HIP_E_BAD_ARG: a null handle or input, a misaligned pointer, a stride below the row) touches nothing.  The device
 * calls are asynchronous on the handle's stream.
 *
 * forward: steps 1-2.  coef_dev receives, clip after clip, ns * nb * M interleaved complex floats: c_q[k][m] of a clip at
 * ((q * nb + k) * M + m) * 2. */
int zen_hip_cqt_forward_device(zen_hip_cqt_t h, const float* in_dev, size_t in_stride, float* coef_dev);
/* steps 1-3.  v_dev receives, clip after clip, T rows of nb floats, v_stride >= nb floats apart. */
int zen_hip_cqt_spectrogram_device(zen_hip_cqt_t h, const float* in_dev, size_t in_stride, float* v_dev, size_t v_stride);
/* steps 6-7 with the mask identically 1, from a caller's coefficients in the layout of forward: out_dev receives n_clips
 * rows of n_samples floats, out_stride floats apart.  inverse(forward(x)) is x to float32 rounding. */
int zen_hip_cqt_inverse_device(zen_hip_cqt_t h, const float* coef_dev, float* out_dev, size_t out_stride);
/* steps 1-7.  Each non-NULL output receives n_clips rows of n_samples floats, out_stride >= n_samples floats apart; an
 * output that is NULL is not synthesised. */
int zen_hip_cqt_separate_device(zen_hip_cqt_t h, const float* in_dev, size_t in_stride, float* harmonic_dev, float* percussive_dev,
                                float* residual_dev, size_t out_stride);
/* The same rows in host memory: plain copies up and down around the device call.  Synchronous. */
int zen_hip_cqt_separate_host(zen_hip_cqt_t h, const float* in_host, size_t in_stride, float* harmonic_host, float* percussive_host,
                              float* residual_host, size_t out_stride);

/* Profiling hooks for the harness (tools/ab_cqt.py), as the repet library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step (the order of ZEN_HIP_CQT_KERNELS'
 * comment) milliseconds, bytes read + written, and launches. */
int zen_hip_cqt_profile(zen_hip_cqt_t h, int enable);
int zen_hip_cqt_profile_get(zen_hip_cqt_t h, double ms[ZEN_HIP_CQT_KERNELS], unsigned long long bytes[ZEN_HIP_CQT_KERNELS],
                            unsigned long long launches[ZEN_HIP_CQT_KERNELS]);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_CQT_H */
