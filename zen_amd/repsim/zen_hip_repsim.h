/*
 * zen_hip_repsim.h -- REPET-SIM on device rows: the repeating background of a recording against its foreground where the
 * repetition has no single period (libzen_hip_repsim.so, linked against libzen_hip.so).
 *
 * zen_hip_repet.h assumes one period for the whole clip.  This library is the same authors' answer for everything else
 * (Rafii and Pardo, "Music/Voice Separation Using the Similarity Matrix", ISMIR 2012): for every frame it finds the frames
 * that look most like it, from the cosine-similarity matrix of the spectrogram, takes the median over those frames, builds
 * the soft mask from that median and resynthesises through the mask.  DESIGN.md section 19 states it in full and says what
 * was measured.
 *
 * The arithmetic (tests/repsim_model.py computes the same bits).  Every float operation on the device is one of + - * /
 * sqrt fma min compare in float32, one rounding each; the two tables are those of zen_hip_repet.h, computed on the host in
 * double (libm cos) and rounded once to float32 -- zen_hip_repsim_table hands them out.
 *
 *   Parameters: fs; the frame N, a power of two in 64..8192, H = N / 2, bins = H + 1; n_clips >= 1 rows of equal length,
 *   each separated on its own.  A clip of n >= 1 samples has m = ceil(n / H) + 1 frames, m <= 16384.  The selection: a
 *   threshold t in [0, 1), a minimum distance dd = max(1, ceil(d_s fs / H)) frames, a number k in 1..256.
 *   Tables: the periodic Hamming window w[i] = 0.54 - 0.46 cos(2 pi i / N); d[i] = float32(N ((double)w[i] + (double)w[i + H])).
 *
 *   1. xp = H zeros, the clip, zeros up to (m + 1) H samples.  Frame a is xp[a H .. a H + N); its row is (xp w, 0); X_a is
 *      the forward N-point transform of the row (zen_hip_fft_exec_batched).
 *   2. V[a][f] = sqrt(re re + im im), f < bins.
 *   3. D[a][b] = fma(V[a][bins-1], V[b][bins-1], ... fma(V[a][1], V[b][1], fma(V[a][0], V[b][0], +0)) ...): a float32 fma
 *      chain over the bins in rising order, one rounding per link; it is symmetric in a, b bit for bit.
 *      nrm[a] = sqrt(D[a][a]); den = nrm[a] nrm[b]; S[a][b] = D[a][b] / den where den > 0, else +0.
 *   4. Per frame a the candidates are the b < m with S[a][b] > (float)t (a NaN never is one).  Until k frames are accepted
 *      or no candidate is left: accept the first index j of the largest candidate, remove every b with |b - j| < dd.
 *      idx[a][0..c_a) are the accepted frames in order of acceptance, c_a in 0..k.  The frame a itself is a frame like any.
 *   5. U[a][f] = the median of V[idx[a][q]][f], q < c_a: sorted s[0..c), s[(c - 1) / 2] for odd c, (s[c / 2 - 1] + s[c / 2])
 *      * 0.5f for even c; +0 where c_a = 0.
 *   6. W = min(U[a][f], V[a][f]); M = W / V where V > 0, else 0; with a high-pass cut-off fc > 0, kc = ceil(fc N / fs) in
 *      double and M = 1 for f < kc.  Y_a[f] = (re M, im M) for f <= H, Y_a[N - f] = (re_{N-f} M[f], im_{N-f} M[f]) for
 *      0 < f < H.
 *   7. g_a = the real part of the unnormalised inverse transform of Y_a.  For sample s, a = floor(s / H), i = s mod H:
 *      background[s] = (g_a[H + i] + g_{a+1}[i]) / d[i], the earlier frame first; foreground[s] = x[s] - background[s].
 * Steps 1, 2 and 7 are those of zen_hip_repet.h bit for bit.  Samples are expected to be finite.
 *
 * Step 3 has two routes that give the same bits: the matrix cores (v_mfma_f32_32x32x2_f32, whose sum over k is the fma
 * chain above) and the vector ALU (the chain written out).  ZEN_HIP_REPSIM="mfma=0" in the environment of
 * zen_hip_repsim_create sends a session down the vector route ("mfma=1": the matrix cores); DESIGN.md section 19 says which
 * one is the default and why.  "band=R" there (options are separated by commas) makes the bands of S R rows, rounded up to
 * 128, where that is fewer than the session would take: the results are the same.
 *
 * Conventions: those of zen_hip.h and zen_hip_repet.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_repsim_last_error() (this library's own thread-local message; failures of the library underneath are copied
 * into it).  All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  Everything is
 * allocated by zen_hip_repsim_create, sized by the frame, n_clips and max_samples, never by a call.
 */
#ifndef ZEN_HIP_REPSIM_H
#define ZEN_HIP_REPSIM_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_repsim* zen_hip_repsim_t;

typedef struct zen_hip_repsim_stats_t {
	unsigned long long calls;        /* separate calls since create, host calls included */
	unsigned long long clips;        /* clips separated since create */
	unsigned long long bands;        /* bands of rows of S computed and selected from since create */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the FFT handle's own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_repsim_stats_t;

/* frame, fft, magnitude, similarity_mfma, similarity_valu, select, gather_median, mask, ifft, overlap_add */
enum { ZEN_HIP_REPSIM_KERNELS = 10 };
/* counts up to REGISTER_NEIGHBOURS are sorted in registers, longer columns searched by rank in LDS: the values are the same */
enum { ZEN_HIP_REPSIM_MAX_NEIGHBOURS = 256, ZEN_HIP_REPSIM_MAX_FRAMES = 16384, ZEN_HIP_REPSIM_REGISTER_NEIGHBOURS = 32 };
enum { ZEN_HIP_REPSIM_TABLE_WINDOW = 0 /* N values */, ZEN_HIP_REPSIM_TABLE_DIVISOR = 1 /* N / 2 values */ };
enum { ZEN_HIP_REPSIM_ROUTE_DEFAULT = 0, ZEN_HIP_REPSIM_ROUTE_MFMA = 1, ZEN_HIP_REPSIM_ROUTE_VALU = 2 };
/* S never exists whole: a session computes it and selects from it a band of rows at a time, through a scratch of at most
 * this many bytes (and at least 128 rows) */
#define ZEN_HIP_REPSIM_BAND_BYTES ((size_t)64 << 20)

const char* zen_hip_repsim_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_repsim_version(void);

/* fs > 0; nfft: the frame N, a power of two in 64..8192; n_clips >= 1 rows separated by every call; max_samples >= 1: the
 * longest clip a call may bring, at most 16384 frames of it (ZEN_HIP_E_BAD_ARG otherwise, before a device is touched).
 * create allocates everything, the transform's own included (it runs its largest batch once, on zeros): afterwards no call
 * of the session allocates.  With m the frames of max_samples, m4 = m rounded up to 4 and the band r = min(m rounded up to
 * 128, max(128, BAND_BYTES / (4 m4) rounded down to 128)) rows that is
 *   n_clips m (8 N + 4 (N / 2 + 4))   the spectra and V
 *   + 4 m (N / 2 + 4)                 U of the clip at hand
 *   + 4 r m4                          the band of S
 *   + 4 n_clips m (256 + 1)           idx and counts
 *   + 12 n_clips max_samples          the host calls' rows
 * bytes and a little more. */
int zen_hip_repsim_create(float fs, size_t nfft, size_t n_clips, size_t max_samples, zen_hip_repsim_t* h);
int zen_hip_repsim_destroy(zen_hip_repsim_t h);
int zen_hip_repsim_set_stream(zen_hip_repsim_t h, void* stream); /* waits for what the previous stream holds */
/* The selection of step 4 and the high-pass of step 6.  threshold in [0, 1) (default 0); distance_s >= 0 seconds between
 * two accepted frames (default 1; anything below one frame is one frame); number in 1..256 (default 100); bins below
 * highpass_hz go to the background whole (default 100, 0 = off).  All finite (ZEN_HIP_E_BAD_ARG, and nothing is changed). */
int zen_hip_repsim_set_params(zen_hip_repsim_t h, double threshold, double distance_s, size_t number, double highpass_hz);

/* Clip c is the n floats from in_dev + c * in_stride on, 1 <= n <= max_samples.  Each non-NULL output receives n_clips rows
 * of n floats, out_stride floats apart; either may be NULL.  counts_dev: NULL, or device memory for n_clips * m int32, c_a
 * of every frame, clip by clip.  indices_dev: NULL, or device memory for n_clips * m * k int32, idx[a][0..k) of every frame
 * with -1 from c_a on.  Pointers need 4-byte alignment only; in_stride >= n, out_stride >= n where an output is asked for
 * (ZEN_HIP_E_BAD_ARG otherwise, nothing is touched).  Nothing outside the named elements is written.  Asynchronous on the
 * handle's stream. */
int zen_hip_repsim_separate_device(zen_hip_repsim_t h, const float* in_dev, size_t in_stride, size_t n, float* background_dev,
                                   float* foreground_dev, size_t out_stride, int* counts_dev, int* indices_dev);
/* The same rows, counts and indices in host memory: plain copies up and down around the device call.  Synchronous. */
int zen_hip_repsim_separate_host(zen_hip_repsim_t h, const float* in_host, size_t in_stride, size_t n, float* background_host,
                                 float* foreground_host, size_t out_stride, int* counts_host, int* indices_host);

/* The three kernels alone, on a caller's device memory.  No handle and no workspace; asynchronous on `stream` (a hipStream_t
 * as void*).  A null or misaligned (4 bytes) pointer, m == 0 or above 16384, bins == 0, a stride below its row:
 * ZEN_HIP_E_BAD_ARG, and nothing is touched.  16-byte loads are used where a pointer is 16-byte aligned and its stride a
 * multiple of 4, single words otherwise: the values are the same.  Nothing outside the named elements is read or written.
 *
 * Step 3: V is m rows of bins floats, v_stride floats apart, any finite values (negative ones included); s_dev receives m
 * rows of m floats, s_stride floats apart.  route: a ZEN_HIP_REPSIM_ROUTE_* value (ZEN_HIP_E_BAD_ARG for any other). */
int zen_hip_repsim_similarity_device(const float* v_dev, size_t m, size_t bins, size_t v_stride, float* s_dev, size_t s_stride, int route,
                                     void* stream);
/* Step 4 on a caller's S (m rows of m floats, any values): idx_dev receives m rows of `number` int32 (-1 from c_a on),
 * counts_dev m int32.  threshold is compared as given (any float that is not a NaN); distance >= 1 frames; number in 1..256. */
int zen_hip_repsim_select_device(const float* s_dev, size_t m, size_t s_stride, float threshold, size_t distance, size_t number, int* idx_dev,
                                 int* counts_dev, void* stream);
/* Step 5 on a caller's V (m rows), idx (`rows` rows of `number` int32) and counts (`rows` int32): u_dev receives `rows` rows
 * of bins floats, u_stride floats apart.  V finite or +inf and not negative (no -0).  rows in 1..16384, number in 1..256; a
 * count is taken as min(max(count, 0), number) and an index as min(max(index, 0), m - 1), so that nothing outside V is read. */
int zen_hip_repsim_gather_median_device(const float* v_dev, size_t m, size_t bins, size_t v_stride, const int* idx_dev, const int* counts_dev,
                                        size_t rows, size_t number, float* u_dev, size_t u_stride, void* stream);

int zen_hip_repsim_stats(zen_hip_repsim_t h, zen_hip_repsim_stats_t* out);

/* Profiling hooks for the harness (tools/ab_repsim.py), as the repet library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step (the order of ZEN_HIP_REPSIM_KERNELS'
 * comment; the similarity route that did not run stays at zero) milliseconds, bytes read + written, and launches. */
int zen_hip_repsim_profile(zen_hip_repsim_t h, int enable);
int zen_hip_repsim_profile_get(zen_hip_repsim_t h, double ms[ZEN_HIP_REPSIM_KERNELS], unsigned long long bytes[ZEN_HIP_REPSIM_KERNELS],
                               unsigned long long launches[ZEN_HIP_REPSIM_KERNELS]);

/* One host table of the frame nfft, computed without a device: `which` is a ZEN_HIP_REPSIM_TABLE_* value.  out receives the
 * table's floats; cap, the floats out has room for, must be at least its length (ZEN_HIP_E_BAD_ARG otherwise, as for an
 * nfft create refuses and an unknown table). */
int zen_hip_repsim_table(size_t nfft, int which, float* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_REPSIM_H */
