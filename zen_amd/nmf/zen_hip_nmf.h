/*
 * zen_hip_nmf.h -- supervised non-negative matrix factorisation of the magnitude spectrogram on device rows: two sources that
 * are both pitched, sustained and non-repeating, separated by their spectra (libzen_hip_nmf.so, linked against libzen_hip.so).
 *
 * The medians of HPR and the repetition of REPET / REPET-SIM cannot tell two instruments apart.  This library is the standard
 * answer (Lee and Seung, "Algorithms for Non-negative Matrix Factorization", NIPS 2001; Smaragdis and Brown, WASPAA 2003;
 * Virtanen, IEEE TASLP 15(3), 2007): V ~ H^T W with the Kullback-Leibler divergence and multiplicative updates.  A dictionary
 * of spectra W is learned per source from isolated material, held fixed on the mixture while only the activations H are
 * learned, and each dictionary's share of the model is a soft mask.  DESIGN.md section 20 states it in full and says what was
 * measured.
 *
 * The arithmetic (tests/nmf_model.py computes the same bits, tolerance 0).  Every float operation on the device is one of
 * + - * / sqrt fma max compare in float32, one rounding each; the two tables are those of zen_hip_repet.h, computed on the host
 * in double (libm cos) and rounded once to float32 -- zen_hip_nmf_table hands them out.
 *
 *   Parameters: fs; the frame N, a power of two in 64..8192, H = N / 2, F = H + 1 bins; K components, 1..256; n_clips >= 1
 *   rows of equal length, each factorised on its own.  A clip of n >= 1 samples has m = ceil(n / H) + 1 frames, m <= 16384.
 *   eps = 2^-40 as a float32.  Samples are expected finite, W and H finite and not negative.
 *
 *   1. xp = H zeros, the clip, zeros up to (m + 1) H samples.  Frame a is xp[a H .. a H + N); its row is (xp w, 0) with the
 *      periodic Hamming window w; X_a is the forward N-point transform of the row (zen_hip_fft_exec_batched).
 *   2. V[a][f] = sqrt(re re + im im), f < F.
 *      Steps 1 and 2 are those of zen_hip_repet.h bit for bit.
 *
 *   The segmented chain sdot(u, v) of operands u[0..L), v[0..L): the indices are cut into segments of 256 (the last may be
 *   shorter); in segment j, c_j = fma(u_l, v_l, ... fma(u_l0, v_l0, +0) ...) over l rising; the result is c_0 for one segment,
 *   otherwise ((c_0 + c_1) + c_2) + ... with float32 adds in rising order.  A plain sum is sdot with v = 1.  The segments are
 *   there so that a long reduction may be split over waves or workgroups without changing a bit.
 *
 *   Layouts: W is K rows of F floats, one spectrum per row; H is K rows of m floats; V, Q and the model L are m rows of F.
 *   The model: L[a][f] = sdot over k of (H[k][a], W[k][f]) -- one segment, a plain chain, since K <= 256.
 *
 *   One iteration, with fixed in 0..K the number of leading components whose spectra are held:
 *   3. Q[a][f] = V[a][f] / max(L[a][f], eps).
 *   4. P[k][a] = sdot over f of (W[k][f], Q[a][f]); s[k] = sdot over f of (W[k][f], 1);
 *      H'[k][a] = (H[k][a] P[k][a]) / max(s[k], eps), the product rounded before the division.
 *   5. If fixed < K: L and Q again with H'; then for k >= fixed only, G[k][f] = sdot over a of (H'[k][a], Q[a][f]),
 *      t[k] = sdot over a of (H'[k][a], 1), W'[k][f] = (W[k][f] G[k][f]) / max(t[k], eps).
 *
 *   Stems: the caller gives group[k] in -1..G-1 and G in 1..K.  After the last iteration L is taken with the final W and H;
 *   L_g[a][f] is the chain over the k with group[k] = g, in rising k, from +0; M_g = L_g / L where L > 0, else +0;
 *   Y_a[f] = (re M_g, im M_g) for f <= H, Y_a[N - f] = (re_{N-f} M_g[f], im_{N-f} M_g[f]) for 0 < f < H; g_a = the real part of
 *   the unnormalised inverse transform of Y_a; for sample s, a = floor(s / H), i = s mod H:
 *   stem_g[s] = (g_a[H + i] + g_{a+1}[i]) / d[i], the earlier frame first, d[i] = float32(N ((double)w[i] + (double)w[i + H])):
 *   zen_hip_repet.h's step 7.  A component of group -1 is in no stem.
 *
 *   Initial values: zen_hip_nmf_init(seed, count, out) is splitmix64.  For value i: z = seed + (i + 1) 0x9E3779B97F4A7C15 mod
 *   2^64; z = (z ^ (z >> 30)) 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) 0x94D049BB133111EB; z = z ^ (z >> 31); the value is
 *   float32((z >> 40) + 1) 2^-24: in (0, 1] and exact.  The binding and the demo take W from `seed` and H from `seed + 1`.
 *
 * Steps 3, 4 and 5 are three matrix products with their divisions as epilogues, each on two routes that give the same bits:
 * the matrix cores (v_mfma_f32_32x32x2_f32, whose sum over k is the fma chain above; a new segment starts a fresh
 * accumulator) and the vector ALU (the chain written out).  ZEN_HIP_NMF="mfma=0" in the environment of zen_hip_nmf_create
 * sends a session down the vector route ("mfma=1": the matrix cores); DESIGN.md section 20 says which is the default.
 *
 * Conventions: those of zen_hip.h and zen_hip_repsim.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_nmf_last_error() (this library's own thread-local message; failures of the library underneath are copied into it).
 * All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  Everything is allocated by
 * zen_hip_nmf_create, never by a call.
 */
#ifndef ZEN_HIP_NMF_H
#define ZEN_HIP_NMF_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_nmf* zen_hip_nmf_t;

typedef struct zen_hip_nmf_stats_t {
	unsigned long long calls;        /* process calls since create, host calls included */
	unsigned long long clips;        /* clips factorised since create */
	unsigned long long iterations;   /* iterations run since create, summed over the clips */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the FFT handle's own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_nmf_stats_t;

/* frame, fft, magnitude, ratio_mfma, ratio_valu, update_h_mfma, update_h_valu, update_w_mfma, update_w_valu, mask, ifft,
 * overlap_add */
enum { ZEN_HIP_NMF_KERNELS = 12 };
enum { ZEN_HIP_NMF_MAX_COMPONENTS = 256, ZEN_HIP_NMF_MAX_FRAMES = 16384, ZEN_HIP_NMF_SEGMENT = 256 };
enum { ZEN_HIP_NMF_TABLE_WINDOW = 0 /* N values */, ZEN_HIP_NMF_TABLE_DIVISOR = 1 /* N / 2 values */ };
enum { ZEN_HIP_NMF_ROUTE_DEFAULT = 0, ZEN_HIP_NMF_ROUTE_MFMA = 1, ZEN_HIP_NMF_ROUTE_VALU = 2 };
/* A session splits the reductions of steps 4 and 5 by segments over workgroups, through a scratch for the segments' sums of
 * at most this many bytes; an update whose sums would not fit walks its segments in sequence.  The bits are the same. */
#define ZEN_HIP_NMF_SPLIT_BYTES ((size_t)128 << 20)

const char* zen_hip_nmf_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_nmf_version(void);

/* fs > 0; nfft: the frame N, a power of two in 64..8192; components: K in 1..256; n_clips >= 1 rows factorised by every
 * call; max_samples >= 1: the longest clip a call may bring, at most 16384 frames of it (ZEN_HIP_E_BAD_ARG otherwise, before a
 * device is touched).  create allocates everything, the transform's own included (it runs its largest batch once, on zeros):
 * afterwards no call of the session allocates.  With m the frames of max_samples and F4 = F rounded up to 4 that is
 *   n_clips m (8 N + 4 F4)                 the spectra X and V
 *   + m (8 N + 4 F4)                       the masked spectra of one stem, and Q of the clip at hand
 *   + 4 n_clips K (F4 + m)                 the host calls' W and H
 *   + 8 n_clips max_samples                the host calls' rows in and one group's rows out
 *   + 4 K max(ceil(F / 256) m, ceil(m / 256) F)   the segments' sums (each of the two counted only if within SPLIT_BYTES)
 * bytes and a little more (the two tables, the segments' row sums). */
int zen_hip_nmf_create(float fs, size_t nfft, size_t components, size_t n_clips, size_t max_samples, zen_hip_nmf_t* h);
int zen_hip_nmf_destroy(zen_hip_nmf_t h);
int zen_hip_nmf_set_stream(zen_hip_nmf_t h, void* stream); /* waits for what the previous stream holds */

/* Clip c is the n floats from in_dev + c * in_stride on, 1 <= n <= max_samples.  Its dictionary is the K rows of F floats,
 * w_stride floats apart, from w_dev + c * w_clip_stride on; its activations the K rows of m floats, h_stride apart, from
 * h_dev + c * h_clip_stride on.  Both are read as the initial values and left as the results of `iterations` >= 0 iterations
 * with the first `fixed` (0..K) spectra held.  w_clip_stride == 0 (one dictionary for every clip) is allowed only with
 * fixed == K: otherwise the clips would race on W, and the call is refused.
 * groups_host: NULL (a fit only: n_groups, stems_dev and out_stride are not looked at), or K ints in -1..n_groups-1 with
 * n_groups in 1..K; stems_dev then receives n_groups * n_clips rows of n floats, row g * n_clips + c starting out_stride
 * floats behind the one before.  Pointers need 4-byte alignment only: 16-byte loads are used where a pointer is 16-byte
 * aligned and its stride a multiple of 4, single words otherwise, and the values are the same.  in_stride >= n,
 * w_stride >= F, h_stride >= m, out_stride >= n, the clip strides at least their clip (ZEN_HIP_E_BAD_ARG otherwise, nothing
 * is touched).  Nothing outside the named elements is read or written.  Asynchronous on the handle's stream. */
int zen_hip_nmf_process_device(zen_hip_nmf_t h, const float* in_dev, size_t in_stride, size_t n, float* w_dev, size_t w_stride,
                               size_t w_clip_stride, float* h_dev, size_t h_stride, size_t h_clip_stride, size_t fixed, int iterations,
                               const int* groups_host, size_t n_groups, float* stems_dev, size_t out_stride);
/* The same with in, W, H and the stems in host memory: plain copies up and down around the device call.  Synchronous. */
int zen_hip_nmf_process_host(zen_hip_nmf_t h, const float* in_host, size_t in_stride, size_t n, float* w_host, size_t w_stride,
                             size_t w_clip_stride, float* h_host, size_t h_stride, size_t h_clip_stride, size_t fixed, int iterations,
                             const int* groups_host, size_t n_groups, float* stems_host, size_t out_stride);

/* The three products alone, on a caller's device memory.  No handle and no workspace; asynchronous on `stream` (a hipStream_t
 * as void*).  components in 1..256, bins >= 1, frames in 1..16384; a null or misaligned (4 bytes) pointer, a stride below its
 * row, a route that is no ZEN_HIP_NMF_ROUTE_* value: ZEN_HIP_E_BAD_ARG, and nothing is touched.  W is `components` rows of
 * `bins` floats, H `components` rows of `frames`, V, Q and L `frames` rows of `bins`.
 *
 * Step 3: Q from V, W and H; lam_dev: NULL, or L is written there as well. */
int zen_hip_nmf_ratio_device(const float* v_dev, size_t v_stride, const float* w_dev, size_t w_stride, const float* h_dev, size_t h_stride,
                             size_t components, size_t bins, size_t frames, float* q_dev, size_t q_stride, float* lam_dev, size_t lam_stride,
                             int route, void* stream);
/* Step 4: H' from W, Q and H.  out_dev may be h_dev. */
int zen_hip_nmf_update_h_device(const float* w_dev, size_t w_stride, const float* q_dev, size_t q_stride, const float* h_dev, size_t h_stride,
                                size_t components, size_t bins, size_t frames, float* out_dev, size_t out_stride, int route, void* stream);
/* Step 5's second half: W' from H, Q and W for the rows from `fixed` (0..components) on; the rows below are not touched.
 * out_dev may be w_dev. */
int zen_hip_nmf_update_w_device(const float* h_dev, size_t h_stride, const float* q_dev, size_t q_stride, const float* w_dev, size_t w_stride,
                                size_t components, size_t bins, size_t frames, size_t fixed, float* out_dev, size_t out_stride, int route,
                                void* stream);

int zen_hip_nmf_stats(zen_hip_nmf_t h, zen_hip_nmf_stats_t* out);

/* Profiling hooks for the harness (tools/ab_nmf.py), as the repsim library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step (the order of ZEN_HIP_NMF_KERNELS'
 * comment; the route that did not run stays at zero) milliseconds, bytes read + written, and launches. */
int zen_hip_nmf_profile(zen_hip_nmf_t h, int enable);
int zen_hip_nmf_profile_get(zen_hip_nmf_t h, double ms[ZEN_HIP_NMF_KERNELS], unsigned long long bytes[ZEN_HIP_NMF_KERNELS],
                            unsigned long long launches[ZEN_HIP_NMF_KERNELS]);

/* `count` initial values from `seed` into host memory (the generator above).  Touches no device. */
int zen_hip_nmf_init(unsigned long long seed, size_t count, float* out);
/* One host table of the frame nfft, computed without a device: `which` is a ZEN_HIP_NMF_TABLE_* value.  out receives the
 * table's floats; cap, the floats out has room for, must be at least its length (ZEN_HIP_E_BAD_ARG otherwise, as for an nfft
 * create refuses and an unknown table). */
int zen_hip_nmf_table(size_t nfft, int which, float* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_NMF_H */
