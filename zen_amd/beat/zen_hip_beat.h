/*
 * zen_hip_beat.h -- beat tracking on device rows: the complex-domain onset function and the cumulative-score beat tracker
 * of Stark, Davies and Plumbley (libzen_hip_beat.so, linked against libzen_hip.so).
 *
 * The reference's third use of its separations (demos/beat-tracking: a beat tracker behind the percussive stream).  A
 * session takes rows of samples that already are in device memory -- the percussive rows a zen_hip_hpr_process call has
 * just written, for one -- and gives four values per hop: the onset function, the cumulative score, a beat flag and the
 * tempo in force, without a trip to the host.  The method is the published one (DAFx 2009, IEEE TASLP 2007; the
 * complex-domain onset function of Bello et al. and Duxbury et al.); DESIGN.md section 15 states it in full and lists
 * where it departs from the demo.
 *
 * The arithmetic (tests/beat_model.py computes the same bits).  Every float operation on the device is one of + - * /
 * sqrt max compare in float32, one rounding each; everything transcendental is a table computed on the host in double
 * (libm exp, log, cos, sqrt) and rounded once to float32 -- zen_hip_beat_table hands them out.
 *
 *   Parameters: hop a power of two in 64..2048, the frame N = 2 hop; bp_j = floor(60 fs / ((80 + 2j) hop) + 0.5), j = 0..40,
 *   the beat periods of 80..160 bpm in whole hops; create wants bp_0 <= 128 and bp_40 >= 4.
 *
 *   Onset function, per hop t: the frame is the 2 hop samples that end with hop t (zeros before the stream), times the Hann
 *   window 0.5 - 0.5 cos(2 pi i / (N - 1)), rotated by half a frame; X_t its N-point transform (zen_hip_fft_exec_batched).
 *   Per bin, m = sqrt(re re + im im), u = (re / m, im / m) or (1, 0) where m = 0, and with (m1, u1) of frame t-1, u2 of
 *   frame t-2 (X_-1 = X_-2 = 0):  s = (u1r u1r - u1i u1i, u1r u1i + u1r u1i),  d = (sr u2r + si u2i, si u2r - sr u2i),
 *   e = (re - m1 dr, im - m1 di),  v = sqrt(er er + ei ei) where m > m1, else 0.  odf[t] = the sum of v over all N bins:
 *   p[l] = v[l] + v[64 + l] + ... left to right for l < 64, then p[l] += p[l + s] for l < s, s = 32, 16, .., 1.
 *
 *   Tracker, per hop, on v = |odf| + 1e-4f; state df[512], cs[512] (newest last), the period b, countdowns m0 and bc, the
 *   tempo index j and prev[41]; r2(b) = 2b, rh(b) = floor(b / 2 + 0.5):
 *     1. m0 -= 1, bc -= 1; v is appended to df;
 *     2. M = max(0, max_k cs[512 - r2 + k] W1[b][k]), k = 0..r2 - rh; score = (1.0f - 0.9f) v + 0.9f M is appended to cs;
 *     3. m0 == 0: fut = cs ++ b zeros; for i = 512..512 + b - 1 in order fut[i] = max(0, max_k fut[i - r2 + k] W1[b][k]);
 *        n = the first index of the largest fut[512 + n] W2[b][n], 0 if none is positive; bc = n, m0 = n + rh;
 *     4. bc == 0: a beat, and the tempo is estimated again: y = thr(df); acf[l] = (sum_{i < 512 - l} y[i] y[i + l]) /
 *        (float)(512 - l); C[i] = sum over a = 1..4, b' = 1 - a..a - 1 of (acf[a i + b' - 1] R[i]) / (float)(2a - 1) for
 *        i = 2..127, C[1] = C[128] = 0; C = thr(C[1..128]); O[j] = C[bp_j] + C[bp_j / 2]; delta[j] = (max_i prev[i]
 *        T[i][j]) O[j], divided by the sum of the positive delta where that is positive; j = the first index of the
 *        largest delta, prev = delta, b = bp_j.
 *   thr(x)[i] = max(x[i] - (sum of x[max(0, i - 8) .. min(len, i + 8))) / (float)count, 0).  All sums start at +0 and add
 *   left to right in float32.
 * Samples are expected to be finite.
 *
 * Conventions: those of zen_hip.h and zen_hip_pitch.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_beat_last_error() (this library's own thread-local message; failures of the library underneath are copied into
 * it).  All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  Everything is
 * allocated by zen_hip_beat_create, sized by hop, n_streams and max_hops, never by the length of a call.
 */
#ifndef ZEN_HIP_BEAT_H
#define ZEN_HIP_BEAT_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_beat* zen_hip_beat_t;

typedef struct zen_hip_beat_stats_t {
	unsigned long long hops;         /* hops analysed since create (all streams) */
	unsigned long long slices;       /* slices run since create: one track launch each */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the FFT handle's own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_beat_stats_t;

enum { ZEN_HIP_BEAT_KERNELS = 4 }; /* frame, fft, csd, track */
enum { ZEN_HIP_BEAT_TEMPI = 41, ZEN_HIP_BEAT_HISTORY = 512, ZEN_HIP_BEAT_MAX_PERIOD = 128 };

/* the tables of zen_hip_beat_table: `index` is b for the two weightings and the row i for the transition matrix */
enum {
	ZEN_HIP_BEAT_TABLE_WINDOW = 0,     /* N = 2 hop values */
	ZEN_HIP_BEAT_TABLE_PERIOD = 1,     /* bp_j, 41 values (whole numbers) */
	ZEN_HIP_BEAT_TABLE_TEMPO = 2,      /* 60 fs / (hop bp_j), 41 values */
	ZEN_HIP_BEAT_TABLE_PAST = 3,       /* W1[b][k] = exp(-(5 ln((2b - k) / b))^2 / 2), r2(b) - rh(b) + 1 values; b one of the bp_j */
	ZEN_HIP_BEAT_TABLE_FUTURE = 4,     /* W2[b][n] = exp(-(n + 1 - b/2)^2 / (2 (b/2)^2)), b values; b one of the bp_j */
	ZEN_HIP_BEAT_TABLE_RAYLEIGH = 5,   /* R[i] = (i / 43^2) exp(-i^2 / (2 43^2)), i = 0..127: 128 values */
	ZEN_HIP_BEAT_TABLE_TRANSITION = 6  /* T[i][j] = exp(-(i - j)^2 / (2 sigma^2)) / (sigma sqrt(2 pi)), sigma = 41/8: row i, 41 values */
};

const char* zen_hip_beat_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_beat_version(void);

/* fs: sample rate; hop: a power of two in 64..2048 with bp_0 <= 128 and bp_40 >= 4, roughly 9.4 <= fs / hop <= 171
 * (ZEN_HIP_E_BAD_ARG otherwise, before a device is touched); n_streams >= 1 rows analysed by every call.  max_hops only
 * sizes the workspace: calls with more hops run in slices of max_hops, each slice one launch of every kernel, so no launch
 * walks more than max_hops hops.  0 = default: 4096.  A slice takes 20 hop + 20 bytes of device memory per hop and stream
 * (the spectrum row 16 hop, the staging row of the host calls' samples 4 hop, the onset value and the four staged results 20).
 * create allocates all of it, the transform's own included (it runs its largest batch once, on zeros): afterwards no call
 * of the session allocates. */
int zen_hip_beat_create(float fs, size_t hop, size_t n_streams, size_t max_hops, zen_hip_beat_t* h);
int zen_hip_beat_destroy(zen_hip_beat_t h);
int zen_hip_beat_reset(zen_hip_beat_t h);                     /* the state of a fresh session, on the handle's stream */
int zen_hip_beat_set_stream(zen_hip_beat_t h, void* stream); /* waits for what the previous stream holds */

/* Hop t of stream s is the `hop` floats from in_dev + s * in_stride + t * hop on.  Each non-NULL result receives n_streams
 * rows of n_hops floats, out_stride floats apart: the onset function, the score appended to cs, 1 or 0 for a beat in the
 * hop, the tempo in bpm after the hop.  The session keeps the last hop of samples, the last two spectra and the tracker's
 * state: a stream gives the same bits however it is cut into calls.  n_hops == 0 is legal and touches nothing.  Nothing
 * outside the named elements is written.  Pointers need 4-byte alignment only; out_stride >= n_hops where a result is
 * asked for and in_stride >= n_hops * hop (ZEN_HIP_E_BAD_ARG otherwise, nothing is touched).  Asynchronous on the handle's
 * stream; calls may be queued back to back. */
int zen_hip_beat_run_device(zen_hip_beat_t h, const float* in_dev, size_t in_stride, size_t n_hops, float* odf_dev, float* score_dev,
                            float* beat_dev, float* tempo_dev, size_t out_stride);
/* The same rows in host memory: plain copies up and down around the device call, slice by slice.  Synchronous. */
int zen_hip_beat_run_host(zen_hip_beat_t h, const float* in_host, size_t in_stride, size_t n_hops, float* odf_host, float* score_host,
                          float* beat_host, float* tempo_host, size_t out_stride);

int zen_hip_beat_stats(zen_hip_beat_t h, zen_hip_beat_stats_t* out);

/* Profiling hooks for the harness (tools/ab_beat.py), as the pitch library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step ([0] frame, [1] FFT, [2] csd,
 * [3] track) milliseconds, bytes read + written, and launches. */
int zen_hip_beat_profile(zen_hip_beat_t h, int enable);
int zen_hip_beat_profile_get(zen_hip_beat_t h, double ms[ZEN_HIP_BEAT_KERNELS], unsigned long long bytes[ZEN_HIP_BEAT_KERNELS],
                             unsigned long long launches[ZEN_HIP_BEAT_KERNELS]);

/* One host table of (fs, hop), computed without a device: `which` is a ZEN_HIP_BEAT_TABLE_* value, the table's length is
 * the one stated there.  out receives that many floats; cap, the floats out has room for, must be at least that
 * (ZEN_HIP_E_BAD_ARG otherwise, as for an (fs, hop) create refuses, an unknown table and a b that is none of the bp_j). */
int zen_hip_beat_table(float fs, size_t hop, int which, size_t index, float* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_BEAT_H */
