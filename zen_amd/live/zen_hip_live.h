/*
 * zen_hip_live.h -- the two-pass separation of zen_hip.h (HPR-I, HPRIOffline) as a bounded-latency STREAM
 * (libzen_hip_live.so, linked against libzen_hip.so).
 *
 * zen_hip_hpri_process* take a whole clip whose length is known in advance.  Nothing in the two passes needs that: both
 * are streaming recurrences (the output of hop i depends on hops <= i, a block call returns what the same hops return one
 * at a time, state is carried from call to call) and the anticausal engine delays its output by `lag` hops.  A session of
 * this library takes samples as they arrive and hands out, a fixed latency later, the samples HPRIOffline::process
 * (hps.cu:128-221) gives for the whole clip -- bit for bit, whatever the sizes of the pushes.
 *
 * The streams.  Pass 1 (hop_h; H1, P1, R1) runs one block of hop_h samples at a time, pass 2 (hop_p; P2) reads the sum
 * Q = P1 + R1 (one IEEE add, no contraction).  With sh1 = lag_h * hop_h and sh2 = lag_p * hop_p
 *     in2[j]  = Q[j + sh1]                        pass 2's input stream
 *     harm[j] = H1[j + sh1]      perc[j] = P2[j + sh2]      dry[j] = in[j]
 * After N samples pushed in total, pass 1 has run B = N / hop_h whole blocks, pass 2 everything in in2[0, B*hop_h - sh1),
 * and the session has delivered exactly max(0, B*hop_h - sh1 - sh2) samples of each output: host arithmetic only.  The
 * latency is sh1 + sh2 samples (zen_hip_live_latency) plus the push granularity hop_h.
 *
 * The end.  zen_hip_live_finish_* completes the stream of n = the samples pushed as the reference completes a clip of n
 * samples: padded1 = (ceilf((float)n / (float)hop_h) + lag_h) * hop_h and padded2 likewise from hop_p, lag_p (hps.cu:109-126,
 * float arithmetic); the carried partial block and zeros go through pass 1 up to padded1; pass 2's input continues with
 *     in2[j] = Q[j + sh1]  j < padded1 - sh1;   Q[j]  j < padded1 (what the reference's in-place shift leaves behind,
 *     SURVEY Q9);   0 beyond,   up to padded2,
 * and the remaining n - delivered (< sh1 + sh2 + hop_h) samples are written with the reference's end mapping
 *     harm[j] = H1[j+sh1]  j < padded1-sh1,  else H1[j]  j < padded1,  else 0
 *     perc[j] = P2[j+sh2]  j < padded2-sh2,  else P2[j]  j < padded2,  else 0
 * The later branches fire only where (float)n loses a block, which needs n > 2^24.
 *
 * The bound.  finish relies on "blocks already processed <= blocks the padder asks for": floor(n / hop) <=
 * ceilf((float)n / (float)hop) for both hops.  Then finish always runs at least lag_h blocks of pass 1, so every sample of Q
 * and H1 that the end mapping names lies in the rows finish has just computed, and likewise for P2.  It holds for every
 * n <= 2^24 (all integers exact), and for n < 2^24 * hop_p where hop_p is a power of two: a block boundary k * hop_p,
 * k < 2^24, is then an exact float (so is every boundary of hop_h, a multiple of hop_p); (float)n is not below it because
 * rounding is monotone; the float quotient of two such numbers is not below the exact k (or floor(n / hop_h)), again by
 * monotone rounding, and those are exact floats.  zen_hip_live_max_samples gives that bound; a push that would take the
 * stream beyond it is refused with ZEN_HIP_E_UNSUPPORTED and touches nothing.
 *
 * Conventions: those of zen_hip.h and zen_hip_ragged.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_live_last_error() (this library's own thread-local message; failures of the engine underneath are copied into
 * it).  All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  Everything is
 * allocated by zen_hip_live_create, sized by max_push and the geometry, never by the length of the stream.
 */
#ifndef ZEN_HIP_LIVE_H
#define ZEN_HIP_LIVE_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_live* zen_hip_live_t;

typedef struct zen_hip_live_stats_t {
	unsigned long long pushed;       /* samples per stream since the last reset */
	unsigned long long delivered;    /* samples of each output written since the last reset */
	unsigned long long device_bytes; /* device memory this session asked zen_hip_malloc for (the engines' own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this session so far */
} zen_hip_live_stats_t;

const char* zen_hip_live_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_live_version(void);
/* the largest stream length a session of these hops accepts (see "The bound"); host arithmetic, no device needed */
int zen_hip_live_max_samples(size_t hop_h, size_t hop_p, unsigned long long* out);

/* The arguments of zen_hip_hpri_create, and its pair of engines: pass 1 at hop_h with H, P and R, pass 2 at hop_p with P,
 * both ZEN_HIP_TIME_ANTICAUSAL with n_streams rows in lock step.  hop_h % hop_p != 0 => ZEN_HIP_E_HOPS_NOT_DIVISIBLE.
 * max_push (0: hop_h) only sizes the buffers: larger pushes are processed in slices of max_push.  create allocates
 * everything, the engines' growth included (both run their largest block on zeros once, then are reset): afterwards no
 * call of the session allocates. */
int zen_hip_live_create(float fs, size_t hop_h, size_t hop_p, float beta_h, float beta_p, int nocopybord, size_t n_streams,
                        size_t max_push, zen_hip_live_t* h);
int zen_hip_live_destroy(zen_hip_live_t h);
int zen_hip_live_set_stream(zen_hip_live_t h, void* stream); /* waits for what the previous stream holds */
/* accepted only before the first push after create / reset / finish, else ZEN_HIP_E_BAD_ARG */
int zen_hip_live_use_sse_filter(zen_hip_live_t h);
int zen_hip_live_use_soft_mask(zen_hip_live_t h);
int zen_hip_live_reset(zen_hip_live_t h); /* forget the stream: the next push starts a new one */

int zen_hip_live_latency(zen_hip_live_t h, size_t* samples);       /* sh1 + sh2 */
int zen_hip_live_produces(zen_hip_live_t h, size_t m, size_t* out); /* what a push of m would write now; host only */
int zen_hip_live_pending(zen_hip_live_t h, size_t* out);           /* what finish would write now */

/* m new samples of every stream: row s of in_dev (rows in_stride floats apart).  m may be anything, 0 included (in_dev may
 * then be NULL).  Each non-NULL output receives n_streams rows out_stride floats apart with the next *produced samples of
 * the stream; nothing at or beyond *produced in a row is touched.  dry is the input delayed like the other two, an exact
 * copy.  Pointers need 4-byte alignment only; the outputs must not overlap the input or each other; in_stride >= m and
 * out_stride >= *produced (ZEN_HIP_E_BAD_ARG otherwise, nothing is touched).  produced may be NULL.  Asynchronous on the
 * handle's stream; calls may be queued back to back. */
int zen_hip_live_push_device(zen_hip_live_t h, const float* in_dev, size_t m, size_t in_stride, float* harm_dev, float* perc_dev,
                             float* dry_dev, size_t out_stride, size_t* produced);
/* The end of the stream: writes the remaining zen_hip_live_pending samples and leaves the session reset. */
int zen_hip_live_finish_device(zen_hip_live_t h, float* harm_dev, float* perc_dev, float* dry_dev, size_t out_stride,
                               size_t* produced);
/* The same rows in host memory: plain copies up and down around the device call (no piece pipeline).  Synchronous. */
int zen_hip_live_push_host(zen_hip_live_t h, const float* in_host, size_t m, size_t in_stride, float* harm_host, float* perc_host,
                           float* dry_host, size_t out_stride, size_t* produced);
int zen_hip_live_finish_host(zen_hip_live_t h, float* harm_host, float* perc_host, float* dry_host, size_t out_stride,
                             size_t* produced);

int zen_hip_live_stats(zen_hip_live_t h, zen_hip_live_stats_t* out);

/* Profiling hooks for the harness (tools/ab_live.py), as the ragged library's.  enable != 0: HIP events around every
 * launch of this library's kernels and of the two engines from now on.  _get synchronises and returns, summed since the
 * last _get, per kernel ([0] feed, [1] mid, [2] out) milliseconds, bytes read + written, and launches.  _get_engine: the
 * per-class times of zen_hip_hpr_profile_get_all for pass 1 or 2. */
int zen_hip_live_profile(zen_hip_live_t h, int enable);
int zen_hip_live_profile_get(zen_hip_live_t h, double ms[3], unsigned long long bytes[3], unsigned long long launches[3]);
int zen_hip_live_profile_get_engine(zen_hip_live_t h, int pass, double ms[6], unsigned long long launches[6]);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_LIVE_H */
