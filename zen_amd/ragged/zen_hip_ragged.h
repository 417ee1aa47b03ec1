/*
 * zen_hip_ragged.h -- ragged offline batches for the two-pass engine of zen_hip.h (libzen_hip_ragged.so, linked against
 * libzen_hip.so): clips of UNEQUAL length separated in one call.
 *
 * zen_hip_hpri_process_device takes one length for every row of its batch.  A library of clips of all-different lengths
 * therefore runs one launch set per clip.  The calls below take a length per row: the rows are zero-padded to the longest
 * clip's hop count, both passes run once over the whole batch through the public block call zen_hip_hpr_process, and two
 * streaming kernels of this library put the per-clip parts of HPRIOffline::process (hps.cu:128-221) around them.
 *
 * Why the samples are the same.  Both passes are streaming recurrences: the output of hop i depends on hops <= i, and a
 * block call returns what the same hops return one at a time.  A clip followed by zeros therefore gives the clip's own
 * samples.  What depends on the clip's own length is the reference's in-place shift between the passes: the
 * sum Q = P1 + R1 is shifted left by sh1 = lag_h * hop_h inside a vector of padded1 samples, whose last sh1 samples keep
 * their contents, and pass 2 reads them.  With padded1_c = (ceilf((float)n_c / (float)hop_h) + lag_h) * hop_h of clip c
 * (hps.cu:109-126, float arithmetic), pass 2's input row of clip c is
 *     in2_c[j] = Q_c[j + sh1]   j <  padded1_c - sh1
 *              = Q_c[j]         padded1_c - sh1 <= j < padded1_c
 *              = 0              j >= padded1_c
 *     harm_c[j] = H1_c[j + sh1], perc_c[j] = P2_c[j + sh2]   j < n_c,   sh2 = lag_p * hop_p
 * Row c of the results is bit-identical to zen_hip_hpri_process_device on an n_clips == 1 handle given that clip alone.
 *
 * Conventions: those of zen_hip.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from zen_hip_ragged_last_error() (this
 * library's own thread-local message; failures of the engine underneath are copied into it).  All device memory comes from
 * zen_hip_malloc: red zones and poison of the memory checker apply.  Scratch is cached on the handle, grows and never
 * shrinks: steady-state calls allocate nothing.  Beside the caller's buffers a call holds 4 floats per padded pass-1
 * sample and 2 per padded pass-2 sample of the batch.
 */
#ifndef ZEN_HIP_RAGGED_H
#define ZEN_HIP_RAGGED_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_ragged* zen_hip_ragged_t;

const char* zen_hip_ragged_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_ragged_version(void);

/* The arguments of zen_hip_hpri_create, and its pair of engines: pass 1 at hop_h with H, P and R, pass 2 at hop_p with P,
 * both ZEN_HIP_TIME_ANTICAUSAL with n_streams == n_clips.  hop_h % hop_p != 0 => ZEN_HIP_E_HOPS_NOT_DIVISIBLE. */
int zen_hip_ragged_create(float fs, size_t hop_h, size_t hop_p, float beta_h, float beta_p, int nocopybord, size_t n_clips,
                          zen_hip_ragged_t* h);
int zen_hip_ragged_destroy(zen_hip_ragged_t h);
int zen_hip_ragged_set_stream(zen_hip_ragged_t h, void* stream); /* waits for what the previous stream holds */
int zen_hip_ragged_use_sse_filter(zen_hip_ragged_t h);
int zen_hip_ragged_use_soft_mask(zen_hip_ragged_t h);

/* Device-resident batch.  Row c of audio_dev (rows `stride` floats apart) holds lens[c] samples; nothing beyond them is
 * read and the input is never written.  `lens` is a host array of n_clips entries, read before the call returns.  Each
 * non-NULL output receives n_clips rows `out_stride` floats apart: row c = the clip's lens[c] samples followed by zeros up
 * to max(lens); nothing at or beyond max(lens) in a row is touched.  lens[c] == 0 gives a row of zeros; all lengths zero:
 * OK, nothing is written.  Pointers need 4-byte alignment only; the outputs must not overlap the input or each other.
 * ZEN_HIP_E_BAD_ARG (nothing is touched): a null handle, input or lens; stride or out_stride < max(lens).
 * Asynchronous on the handle's stream; calls may be queued back to back. */
int zen_hip_ragged_process_device(zen_hip_ragged_t h, const float* audio_dev, const size_t* lens, size_t stride,
                                  float* harm_dev, float* perc_dev, size_t out_stride);

/* The same for a caller that holds SEPARATE HOST buffers: clips[c] = lens[c] samples; harm / perc = NULL or n_clips
 * pointers (a NULL entry skips that clip), each receiving lens[c] samples.  No padded matrix is built on the host: every
 * clip goes straight into its row of the staging buffer and every result comes down from its row.  Synchronous. */
int zen_hip_ragged_process_host(zen_hip_ragged_t h, const float* const* clips, const size_t* lens, float* const* harm,
                                float* const* perc);

/* hops the two passes run for a batch whose longest clip has max_len samples, and the row lengths they run on */
int zen_hip_ragged_hop_counts(zen_hip_ragged_t h, size_t max_len, size_t* n_hops_h, size_t* n_hops_p);

/* Profiling hooks for the harness (tools/ab_ragged.py).  enable != 0: HIP events around every launch of this library's
 * kernels and of the two engines from now on.  _get synchronises and returns, summed since the last _get, per kernel
 * ([0] pack, [1] splice, [2] trim) milliseconds, bytes read + written, and launches.  _get_engine: the per-class times of
 * zen_hip_hpr_profile_get_all for pass 1 or 2. */
int zen_hip_ragged_profile(zen_hip_ragged_t h, int enable);
int zen_hip_ragged_profile_get(zen_hip_ragged_t h, double ms[3], unsigned long long bytes[3], unsigned long long launches[3]);
int zen_hip_ragged_profile_get_engine(zen_hip_ragged_t h, int pass, double ms[6], unsigned long long launches[6]);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_RAGGED_H */
