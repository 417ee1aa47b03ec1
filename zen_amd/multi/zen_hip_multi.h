/*
 * zen_hip_multi.h -- multichannel separation: interleaved frames in, every channel kept (libzen_hip_multi.so, linked against
 * libzen_hip.so).
 *
 * A WAV file, a sound card and a socket hold FRAMES: sample f * C + c is channel c of frame f.  The engines of zen_hip.h
 * take planar rows -- zen_hip_hpr_create(..., n_streams, ...) and zen_hip_hpri_create(..., n_clips, ...) run independent
 * rows in lock step, each bit-identical to that row alone.  This library is the path between the two, on the device: split
 * turns C interleaved channels into C rows, the engine separates row c as stream or clip c, join turns the rows of a stem
 * back into frames.  16-bit audio crosses the host link at 2 bytes per sample.
 *
 * The arithmetic (tests/multi_model.py computes the same bits; the sample formulas are zen_amd/pcm/pcm_convert.h's, the
 * ones the PCM library and zen_amd/cli/wav.h use).  C channels, 1 <= C <= 8 (ZEN_HIP_MULTI_MAX_CHANNELS); the sample format
 * is ZEN_HIP_MULTI_I16 (int16_t) or ZEN_HIP_MULTI_F32 (float).
 *   split  row c, element f = pcm16_to_float(s[f C + c]) = (float)s / 32767.f   (I16)
 *                           = the 32 bits of s[f C + c], NaN payloads included    (F32)
 *   engine output row c is bit for bit what the mono call returns for channel c alone.
 *   join   d[f C + c] = the 32 bits of row c, element f: no gain, no normalisation, the mode is ignored      (F32)
 *                     = float_to_pcm16_gain(y, gain): y * gain rounded, halves away from zero, saturated       (I16, GAIN)
 *                     = float_to_pcm16_peak(y, peak): y / peak, then * 32767.f, rounded alike; peak == 0 gives 0 (I16, PEAK)
 *   peak   ONE per stem, over all its channels together: pcm16_peak_of(min, max) = max(-min, max) of the C rows, NaNs
 *          ignored.  Every channel of a stem is divided by the same number, so the stem keeps the balance between its
 *          channels (its stereo image); for C = 1 this is exactly what `zen offline` writes.  min and max are exact and
 *          commute: the reduction gives the same bits in any order, nothing is summed.
 *
 * Conventions: those of zen_hip.h and the other add-ons -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_multi_last_error() (this library's own thread-local message; failures of the library underneath are copied into
 * it).  All device memory comes from zen_hip_malloc: red zones and poison of the memory checker apply.  int16_t pointers
 * need 2-byte alignment and float pointers 4-byte alignment, nothing more: 16-byte accesses are used wherever the addresses
 * allow, scalar ones for the rest.  Nothing outside the named elements is read or written.
 */
#ifndef ZEN_HIP_MULTI_H
#define ZEN_HIP_MULTI_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ZEN_HIP_MULTI_I16 = 0, ZEN_HIP_MULTI_F32 = 1 };   /* the sample format of interleaved buffers */
enum { ZEN_HIP_MULTI_PEAK = 0, ZEN_HIP_MULTI_GAIN = 1 }; /* how I16 outputs are narrowed (ZEN_PCM_MODE_*) */
enum { ZEN_HIP_MULTI_MAX_CHANNELS = 8 };

typedef struct zen_hip_multi_offline* zen_hip_multi_offline_t;
typedef struct zen_hip_multi_realtime* zen_hip_multi_realtime_t;

typedef struct zen_hip_multi_stats_t {
	unsigned long long calls;        /* device and host calls since create */
	unsigned long long device_bytes; /* device memory this handle asked zen_hip_malloc for so far (the engine's own not included) */
	unsigned long long allocations;  /* zen_hip_malloc calls of this handle so far */
	unsigned long long row_stride;   /* floats between the planar rows of the staging in use */
} zen_hip_multi_stats_t;

const char* zen_hip_multi_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_multi_version(void);

/* ---- the kernels alone, on device pointers, asynchronous on `stream` (a hipStream_t as void*) --------------------------
 * n_frames == 0 is legal and touches nothing.  `channels` outside 1..8, an unknown format or mode, a null pointer with
 * n_frames > 0, a pointer that is not aligned to its element or row_stride < n_frames: ZEN_HIP_E_BAD_ARG, nothing is touched.
 * With split and join in front of and behind a session of n_streams = channels, the live library's pushes
 * (zen_hip_live.h) work on stereo with no further code. */

/* n_frames interleaved frames at src_dev -> `channels` rows of n_frames floats at dst_rows_dev, row_stride floats apart */
int zen_hip_multi_split(int fmt, const void* src_dev, int channels, size_t n_frames, float* dst_rows_dev, size_t row_stride, void* stream);
/* minmax_dev[0] = min(minmax_dev[0], min of the rows), minmax_dev[1] = max(minmax_dev[1], max of the rows): the contract of
 * zen_hip_pcm_peak over `channels` rows -- accumulating, the caller initialises the two words (+INFINITY, -INFINITY), NaNs
 * are ignored, bit-exact against a serial min / max in any order (up to the sign of a zero). */
int zen_hip_multi_peak(const float* rows_dev, int channels, size_t n_frames, size_t row_stride, float* minmax_dev, void* stream);
/* `channels` rows -> n_frames interleaved frames at dst_dev.  I16, ZEN_HIP_MULTI_PEAK: divides by max(-minmax_dev[0],
 * minmax_dev[1]), read on the device when the kernel runs (`gain` ignored); I16, ZEN_HIP_MULTI_GAIN: multiplies by `gain`
 * (`minmax_dev` may be NULL); F32: copies (mode, gain and minmax_dev are ignored). */
int zen_hip_multi_join(int fmt, const float* rows_dev, int channels, size_t n_frames, size_t row_stride, int mode, float gain,
                       const float* minmax_dev, void* dst_dev, void* stream);

/* ---- offline, two-pass -------------------------------------------------------------------------------------------------
 * The handle owns a zen_hip_hpri_t made with n_clips = channels and the arguments of zen_hip_hpri_create, and planar
 * staging rows from zen_hip_malloc: three sets of `channels` rows (input, harmonic, percussive), sized by the largest call
 * so far, never shrunk -- a second call of the same size allocates nothing (zen_hip_multi_stats).  Growing waits for the
 * handle's stream.  There is no residual output: the reference never writes pass 2's residual, it would be zeros. */
int zen_hip_multi_offline_create(float fs, size_t hop_h, size_t hop_p, float beta_h, float beta_p, int nocopybord, int channels,
                                 zen_hip_multi_offline_t* h);
int zen_hip_multi_offline_destroy(zen_hip_multi_offline_t h);
int zen_hip_multi_offline_use_sse_filter(zen_hip_multi_offline_t h);
int zen_hip_multi_offline_use_soft_mask(zen_hip_multi_offline_t h);
int zen_hip_multi_offline_set_stream(zen_hip_multi_offline_t h, void* stream); /* waits for what the previous stream holds */
/* n_frames interleaved frames of format fmt at in_dev -> the harmonic and the percussive stem, interleaved, same format,
 * n_frames frames each; either output may be NULL.  split -> zen_hip_hpri_process_device -> (peak) -> join, all on the
 * handle's stream with no host round trip in between: asynchronous.  mode and gain: as zen_hip_multi_join (I16 only).
 * peaks_dev: NULL, or device memory for two floats that receive, in stream order, the peak the harmonic and the percussive
 * stem were divided by (I16 PEAK; 0 for an output that was not asked for, and in every other mode).  n_frames == 0 touches
 * nothing, peaks_dev included.  The buffers, peaks_dev among them, must not overlap (ZEN_HIP_E_BAD_ARG, nothing is touched). */
int zen_hip_multi_offline_device(zen_hip_multi_offline_t h, int fmt, const void* in_dev, size_t n_frames, void* harm_dev, void* perc_dev,
                                 int mode, float gain, float* peaks_dev);
/* The same on host buffers: plain copies up and down around the device call (2 bytes per sample for I16), on the handle's
 * stream.  Unpipelined: the copies do not overlap the kernels.  Synchronous.  peaks: NULL or two floats in host memory.
 * The buffers must not overlap (ZEN_HIP_E_BAD_ARG, nothing is touched). */
int zen_hip_multi_offline_host(zen_hip_multi_offline_t h, int fmt, const void* in_host, size_t n_frames, void* harm_host, void* perc_host,
                               int mode, float gain, float peaks[2]);
int zen_hip_multi_stats(zen_hip_multi_offline_t h, zen_hip_multi_stats_t* out);

/* ---- realtime block ----------------------------------------------------------------------------------------------------
 * The handle owns a causal zen_hip_hpr_t with n_streams = channels (zen_hip_hpr_create's fs, hop, beta, output_flags) and
 * staging for max_hops hops (0: 256), all allocated by create.  Each call takes n_hops * hop interleaved frames in and
 * writes the same number into each non-NULL output whose flag was given to create (an output without its flag:
 * ZEN_HIP_E_BAD_ARG).  The engine's state is carried from call to call: a block split over several calls, n_hops == 1
 * included, gives the same samples as one call; calls longer than max_hops run in slices of max_hops.  I16 outputs are
 * GAIN only (a stream cannot know its peak); F32 outputs are the engine's raw output and `gain` is ignored. */
int zen_hip_multi_realtime_create(float fs, size_t hop, float beta, unsigned output_flags, int channels, size_t max_hops,
                                  zen_hip_multi_realtime_t* h);
int zen_hip_multi_realtime_destroy(zen_hip_multi_realtime_t h);
int zen_hip_multi_realtime_use_sse_filter(zen_hip_multi_realtime_t h);
int zen_hip_multi_realtime_use_soft_mask(zen_hip_multi_realtime_t h);
int zen_hip_multi_realtime_reset(zen_hip_multi_realtime_t h); /* the state of a fresh stream (zen_hip_hpr_reset_buffers) */
int zen_hip_multi_realtime_set_stream(zen_hip_multi_realtime_t h, void* stream);
/* asynchronous on the handle's stream */
int zen_hip_multi_realtime_device(zen_hip_multi_realtime_t h, int fmt, const void* in_dev, size_t n_hops, void* harm_dev, void* perc_dev,
                                  void* resid_dev, float gain);
/* the same on host buffers, slice by slice: plain copies around the device call.  Synchronous.  The buffers must not overlap. */
int zen_hip_multi_realtime_host(zen_hip_multi_realtime_t h, int fmt, const void* in_host, size_t n_hops, void* harm_host, void* perc_host,
                                void* resid_host, float gain);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_MULTI_H */
