/*
 * zen_hip_pcm.h -- 16- and 24-bit PCM host I/O for the engines of zen_hip.h (libzen_hip_pcm.so, linked against libzen_hip.so).
 *
 * The engines are float-only; this library owns sample formats.  A caller with a WAV file, a sound card or a network
 * stream holds int16_t.  Instead of widening on the CPU, moving 4 bytes per sample each way over the host link and
 * narrowing on the CPU again, the calls below move 2 bytes per sample each way and convert on the device, between the
 * copy and the engine, with the arithmetic of zen_amd/cli/wav.h (pcm_convert.h states it):
 *   in : s / 32767.f (IEEE division); two interleaved channels are mixed as (L + R) / 2.0f
 *   out: lroundf(x * 32767.f), halves away from zero, SATURATED to [-32768, 32767] (wav.h's cast wraps instead), NaN -> 0.
 * The engines' outputs are not at unit gain (the inverse transform is unnormalised and the COLA factor multiplies on top),
 * so x is one of
 *   ZEN_HIP_PCM_PEAK: x = y / peak, peak = max(-min(y), max(y)) over the WHOLE output of the call -- what the command line
 *                     tool's peak_normalise followed by its encoder write, sample for sample; peak == 0 (silence) gives
 *                     zeros where the tool divides 0 by 0.  NaNs in an output are ignored by the peak.
 *   ZEN_HIP_PCM_GAIN: the rounded value is y * gain for the caller's gain (a stream cannot know its peak: saturation is
 *                     what protects it).
 *
 * Packed 24-bit samples (ZEN_HIP_PCM_I24: three little-endian bytes each, what a 24-bit WAV file holds) move 3 bytes per
 * sample each way through the calls that take a format, with wav.h:80-86's arithmetic on the scale 2^23:
 *   in : v / 8388608.f, exact for every code; the stereo mix as above
 *   out: x * 8388608.f rounded as above, SATURATED to [-8388608, 8388607], NaN -> 0.  The multiplier is the reader's
 *        divisor, so every code k survives k / 2^23 and back; PEAK and GAIN supply x as for 16 bits (GAIN rounds y * gain).
 * Input and output format are independent: 24 in and 16 out is the CD master, 16 in and 24 out keeps what the separation
 * computed in float32.
 * Alignment.  A packed 24-bit buffer is only byte-aligned, and a piece of a pipeline starts at any sample.  3 is coprime to
 * 16, so one of the next 16 samples from any address starts on a 16-byte boundary: the kernels convert a head of at most 15
 * samples and a tail byte by byte, and between them groups of 16 samples as 48 bytes in three 16-byte accesses per lane
 * (four on the float side where that is aligned too).  Head and tail of the packing kernel are byte stores: nothing beside
 * the 3 n bytes named is read or written, so neighbouring pieces may be in flight.  Stereo input at an odd address, where
 * every 6-byte frame straddles every boundary, is converted byte by byte; the host calls never produce one.
 * Measured (profiles/pcm24_host_ab.json, tools/ab_pcm_host.py --fmt i24; one hour of mono audio, three outputs, pinned
 * buffers, medians): GAIN 21.4 ms against 15.6 ms for the int16 call (1.37x for 1.5x the bytes) and 35.4 ms for the float
 * call alone; PEAK 34.0 ms against 28.7 ms and the same 35.4 ms -- a PEAK call brings nothing down under the engine's
 * kernels, so only its tail (17.5 ms: 2 x 476 MB at 54 GB/s) grows with the bytes.  Today's route for a 24-bit file (unpack
 * and widen on the host, float call, peak / scale / round / pack on one host thread) takes 1127 ms.  Each kernel on a piece
 * of 8 Mi samples: 0.020 ms (unpack) and 0.016 ms (pack) beside 0.46 ms for the link's copy of the piece's 25 MB.
 *
 * Conventions: those of zen_hip.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from zen_hip_pcm_last_error() (this
 * library's own thread-local message; failures of the engine underneath are copied into it).
 *
 * Streams.  The C ABI of the engines has no getter for the stream an engine launches on, and the pipelines below must
 * order their conversion launches against the engine's.  The two *_process* calls therefore put the engine on a stream
 * that belongs to this library's context for that handle (zen_hip_hpr_set_stream / zen_hip_hpri_set_stream, which wait for
 * what the engine's previous stream holds) and LEAVE IT THERE: after the first PCM call the engine's float calls run on
 * that stream too.  A caller that moves the engine to another stream may do so; the next PCM call moves it back.
 *
 * Contexts.  Staging memory (from zen_hip_malloc: red zones and poison of the memory checker apply), three streams and
 * the events live in a context cached per engine handle; it grows and is never shrunk, so steady-state calls allocate
 * nothing.  The CALLER releases it with zen_hip_pcm_release(handle) BEFORE destroying the engine handle (the engine must
 * not be left on a destroyed stream while it is still used; release waits for the context's streams and puts the engine
 * back on the null stream).  zen_hip_pcm_release_all() drops the buffers of every context without touching any engine:
 * for process exit, after the engines are gone.
 */
#ifndef ZEN_HIP_PCM_H
#define ZEN_HIP_PCM_H

#include <stddef.h>
#include <stdint.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ZEN_HIP_PCM_PEAK = 0, ZEN_HIP_PCM_GAIN = 1 };
enum { ZEN_HIP_PCM_I16 = 0, ZEN_HIP_PCM_I24 = 1 }; /* 2 and 3 bytes per sample, little-endian, packed */

const char* zen_hip_pcm_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_pcm_version(void);

size_t zen_hip_pcm_sample_bytes(int fmt); /* 0 for an unknown format; host only */

/* ---- the kernels alone, on device pointers, asynchronous on `stream` (a hipStream_t as void*) --------------------
 * for callers who keep their own buffers on the device.  int16_t pointers need 2-byte alignment, float pointers 4-byte
 * alignment, nothing more: 16-byte accesses are used where the addresses allow, scalar ones for the rest. */

/* n_frames frames of `channels` (1 or 2) interleaved samples -> n_frames floats */
int zen_hip_pcm_to_float(const int16_t* src_dev, int channels, size_t n_frames, float* dst_dev, void* stream);
/* minmax_dev[0] = min(minmax_dev[0], min(src)), minmax_dev[1] = max(minmax_dev[1], max(src)): accumulating, so that the
 * pieces of one output can be folded in one after the other; the caller initialises the two words (+INFINITY, -INFINITY).
 * NaNs are ignored.  The result does not depend on the order of the reduction: bit-exact against a serial min / max
 * (up to the sign of a zero). */
int zen_hip_pcm_peak(const float* src_dev, size_t n, float* minmax_dev, void* stream);
/* n floats -> n int16_t.  ZEN_HIP_PCM_PEAK: divides by max(-minmax_dev[0], minmax_dev[1]), read on the device when the
 * kernel runs (`gain` ignored); ZEN_HIP_PCM_GAIN: multiplies by `gain` (`minmax_dev` ignored, may be NULL). */
int zen_hip_pcm_from_float(const float* src_dev, size_t n, int mode, float gain, const float* minmax_dev,
                           int16_t* dst_dev, void* stream);

/* The same two by format: zen_hip_pcm_to_float and zen_hip_pcm_from_float are these with ZEN_HIP_PCM_I16.  I24 pointers need
 * no alignment, I16 pointers 2 bytes; an unknown format is ZEN_HIP_E_BAD_ARG. */
int zen_hip_pcm_unpack(int fmt, const void* src_dev, int channels, size_t n_frames, float* dst_dev, void* stream);
int zen_hip_pcm_pack(int fmt, const float* src_dev, size_t n, int mode, float gain, const float* minmax_dev, void* dst_dev,
                     void* stream);

/* ---- realtime block engine, host to host ----------------------------------------------------------------------------
 * The contract of zen_hip_hpr_process_host with 16-bit samples: n_hops * hop frames of `channels` interleaved int16_t in,
 * n_hops * hop int16_t into each non-NULL output; one stream per engine (n_streams == 1); synchronous; the engine's state
 * is carried from call to call exactly as the float calls carry it (a block may be split over several calls, and float
 * and PCM calls may be mixed).  Buffers the runtime knows as pinned (zen_hip_host_alloc_mapped) are copied asynchronously,
 * pageable ones are registered for the duration of the call.  No two of the four buffers may overlap
 * (ZEN_HIP_E_BAD_ARG, nothing is touched).
 * Pieces of `piece_hops` hops (0: the default, 4 Mi samples per piece in GAIN and 8 Mi in PEAK mode) go up as int16_t,
 * are widened, run through zen_hip_hpr_process and
 *   GAIN: are narrowed and come down while the next piece runs;
 *   PEAK: stay on the device as floats while min and max accumulate behind each piece; when the last piece is through,
 *         the outputs are narrowed and come down in pieces.  The block is the unit that is normalised, as `zen fakert`
 *         normalises a whole file.
 * peaks (may be NULL) receives what the harmonic, percussive and residual output were divided by (PEAK; 0 for an output
 * that was not asked for) -- in GAIN mode it is not written. */
int zen_hip_pcm_hpr_process_host(zen_hip_hpr_t h, const int16_t* in_host, int channels, size_t n_hops, int16_t* harm,
                                 int16_t* perc, int16_t* resid, int mode, float gain, float peaks[3], size_t piece_hops);

/* The same call with a format for the input and one for all outputs (zen_hip_pcm_hpr_process_host is this one with
 * ZEN_HIP_PCM_I16 twice): the contract above with zen_hip_pcm_sample_bytes(fmt) in place of 2 -- copies, registration and
 * the overlap check count bytes of the buffer's own format.  An unknown format is refused before anything is touched. */
int zen_hip_pcm_hpr_process_host_fmt(zen_hip_hpr_t h, int in_fmt, const void* in_host, int channels, size_t n_hops, int out_fmt,
                                     void* harm, void* perc, void* resid, int mode, float gain, float peaks[3], size_t piece_hops);

/* ---- offline two-pass engine, host to host --------------------------------------------------------------------------
 * The contract of zen_hip_hpri_process with 16-bit samples (handle created with n_clips == 1): n_frames frames in, n_frames
 * int16_t into each non-NULL output; synchronous; the buffers must not overlap.  In PEAK mode harm / perc hold what
 * `zen offline` writes into its WAV files, sample for sample (an all-silent output excepted, see above).
 * Clips longer than one range run as a pipeline over time ranges of `range_samples` frames (0: the default -- 8 Mi for
 * clips of 32 Mi frames and more, 4 Mi for shorter ones, one range below 8 Mi; rounded up to a multiple of 16384):
 * range k+1 goes up and is widened, range k-1 is narrowed and comes down under the kernels of range k
 * (zen_hip_hpri_range_halo / zen_hip_hpri_process_range; a clip of one range is the range [0, n_frames) of the same call,
 * bit-identical to zen_hip_hpri_process_device -- which, unlike it, cannot tell a handle of several clips).  In PEAK mode
 * the peak is the whole clip's: narrowing starts when the last range is through.
 * resid is filled with zeros on the host in either mode (the reference never writes pass 2's residual); peaks[2] = 0. */
int zen_hip_pcm_hpri_process(zen_hip_hpri_t h, const int16_t* audio_host, int channels, size_t n_frames, int16_t* harm,
                             int16_t* perc, int16_t* resid, int mode, float gain, float peaks[3], size_t range_samples);

/* with formats, as above; resid is n_frames * zen_hip_pcm_sample_bytes(out_fmt) zero bytes */
int zen_hip_pcm_hpri_process_fmt(zen_hip_hpri_t h, int in_fmt, const void* audio_host, int channels, size_t n_frames, int out_fmt,
                                 void* harm, void* perc, void* resid, int mode, float gain, float peaks[3], size_t range_samples);

/* what the last host-to-host call of this thread did, for the harness (tools/ab_pcm_host.py) */
typedef struct {
	size_t n_pieces, piece_frames;
	int input_pinned, outputs_pinned; /* known to the runtime or registered for the call: asynchronous copies */
	double setup_ms;                  /* staging buffers + registration */
	double tail_ms;                   /* PEAK: from the end of the last piece's kernels to the end of the call */
	double total_ms;
} zen_hip_pcm_host_stats;
int zen_hip_pcm_host_stats_get(zen_hip_pcm_host_stats* out);

/* release the context of an engine handle (zen_hip_hpr_t or zen_hip_hpri_t); see "Contexts" above.  Unknown handle: OK. */
int zen_hip_pcm_release(void* engine_handle);
int zen_hip_pcm_release_all(void);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_PCM_H */
