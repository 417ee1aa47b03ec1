/*
 * zen_hip_blockrun.h -- the headline block call with runs of consecutive hops per workgroup
 * (libzen_hip_blockrun.so, linked against libzen_hip.so).
 *
 * zen_hip_blockrun_process has the contract of zen_hip_hpr_process (zen_hip.h) and works on the same engine handle.
 * Calls of the headline configuration -- a causal engine at nfft 4096 with the 47-tap frequency median, the percussive
 * output alone, hard mask -- that are large enough run through the library's own kernel: one workgroup walks a run of
 * consecutive hops of one stream, the overlap-add stays on the chip between the frames of a run, and the engine is left
 * in the state zen_hip_hpr_process would have left it in.  Every other call is forwarded to zen_hip_hpr_process
 * unchanged.  The outputs are the same bit for bit either way.
 *
 * Unlike the other add-on libraries this one shares the layout of the engine's state with libzen_hip.so at compile time
 * (zen_amd/csrc/hpr_engine.h): the two are built from one tree and used as a pair.
 *
 * Conventions: those of zen_hip.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from zen_hip_last_error().
 */
#ifndef ZEN_HIP_BLOCKRUN_H
#define ZEN_HIP_BLOCKRUN_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* As zen_hip_hpr_process: n_hops hops of every stream from in_dev (rows in_stride floats apart); the finished hops of
 * the wanted outputs to harm / perc / resid (null: not wanted; rows out_stride floats apart). */
int zen_hip_blockrun_process(zen_hip_hpr_t h, const float* in_dev, size_t n_hops, size_t in_stride, float* harm, float* perc,
                             float* resid, size_t out_stride);

/* Process-wide settings, for tests and A/B runs.  Keys:
 *   "run_len"    hops per run at most; 0 (default): chosen per call (blockrun_partition.h)
 *   "min_items"  calls of fewer than this many hops over all streams are forwarded; default 4096
 *   "off"        != 0: every call is forwarded
 * An unknown key or a negative value is ZEN_HIP_E_BAD_ARG. */
int zen_hip_blockrun_set(const char* key, int value);

/* Calls of zen_hip_blockrun_process since the library was loaded: served by the run kernel / forwarded (either may be
 * null).  What a test looks at to know which path it has compared. */
int zen_hip_blockrun_stats(unsigned long long* routed, unsigned long long* forwarded);

#ifdef __cplusplus
}
#endif

#endif
