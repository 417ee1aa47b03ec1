// ragged_kernels.h -- launchers of ragged_kernels.hip, for ragged.hip.  All asynchronous on `s`; empty work launches nothing.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace zen_ragged {

// the per-clip table on the device: tab[c] = len_c, tab[n_clips + c] = padded1_c (0 for an empty clip)
typedef unsigned long long tab_t;

// staged[c][j] = j < len_c ? audio[c * stride + j] : 0, j < row (row = the batch's padded pass-1 length = staged's row stride)
hipError_t launch_pack(const float* audio, size_t stride, const tab_t* tab, size_t n_clips, float* staged, size_t row,
                       hipStream_t s);
// in2 (may be NULL) [c][j], j < row2: (P1 + R1)_c spliced as zen_hip_ragged.h states; harm (may be NULL) [c][j], j < max_len:
// j < len_c ? H1_c[j + sh1] : 0.  h1 / p1 / r1: rows `row1` apart.
hipError_t launch_splice(const float* h1, const float* p1, const float* r1, size_t row1, size_t sh1, const tab_t* tab,
                         size_t n_clips, float* in2, size_t row2, float* harm, size_t out_stride, size_t max_len, hipStream_t s);
// perc[c][j] = j < len_c ? P2_c[j + sh2] : 0, j < max_len
hipError_t launch_trim(const float* p2, size_t row2, size_t sh2, const tab_t* tab, size_t n_clips, float* perc, size_t out_stride,
                       size_t max_len, hipStream_t s);

} // namespace zen_ragged
