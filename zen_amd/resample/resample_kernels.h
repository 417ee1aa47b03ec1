// resample_kernels.h -- launch interface of the kernels of libzen_hip_resample.so (resample_kernels.hip).
// The device tables have rows of Tp floats, T rounded up to a multiple of 8, the floats behind tap T - 1 zero: a row is read
// in 16-byte pieces and the eight chains of an output advance together.  `table`: the L + 1 rows h[p]; `poly`: the num rows
// c[rem] of the polyphase route.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace zen_resample {

enum { TILE = 256, PHASES = 512, MAX_TAPS = 256 };
// the samples a tile stages: at most 4 (TILE - 1) + 1 first taps, T - 1 more behind the last one, and the row's padding
enum { STAGE = 4 * TILE + MAX_TAPS + 8 };

struct ExpandArgs { // poly[rem][j] = h[p][j] + mu (h[p + 1][j] - h[p][j]), (p, mu) of rem, for rem < num, j < Tp
	const float* table;
	float* poly;
	uint32_t num;
	int Tp;
};

struct FirArgs {
	const float* in;    // row r: in + r * in_stride, the in_count samples from index in_first of the virtual row on
	float* out;         // row r: out + r * out_stride, the outputs out_first .. out_first + out_count
	const float* coef;  // poly: the expanded rows; else the table
	uint64_t in_stride, out_stride, in_first, in_count, n_total, out_first, out_count;
	uint32_t num, den, tiles, n_rows; // tiles = ceil(out_count / TILE) per row
	int W, Tp;
	bool poly;
};

hipError_t launch_expand(const ExpandArgs& a, hipStream_t s);
hipError_t launch_fir(const FirArgs& a, hipStream_t s);

} // namespace zen_resample
