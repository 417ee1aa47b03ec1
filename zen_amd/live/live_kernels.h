// live_kernels.h -- launchers of live_kernels.hip, for live.hip.  All asynchronous on `s`; empty work launches nothing.
// Every row pointer is the row of stream 0; stream c's row is `stride` floats further per stream.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace zen_live {

// a source row read through the reference's shift: position j of a stream gives
//     j < shifted_end ? row[j + off_shifted] : j < stale_end ? row[j + off_stale] : 0
// (a running stream: shifted_end = stale_end = SIZE_MAX).  The offsets place the stream's positions in the row.
struct Shifted {
	const float* row;
	size_t stride;
	size_t shifted_end, stale_end;
	long long off_shifted, off_stale;
};

// The stream X = the carried partial block (c samples of carry_cur), then the m new samples of `in`, then zeros.
struct FeedArgs {
	const float* in; // may be NULL when m == 0
	size_t in_stride, m;
	const float* carry_cur;
	float* carry_next;
	size_t carry_stride, c, c_next; // carry_next[k] = X[len1 + k], k < c_next
	float* in1;                     // in1[i] = X[i], i < len1: pass 1's input rows
	size_t in1_stride, len1;
	float* dry; // ring[(dry_pos + i) % dry_len] = in[i], i < m (m < dry_len)
	size_t dry_stride, dry_len, dry_pos;
	size_t n_streams;
};
hipError_t launch_feed(const FeedArgs& a, hipStream_t s);

// in2[j] = q(t0 + j), j < len2, where q reads P1 + R1 (two rows of the same geometry: p and the row r1) through `Shifted`;
// hist_next[i] = hist_cur[hist_from + i], i < hist_len (the H1 delay: the last samples of [history | this call's H1]).
struct MidArgs {
	Shifted p;
	const float* r1;
	float* in2;
	size_t in2_stride, len2, t0;
	const float* hist_cur;
	float* hist_next;
	size_t hist_stride, hist_from, hist_len;
	size_t n_streams;
};
hipError_t launch_mid(const MidArgs& a, hipStream_t s);

// cnt samples from stream position d0 on into the caller's rows (each may be NULL): perc and harm through `Shifted`, dry
// from its ring
struct OutArgs {
	Shifted p2, h1;
	const float* dry;
	size_t dry_stride, dry_len, dry_pos; // dry_pos = d0 % dry_len
	float *harm_out, *perc_out, *dry_out;
	size_t out_stride, cnt, d0;
	size_t n_streams;
};
hipError_t launch_out(const OutArgs& a, hipStream_t s);

} // namespace zen_live
