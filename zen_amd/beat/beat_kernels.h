// beat_kernels.h -- launch interface of the three kernels of libzen_hip_beat.so (beat_kernels.hip).
// A slice is `hops` hops of each of `n_streams` streams.  Its spectrum rows are packed hop by hop: group g holds the
// n_streams rows (N complex values each) of one frame; groups 0 and 1 are the frames t-2 and t-1 the session kept, group
// 2 + c is hop c of the slice, so one batched transform covers the slice.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace zen_beat {

enum { STATE_WORDS = 1088 }; // per stream: df[512] | cs[512] | prev[41] | b, m0, bc, j, head | padding

struct FrameArgs {
	const float* in;   // hop c of stream s of this slice: in + s * in_stride + c * hop
	const float* tail; // n_streams rows of hop floats: the hop in front of the slice
	const float* win;  // N floats
	float* rows;       // the spectrum groups
	size_t in_stride, hops, n_streams;
	int hop;
};

struct CsdArgs {
	const float* rows;
	float* odf; // n_streams rows of odf_stride floats: element (s, c)
	size_t odf_stride, hops, n_streams;
	int hop;
};

struct TrackArgs {
	const float* odf_ws; // as CsdArgs::odf
	size_t odf_stride;
	const float* tables; // beat_tables.h's device copy
	float* state;        // STATE_WORDS words per stream
	float *odf, *score, *beat, *tempo; // any may be NULL; element (s, c0 + c) of rows out_stride apart
	size_t out_stride, c0, hops, n_streams;
};

hipError_t launch_frame(const FrameArgs& a, hipStream_t s);
hipError_t launch_csd(const CsdArgs& a, hipStream_t s);
hipError_t launch_track(const TrackArgs& a, hipStream_t s);

} // namespace zen_beat
