// blockrun_kernel.h -- launch interface of the run kernel (blockrun_kernel.hip): the headline block call (causal, nfft
// 4096, hop 1024, 47 taps, percussive output, hard mask) with one workgroup per run of consecutive hops of a stream.
#pragma once
#include <hip/hip_runtime.h>

#include "blockrun_partition.h"

namespace zen_blockrun {

constexpr int HOP = 1024, NFFT = 4096, TAPS = 47;

// what RtFusedArgs (csrc/rt_fused.h) holds for such a call, without the fields of the other builds
struct RunArgs {
	const float* in; // stream s: in[s*in_stride .. +n_frames*HOP)
	long long in_stride;
	const float* tail_prev; // [n_streams][HOP]: the hop before the call's first
	float* tail_next;       // receives the call's last hop
	const float* window;    // HOP * 2 values
	const float2* tw;
	int tw_symmetric;       // the host table passed blockrun_first_pass.h's table_is_symmetric (the engine's does)
	float2 tw16, tw8, tw3_16; // tw[N/16], tw[N/8], tw[3N/16] of the host table: all the first analysis pass multiplies with
	float* mag;             // magnitude ring: the call's last keep_mag_rows frames store their rows
	int keep_mag_rows;
	long long ring_rows, row0;
	int n_frames, n_streams, prev_frames;
	float* carry; // [n_streams][HOP]: second half of the previous call's last frame (saved by this launch)
	float* Y;     // synthesis rows, 2 * HOP floats per frame
	long long y_stream_stride;
	float* out;   // the finished hops
	long long out_stride;
	unsigned* need; // per item (stream * n_frames + frame): 1 = left for the fix-up launch
	float cola;
	double thr;     // masks.h hard_mask_threshold
	zen_blockrun_part part;
};

constexpr size_t LDS_BYTES_MAX = 53 * 1024;
size_t run_kernel_lds_bytes();
int launch_run(const RunArgs& a, hipStream_t stream);   // n_streams * part.runs_per_stream workgroups
int launch_fixup(const RunArgs& a, hipStream_t stream); // one wavefront per item, the marked ones are added up

} // namespace zen_blockrun
