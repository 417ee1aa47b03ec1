/* blockrun_partition.h -- how a block call's hops are dealt to the workgroups of the run kernel (blockrun_kernel.hip):
 * every stream's n_hops consecutive hops are cut into the same number of runs, the first n_long of them one hop longer
 * than the rest.  Plain C, no HIP: the launcher, the kernel and the host test (tests/test_blockrun_abi.py) share it. */
#ifndef ZEN_HIP_BLOCKRUN_PARTITION_H
#define ZEN_HIP_BLOCKRUN_PARTITION_H

#if defined(__HIPCC__)
#define ZEN_BLOCKRUN_FN static __host__ __device__ inline
#else
#define ZEN_BLOCKRUN_FN static inline
#endif

typedef struct zen_blockrun_part {
	int runs_per_stream; /* 1 .. n_hops */
	int base_len;        /* n_hops / runs_per_stream (>= 1) */
	int n_long;          /* n_hops % runs_per_stream: the stream's first n_long runs have base_len + 1 hops */
} zen_blockrun_part;

/* Hops per run the launcher aims at when none is asked for: long enough that a run's start (arguments, index arithmetic,
 * the first frame's loads) and its one fix-up hop are an eighth of it, short enough that a full-size call of 25 840 hops
 * is four runs per slot of a 256-CU device with at most one hop of imbalance between workgroups. */
#define ZEN_BLOCKRUN_TARGET_LEN_X2 17 /* 8.5 hops */

/* slots: workgroups the device holds at once (3 per CU).  run_len > 0: runs of at most that many hops; 0: the number of
 * runs of the whole call is the multiple of `slots` that brings the run length closest to 8.5 hops (at least one
 * multiple), shared out evenly among the streams (rounded up per stream, never more runs than hops). */
ZEN_BLOCKRUN_FN zen_blockrun_part zen_blockrun_partition(int n_streams, int n_hops, int slots, int run_len)
{
	zen_blockrun_part p;
	long long rps;
	if (run_len > 0) {
		rps = ((long long)n_hops + run_len - 1) / run_len;
	}
	else {
		const long long total = (long long)n_streams * n_hops;
		long long k = (2 * total + (long long)slots * ZEN_BLOCKRUN_TARGET_LEN_X2 / 2) / ((long long)slots * ZEN_BLOCKRUN_TARGET_LEN_X2);
		if (k < 1)
			k = 1;
		rps = (k * slots + n_streams - 1) / n_streams;
	}
	if (rps > n_hops)
		rps = n_hops;
	if (rps < 1)
		rps = 1;
	p.runs_per_stream = (int)rps;
	p.base_len = n_hops / (int)rps;
	p.n_long = n_hops % (int)rps;
	return p;
}

/* run r (0 .. n_streams * runs_per_stream - 1) -> its stream, first hop and length */
ZEN_BLOCKRUN_FN void zen_blockrun_run(const zen_blockrun_part* p, int run, int* stream, int* first, int* len)
{
	const int s = run / p->runs_per_stream, j = run - s * p->runs_per_stream;
	*stream = s;
	*first = j * p->base_len + (j < p->n_long ? j : p->n_long);
	*len = p->base_len + (j < p->n_long ? 1 : 0);
}

#endif
