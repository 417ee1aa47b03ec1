// blockrun_kernel.hip -- the headline block call with one workgroup per RUN of consecutive hops of a stream.
//
// rt_fused.hip's block build runs one workgroup per hop; the overlap-add crosses workgroups, so every workgroup pays, per
// hop and serially, for its arguments and index arithmetic, for two publication words and 8 KB of another workgroup's Y
// rows in front of its first butterfly, and for a drained memory counter, a barrier and a publication behind its last
// store.  Here a workgroup walks a run of hops: per frame the same arithmetic in the same order (the functors below are
// rt_fused.hip's, the transforms, the median and the mask are the shared headers'), and between the frames of a run
//   - the frame's second half stays in LDS and is added to the next frame's first half: the finished hop leaves as plain
//     stores nobody waits for;
//   - the frame's new input hop is the next frame's previous hop: kept in LDS, not loaded again;
//   - the next hop's four samples per thread are requested before the inverse transform and used after it.
// Every thread owns the same four positions of a hop in all three roles (idx = slot * 256 + tf of the forward transform's
// first pass and of the inverse transform's last), so the carry, the kept hop and the window sit in words of LDS only
// their thread touches: no barrier is spent on them.
// The engine's state is left as rt_fused.hip leaves it (every Y row, the input tail, the last magnitude rows, the
// previous call's carry); the first hop of every run is marked in `need` and added up by the fix-up launch.
#include "../csrc/common.h"
#include "../csrc/fft_dev.h"
#include "../csrc/masks.h"
#include "../csrc/median47_core.h"
#include "../csrc/median_net.h"
#include "blockrun_kernel.h"
#include "blockrun_first_pass.h"
#include "blockrun_edge_count.h"

#pragma clang fp contract(off)

namespace zen_blockrun {
namespace {

using zen_hip_impl::hard_mask_exact;
using PL = zfft::Plan<12>;
constexpr int N = PL::N, TF = PL::TF;
static_assert(N == NFFT && TF == 256 && HOP == 4 * TF, "four samples of a hop per thread");

// the magnitude image of the median stage: 16-word chunks 20 words apart, column k at word k + 24 (median47_core.h)
constexpr int MID = TAPS / 2, MID_AL = 24, IMG_END = 255 * 16 + 64;
__device__ __forceinline__ int img_addr(int g) { return (g >> 4) * zm47::RSTR + (g & 15); }
// the mirrored columns the median stage reads: those of bins 1 .. MIR_LO and N/2 - MIR_HI .. N/2 - 1 (FwdOut)
constexpr int MIR_LO = 56, MIR_HI = 39;
static_assert(N - MIR_LO <= 16 * 254 - 24 && N / 2 + MIR_HI >= 16 * 128 + 39, "blocks 254 / 255 and 126 .. 128 read written columns");
static_assert(EDGE_IMG_COL0 == MID_AL && EDGE_IMG_RSTR == zm47::RSTR && EDGE_OUTPUTS == MID + 1, "blockrun_edge_count.h reads this image");
// rt_fused.hip's lean layout inside the frame image: the compact P row and the wave-edge records
constexpr int PC_WORD = 5184, PC_TAIL = 2052, EDGE_WORD = PC_WORD + PC_TAIL + 512 + 4;
static_assert((EDGE_WORD + 256) * 4 <= PL::LDS_FLOAT2 * 8, "lean layout must fit in the frame image");
// behind the frame image, per thread: the kept hop, the carry (4 words each) and the window (8 words), word m * 256 + tf
constexpr int KEEP_WORD = PL::LDS_FLOAT2 * 2, CARRY_WORD = KEEP_WORD + HOP, WIN_WORD = CARRY_WORD + HOP;
constexpr size_t LDS_BYTES = (size_t)(WIN_WORD + 2 * HOP) * 4;
static_assert(LDS_BYTES <= LDS_BYTES_MAX, "three workgroups per CU");

__device__ __forceinline__ void lds_barrier()
{
	// the workgroup exchanges through LDS only: its counter drained, then the barrier (__syncthreads() would also wait for
	// every global load and store in flight: the next hop's samples, the rows and the hop stored in the background)
	asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// fft_dev.h's TwGlobal with the table entry addressed as (uniform base, 32-bit byte offset): the same entries, and the
// loads take their address from two scalar registers and one vector register instead of a 64-bit vector pair each --
// a dozen registers the kernel does not have at three workgroups per CU
struct TwGlobal32 {
	static constexpr bool PLAIN = true;
	static constexpr bool PACKED = true;
	const float2* __restrict__ p;
	__device__ __forceinline__ float2 get(int, int, int, int idx) const
	{
		return *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(p) + (unsigned)(idx << 3));
	}
};

struct Spec {
	float2 S[16]; // the frame's spectrum, bins tf + slot * TF
};

struct FwdInPre { // rt_fused.hip: the eight samples and window values of the thread in registers
	float x[8], w[8];
	__device__ __forceinline__ float2 operator()(int, int slot) const { return make_float2(x[slot] * w[slot], 0.0f); } // window_functor hps.h:24-33
};

// rt_fused.hip FwdOut<16, 256> without the rings (the magnitude ring's rows are copied from the image) and without the
// mirrored columns nobody reads.  The median stage selects columns 0 .. 2047 of the P row (blocks 0 .. 127, waves 0 and 1)
// and counts the masks of columns 2048 and 4073 .. 4095 from the lower half (blockrun_edge_count.h, wave 3); a block t reads
// columns 16t - 24 .. 16t + 39, so of the upper half of the row blocks 126 / 127 (wave 1's last lanes) read up to column
// 2055 / 2071 (the edge record of blocks 128 and 129, sorted by wave 2's lanes 0 and 1; chunk 130): the mirrors of bins
// 2025 .. 2047.  The stores cover more (bins 2009 .. 2047: slot 7, tf >= 217; bins 1 .. 56: slot 0, 1 <= tf <= 56, and the
// border replica of column 4095), as when a third median stream read them.  Wave 2's other lanes (blocks 130 .. 191) sort
// whatever the image holds there (words of the image, never outside it) and their records are not read.  InvIn and the
// magnitude rows take |S[k]| of the upper half from the mirrored lower column.  Bin N/2 belongs to thread 0 alone.
struct FwdOut {
	Spec* r;
	int* img;
	__device__ __forceinline__ void operator()(int idx, float2 X, bool lower, int slot) const
	{
		r->S[slot] = X;
		if (slot == 8) {
			// bin N/2 is thread 0's alone: a branch waves 1 .. 3 skip, not a magnitude every thread computes and drops
			if (__builtin_amdgcn_readfirstlane(idx) < (N >> 1) + 64 && idx == (N >> 1))
				img[img_addr((N >> 1) + MID_AL)] = __float_as_int(zfft::cabs_exact(X.x, X.y));
		}
		else if (lower) {
			const float m = zfft::cabs_exact(X.x, X.y); // complex_abs_functor hps.h:82-89
			const int key = __float_as_int(m);
			constexpr int CH = (TF / 16) * zm47::RSTR;
			const int tfl = idx - slot * TF;
			img[img_addr(tfl + MID_AL) + slot * CH] = key;
			if (slot == 0 && tfl >= 1 && tfl <= MIR_LO)
				img[img_addr(N - tfl + MID_AL)] = key;
			if (slot == 7 && tfl >= TF - MIR_HI)
				img[img_addr(N - 7 * TF - tfl + MID_AL)] = key;
		}
	}
};

struct InvIn { // rt_fused.hip InvInLean<4096, 256, 23, true>
	const Spec* r;
	const int* img;
	const float* pc;
	double thr;
	__device__ __forceinline__ float2 operator()(int idx, int slot) const
	{
		const int lo = slot * TF, hi = lo + TF - 1;
		int pi;
		if (hi <= N / 2)
			pi = idx;
		else if (lo > N / 2 && hi < N - MID)
			pi = N - idx;
		else
			pi = (idx > N / 2 && idx < N - MID) ? N - idx : (idx > N / 2 ? idx - (N - 512) + PC_TAIL : idx);
		// |S[idx]|: column idx of the image, for the upper half of the Hermitian row column N - idx (FwdOut)
		// (N - idx = (15 - slot) * TF + TF - tf: one base per half, the slot in the instruction's offset)
		const int g0 = hi <= N / 2 ? idx + 24 - slot * TF : TF + 24 - (idx - slot * TF);
		const float mag = __int_as_float(img[(g0 >> 4) * 20 + (g0 & 15) + (hi <= N / 2 ? slot : 15 - slot) * (TF / 16) * 20]);
		const float2 z = r->S[slot];
		const float p = pc[pi];
		float m = hard_mask_exact(p, mag + FLT_EPSILON, thr);
		// bin N/2 and the bins N - 23 .. N - 1: the word holds the mask itself (blockrun_edge_count.h), slots 8 and 15 only
		if (hi > N / 2 && !(lo > N / 2 && hi < N - MID))
			m = (idx == N / 2 || idx >= N - MID) ? p : m;
		return make_float2(z.x * m, z.y * m); // apply_mask_functor hps.h:58-66
	}
};

struct InvOut {
	float* Y;      // the frame's row
	float* out;    // the hop this frame finishes (first frame of a run: zeros in the carry; the fix-up launch stores the hop again)
	float* carry;  // LDS, this thread's words: second half of the previous frame in, of this frame out
	float cola;
	__device__ __forceinline__ void operator()(int idx, float2 x, bool, int slot) const
	{
		const float y = x.x * cola;
		ZH_CHK(Y + idx, 1);
		Y[idx] = y;
		if (slot < 4) {
			ZH_CHK(out + idx, 1);
			out[idx] = carry[(slot & 3) * TF] + y; // hps.cu:435-449, :526-528
		}
		else {
			carry[(slot & 3) * TF] = y;
		}
	}
};

// SYM: the twiddle table has the symmetry first_pass16's conjugate shortcut needs (blockrun_first_pass.h)
template <bool SYM>
__device__ __forceinline__ void run_body(const RunArgs& a)
{
	extern __shared__ float2 lds[];
	int* img = reinterpret_cast<int*>(lds);
	float* Prow = reinterpret_cast<float*>(img + PC_WORD);
	const int tf = (int)threadIdx.x;
	float* keep = reinterpret_cast<float*>(img + KEEP_WORD) + tf;
	float* carry = reinterpret_cast<float*>(img + CARRY_WORD) + tf;
	float* win = reinterpret_cast<float*>(img + WIN_WORD) + tf;

	int s, f0, len;
	zen_blockrun_run(&a.part, (int)blockIdx.x, &s, &f0, &len);
	if (s >= a.n_streams || f0 + len > a.n_frames) // (a launch larger than its partition: nothing to do)
		return;
	const float* cur = a.in + (long long)s * a.in_stride + (long long)f0 * HOP;
	float* Yrow = a.Y + (long long)s * a.y_stream_stride + (long long)f0 * (2 * HOP);
	float* orow = a.out + (long long)s * a.out_stride + (long long)f0 * HOP;

	// ---- once per run: the previous call's carry (rt_fused.hip's housekeeping: the workgroup that overwrites that row, or
	// the call's last, saves its second half first), the hop before the run, the window, the first frame's new hop
	if (a.prev_frames > 0) {
		const int fc = a.prev_frames - 1 < a.n_frames - 1 ? a.prev_frames - 1 : a.n_frames - 1;
		if (fc >= f0 && fc < f0 + len) {
			const float* y = a.Y + (long long)s * a.y_stream_stride + (long long)(a.prev_frames - 1) * (2 * HOP) + HOP;
			float v[4];
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				ZH_CHK(y + tf + i * TF, 1);
				v[i] = y[tf + i * TF];
			}
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				ZH_CHK(a.carry + ((long long)s * HOP + tf + i * TF), 1);
				a.carry[(long long)s * HOP + tf + i * TF] = v[i];
			}
		}
	}
	float nx[4];
	{
		const float* pv = f0 > 0 ? cur - HOP : a.tail_prev + (long long)s * HOP;
		float p[4], w[8];
#pragma unroll
		for (int m = 0; m < 4; ++m) {
			ZH_CHK(pv + m * TF + tf, 1);
			ZH_CHK(cur + m * TF + tf, 1);
			p[m] = pv[m * TF + tf];
			nx[m] = cur[m * TF + tf];
		}
#pragma unroll
		for (int m = 0; m < 8; ++m) {
			ZH_CHK(a.window + m * TF + tf, 1);
			w[m] = a.window[m * TF + tf];
		}
#pragma unroll
		for (int m = 0; m < 4; ++m) {
			keep[m * TF] = p[m];
			carry[m * TF] = 0.0f;
		}
#pragma unroll
		for (int m = 0; m < 8; ++m)
			win[m * TF] = w[m];
	}
	if (tf == 0) {
		ZH_CHK(a.need + ((long long)s * a.n_frames + f0), 1);
		a.need[(long long)s * a.n_frames + f0] = 1u; // the run's first hop: its other half belongs to another workgroup (or the carry)
	}

	const int tf_run = tf;
	for (int k = 0; k < len; ++k) {
		const int f = f0 + k;
		// opaque per frame (as rt_fused.hip has it per output): otherwise every LDS address and twiddle of the two transforms,
		// all functions of the thread index alone, is hoisted out of the loop and kept in registers the kernel does not have
		int tf = tf_run, tw_off = 0;
		asm volatile("" : "+v"(tf));
		tf &= TF - 1; // (known to be a small non-negative number again: addresses stay 32-bit offsets from scalar bases)
		asm volatile("" : "+s"(tw_off));
		const float2* tw = a.tw + tw_off;
		float* keep = reinterpret_cast<float*>(img + KEEP_WORD) + tf;
		float* carry = reinterpret_cast<float*>(img + CARRY_WORD) + tf;
		float* win = reinterpret_cast<float*>(img + WIN_WORD) + tf;
		// ---- analysis: hps.cu:452-472, :492
		Spec r;
		{
			FwdInPre pre;
#pragma unroll
			for (int m = 0; m < 4; ++m) {
				pre.x[m] = keep[m * TF];
				pre.x[4 + m] = nx[m];
			}
#pragma unroll
			for (int m = 0; m < 8; ++m)
				pre.w[m] = win[m * TF];
#pragma unroll
			for (int m = 0; m < 4; ++m)
				keep[m * TF] = nx[m]; // this frame's new hop is the next frame's previous hop
			if (f == a.n_frames - 1) { // the call's last frame hands its new hop to the next call
				float* tail = a.tail_next + (long long)s * HOP;
#pragma unroll
				for (int m = 0; m < 4; ++m) {
					ZH_CHK(tail + m * TF + tf, 1);
					tail[m * TF + tf] = nx[m];
				}
			}
			FwdOut out;
			out.r = &r;
			out.img = img;
			// pass 0 as the real 16-point transform it is (blockrun_first_pass.h), its results where PassRunner<12, 0, ...>
			// puts them (autosort layout: output c of thread tf at element tf + c * N/16); the runner goes on from pass 1
			{
				float p[8];
#pragma unroll
				for (int m = 0; m < 8; ++m)
					p[m] = pre.x[m] * pre.w[m]; // window_functor hps.h:24-33
				float2 Y0[16];
				first_pass16<true, SYM>(p, a.tw16, a.tw8, a.tw3_16, Y0); // (the table's entries as arguments: scalar registers)
#pragma unroll
				for (int c = 0; c < 16; ++c)
					lds[PL::pad_off(tf, c * (N / 16))] = Y0[c];
				zfft::frame_sync<TF>();
			}
			zfft::PassRunner<12, 1, false, true, false, FwdInPre, FwdOut, false, TwGlobal32>::run(tf, lds, TwGlobal32{tw}, pre, out, true);
		}
		lds_barrier();
		// A later use_sse_filter() reads the magnitude rows of the stft_width-1 frames before it: the call's last frames store
		// theirs, from the image (column k at word k + 24 holds the bits of |S[k]|, k <= N/2; the upper half of the Hermitian row mirrors it)
		if (f >= a.n_frames - a.keep_mag_rows) {
			float* mag = a.mag + (((a.row0 + f) % a.ring_rows) + (long long)s * a.ring_rows) * N;
			for (int g = tf; g < N; g += TF) {
				ZH_CHK(mag + g, 1);
				mag[g] = __int_as_float(img[img_addr((g <= N / 2 ? g : N - g) + MID_AL)]);
			}
		}
		// replicate border of the magnitude row (ippBorderRepl)
		{
			const int v0 = img[img_addr(MID_AL)], v1 = img[img_addr(N - 1 + MID_AL)];
			for (int g = tf; g < MID_AL; g += TF)
				img[img_addr(g)] = v0;
			for (int g = N + MID_AL + tf; g < IMG_END; g += TF)
				img[img_addr(g)] = v1;
		}
		lds_barrier();
		// ---- percussive estimate: frequency-direction median of the row (hps.cu:496).  Waves 0 and 1 filter blocks 0 .. 127.
		// Wave 2 sorts blocks 128 .. 191 for the edge record of wave 1's last lanes (the sorted block 128 and the pieces of
		// blocks 128 and 129; its other lanes' records are not read) and selects nothing.  Wave 3 counts the masks of bin N/2
		// and of the bins N - 23 .. N - 1 while the others sort (blockrun_edge_count.h): InvIn reads them as they stand.
		{
			int(*edge)[64] = reinterpret_cast<int(*)[64]>(img + EDGE_WORD);
			const int lane = tf & 63, wave = __builtin_amdgcn_readfirstlane(tf >> 6);
			zm47::Pieces pc;
			if (wave < 3) {
				zm47::m47_sort_and_publish(img, edge, tf, lane, wave, tf == 0, false, pc);
			}
			else {
				const unsigned bits = edge_count_wave(img, lane, a.thr, N / 2);
				if (lane < EDGE_OUTPUTS)
					Prow[lane == 0 ? N / 2 : PC_TAIL + 512 - lane] = (bits >> lane) & 1u ? 1.0f : 0.0f;
			}
			lds_barrier();
			if (wave < 2) {
				int o[16];
				zm47::m47_select(img, edge, tf, wave, pc, o);
#pragma unroll
				for (int v = 0; v < 4; ++v)
					*reinterpret_cast<int4*>(&Prow[tf * 16 + 4 * v]) = make_int4(o[4 * v], o[4 * v + 1], o[4 * v + 2], o[4 * v + 3]);
			}
		}
		lds_barrier(); // P row complete
		// ---- the next hop's samples: on their way while the inverse transform runs
		cur += HOP;
		if (k + 1 < len) {
#pragma unroll
			for (int m = 0; m < 4; ++m) {
				ZH_CHK(cur + m * TF + tf, 1);
				nx[m] = cur[m * TF + tf];
			}
		}
		// ---- synthesis: hps.cu:498-528 (H = |S| of the same row: causal)
		{
			// (opaque again: what the two transforms share -- twiddle offsets, image addresses -- is computed twice instead of
			// living in registers through the median stage, which has none to spare)
			asm volatile("" : "+v"(tf));
			asm volatile("" : "+s"(tw_off));
			tf &= TF - 1;
			tw = a.tw + tw_off;
			carry = reinterpret_cast<float*>(img + CARRY_WORD) + tf;
			InvIn in;
			in.r = &r;
			in.img = img;
			in.pc = Prow;
			in.thr = a.thr;
			InvOut out;
			out.Y = Yrow;
			out.out = orow;
			out.carry = carry;
			out.cola = a.cola;
			zfft::PassRunner<12, 0, true, false, true, InvIn, InvOut, true, TwGlobal32>::run(tf, lds, TwGlobal32{tw}, in, out, true);
		}
		Yrow += 2 * HOP;
		orow += HOP;
	}
}

__global__ __launch_bounds__(256, 3) void blockrun_kernel(RunArgs a) { run_body<true>(a); }
// the same for a table without the symmetry: outputs 9 .. 15 of the first pass computed one by one
__global__ __launch_bounds__(256, 3) void blockrun_kernel_plain_table(RunArgs a) { run_body<false>(a); }

// the hops the run kernel left: out = (previous frame's second half, or the carry for the first hop of the call) + this
// frame's first half -- rt_fused.hip's fix-up for one output; one wavefront per item, all marks read side by side
__global__ __launch_bounds__(256) void blockrun_fixup_kernel(RunArgs a)
{
	const long long total = (long long)a.n_streams * a.n_frames;
	const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (item >= total)
		return;
	ZH_CHK(a.need + item, 1);
	if (!a.need[item])
		return;
	const int s = (int)(item / a.n_frames), f = (int)(item - (long long)s * a.n_frames);
	const float* Y = a.Y + (long long)s * a.y_stream_stride + (long long)f * (2 * HOP);
	const float* prev = f == 0 ? a.carry + (long long)s * HOP : Y - HOP;
	float* o = a.out + (long long)s * a.out_stride + (long long)f * HOP;
	// (a run kernel leaves three times the hops rt_fused.hip's hand-off leaves: 16 bytes per lane and access where the
	// caller's rows allow it -- the engine's own rows always do)
	if (((reinterpret_cast<uintptr_t>(o) | reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(Y)) & 15) == 0) {
		float4 p[HOP / 256], y[HOP / 256];
#pragma unroll
		for (int i = 0; i < HOP / 256; ++i) {
			const int k = i * 256 + lane * 4;
			ZH_CHK(prev + k, 4);
			ZH_CHK(Y + k, 4);
			p[i] = *reinterpret_cast<const float4*>(prev + k);
			y[i] = *reinterpret_cast<const float4*>(Y + k);
		}
#pragma unroll
		for (int i = 0; i < HOP / 256; ++i) {
			const int k = i * 256 + lane * 4;
			ZH_CHK(o + k, 4);
			*reinterpret_cast<float4*>(o + k) = make_float4(p[i].x + y[i].x, p[i].y + y[i].y, p[i].z + y[i].z, p[i].w + y[i].w);
		}
	}
	else {
		for (int k = lane; k < HOP; k += 64) {
			ZH_CHK(o + k, 1);
			ZH_CHK(prev + k, 1);
			ZH_CHK(Y + k, 1);
			o[k] = prev[k] + Y[k];
		}
	}
	if (lane == 0)
		a.need[item] = 0u;
}

} // namespace

size_t run_kernel_lds_bytes() { return LDS_BYTES; }

int launch_run(const RunArgs& a, hipStream_t stream)
{
	const long long runs = (long long)a.n_streams * a.part.runs_per_stream;
	if (a.tw_symmetric)
		hipLaunchKernelGGL(blockrun_kernel, dim3((unsigned)runs), dim3(TF), LDS_BYTES, stream, a);
	else
		hipLaunchKernelGGL(blockrun_kernel_plain_table, dim3((unsigned)runs), dim3(TF), LDS_BYTES, stream, a);
	ZH_HIP(hipGetLastError());
	return ZEN_HIP_OK;
}

int launch_fixup(const RunArgs& a, hipStream_t stream)
{
	const long long total = (long long)a.n_streams * a.n_frames;
	hipLaunchKernelGGL(blockrun_fixup_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, stream, a);
	ZH_HIP(hipGetLastError());
	return ZEN_HIP_OK;
}

} // namespace zen_blockrun
