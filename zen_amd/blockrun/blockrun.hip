// blockrun.hip -- zen_hip_blockrun.h: the headline block call routed to the run kernel (blockrun_kernel.hip), every other
// call forwarded to zen_hip_hpr_process.  The host side of a routed call is run_hop_fused's (csrc/hpr.hip) for the one
// configuration the kernel serves: same arguments, same bookkeeping, same profile classes -- the engine cannot tell which
// of the two libraries served a call, and neither can the call after it.
#include "../csrc/hpr_engine.h"
#include "../csrc/masks.h"
#include "blockrun_first_pass.h"
#include "blockrun_kernel.h"
#include "zen_hip_blockrun.h"

#include <atomic>
#include <cstring>
#include <vector>

using namespace zen_hip_impl;

namespace {

std::atomic<int> g_run_len{0}, g_min_items{4096}, g_off{0};
std::atomic<unsigned long long> g_routed{0}, g_forwarded{0};

// hpr.hip's ProfScope: HIP events around a launch, accounted in the engine's own fields (zen_hip_hpr_profile_get* resolves them)
struct ProfScope {
	zen_hip_hpr* e;
	int k;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	ProfScope(zen_hip_hpr* e_, int k_)
	    : e(e_)
	    , k(k_)
	{
		if (!e->prof)
			return;
		if (!e->prof_pool.empty()) {
			e0 = e->prof_pool.back().first;
			e1 = e->prof_pool.back().second;
			e->prof_pool.pop_back();
		}
		else if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
			e0 = e1 = nullptr;
			return;
		}
		(void)hipEventRecord(e0, e->stream);
	}
	~ProfScope()
	{
		if (!e0)
			return;
		(void)hipEventRecord(e1, e->stream);
		e->prof_pending.push_back({k, e0, e1});
		e->prof_launches[k] += 1;
	}
};

// workgroups the device holds at once: three per CU (the kernel's launch bounds and its LDS)
int device_slots(int* slots)
{
	static std::atomic<int> cached[64];
	int dev = 0;
	ZH_HIP(hipGetDevice(&dev));
	int v = (dev >= 0 && dev < 64) ? cached[dev].load() : 0;
	if (v == 0) {
		int cus = 0;
		ZH_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
		v = 3 * (cus > 0 ? cus : 1);
		if (dev >= 0 && dev < 64)
			cached[dev].store(v);
	}
	*slots = v;
	return ZEN_HIP_OK;
}

// Whether the engine's twiddle table (every engine of nfft 4096 builds the same one: make_twiddles, csrc/api.hip) has the
// symmetry the first pass's conjugate shortcut relies on -- checked on the host table, once, before the first launch of the
// run kernel; without it the launch takes the kernel that computes every output of the first pass (blockrun_first_pass.h).
// With it the three entries that pass multiplies with, taken from the same host table.
struct FirstPassTable {
	int symmetric;
	float2 tw16, tw8, tw3_16; // tw[N/16], tw[N/8], tw[3N/16]
};
const FirstPassTable& first_pass_table()
{
	static const FirstPassTable t = [] {
		constexpr int n = zen_blockrun::NFFT;
		std::vector<float> tw(n);
		make_twiddles(tw.data(), tw.size());
		FirstPassTable r;
		r.symmetric = zen_blockrun::table_is_symmetric(tw.data(), n) ? 1 : 0;
		r.tw16 = make_float2(tw[2 * (n / 16)], tw[2 * (n / 16) + 1]);
		r.tw8 = make_float2(tw[2 * (n / 8)], tw[2 * (n / 8) + 1]);
		r.tw3_16 = make_float2(tw[2 * (3 * n / 16)], tw[2 * (3 * n / 16) + 1]);
		return r;
	}();
	return t;
}

bool takes(const zen_hip_hpr* h, const float* in, size_t n_hops, size_t in_stride, const float* harm, const float* perc,
           const float* resid, size_t out_stride)
{
	if (g_off.load() || !h || !in || !perc || harm || resid || n_hops == 0)
		return false;
	// the configuration: causal, nfft 4096 at hop 1024, 47 taps, the percussive output alone, hard mask by comparison
	if (h->causality != ZEN_HIP_TIME_CAUSAL || h->log2n != 12 || h->mf != zen_blockrun::TAPS || h->hop != (size_t)zen_blockrun::HOP
	    || h->nfft != (size_t)zen_blockrun::NFFT || h->nwin != 2 * h->hop)
		return false;
	if (!h->out_p || h->out_h || h->out_r || h->soft || h->use_sse)
		return false;
	// nothing pending that the base would act on first
	if ((h->drain[0] | h->drain[1] | h->drain[2]) || h->rows_stale || h->run_mode || h->res_idle_ms != 0 || h->res_active || h->dbg_stamps)
		return false;
	// the base has served a direct block call of at least this size on this engine: allocation and growth stay its business
	if (!h->d_Y[0] || !h->d_blk_need || !h->d_carry[0] || !h->d_mag || n_hops > h->max_hops)
		return false;
	if (h->n_streams * n_hops < (size_t)g_min_items.load() || h->n_streams * n_hops > 0x3fffffffu)
		return false;
	int inc = 0;
	if (hard_mask_threshold(h->beta, &inc) == 0.0) // (beta outside the comparison's range: the divide builds of the base)
		return false;
	// an output that overlaps the input is left to the base (its overlap-add launch runs after every read of the chunk)
	const size_t S = h->n_streams;
	const char *in0 = (const char*)in, *in1 = (const char*)(in + (S - 1) * in_stride + n_hops * h->hop);
	const char *o0 = (const char*)perc, *o1 = (const char*)(perc + (S - 1) * out_stride + n_hops * h->hop);
	return !(o0 < in1 && in0 < o1);
}

} // namespace

extern "C" int zen_hip_blockrun_process(zen_hip_hpr_t h, const float* in_dev, size_t n_hops, size_t in_stride, float* harm, float* perc,
                                        float* resid, size_t out_stride)
{
	if (!takes(h, in_dev, n_hops, in_stride, harm, perc, resid, out_stride)) {
		g_forwarded.fetch_add(1);
		return zen_hip_hpr_process(h, in_dev, n_hops, in_stride, harm, perc, resid, out_stride);
	}
	g_routed.fetch_add(1);
	int slots = 0;
	ZH_TRY(device_slots(&slots));
	// ---- run_hop_fused (hpr.hip) for M = n_hops, one output, direct delivery
	zen_blockrun::RunArgs a;
	memset(&a, 0, sizeof(a));
	a.in = in_dev;
	a.in_stride = (long long)in_stride;
	a.tail_prev = h->d_tail[h->tail_sel];
	a.tail_next = h->d_tail[h->tail_sel ^ 1];
	a.window = h->d_window;
	a.tw = h->d_tw;
	{
		// the three entries the first analysis pass multiplies with travel as arguments: the same for every thread and frame
		const FirstPassTable& t = first_pass_table();
		a.tw_symmetric = t.symmetric;
		a.tw16 = t.tw16;
		a.tw8 = t.tw8;
		a.tw3_16 = t.tw3_16;
	}
	a.mag = h->d_mag;
	a.keep_mag_rows = (int)h->W - 1;
	a.ring_rows = h->ring_rows;
	a.row0 = h->abs_frame;
	a.n_frames = (int)n_hops;
	a.n_streams = (int)h->n_streams;
	a.prev_frames = (int)h->last_frames;
	a.carry = h->d_carry[0];
	a.Y = h->d_Y[0];
	a.y_stream_stride = (long long)(h->max_hops * h->nwin);
	a.out = perc;
	a.out_stride = (long long)out_stride;
	a.need = h->d_blk_need;
	a.cola = h->cola;
	int inc = 0;
	a.thr = hard_mask_threshold(h->beta, &inc);
	a.part = zen_blockrun_partition(a.n_streams, a.n_frames, slots, g_run_len.load());
	for (int o = 0; o < 3; ++o) {
		h->ready_valid[o] = false;
		h->direct_done[o] = false;
	}
	{
		ProfScope ps(h, zen_hip_hpr::K_FUSED);
		ZH_TRY(zen_blockrun::launch_run(a, h->stream));
	}
	{
		ProfScope ps(h, zen_hip_hpr::K_FINALIZE);
		ZH_TRY(zen_blockrun::launch_fixup(a, h->stream));
	}
	h->tail_sel ^= 1;
	h->abs_frame += (long long)n_hops;
	h->last_frames = n_hops;
	return ZEN_HIP_OK;
}

extern "C" int zen_hip_blockrun_set(const char* key, int value)
{
	if (!key || value < 0)
		ZH_FAIL(ZEN_HIP_E_BAD_ARG, "blockrun_set: null key or negative value");
	if (!strcmp(key, "run_len"))
		g_run_len.store(value);
	else if (!strcmp(key, "min_items"))
		g_min_items.store(value);
	else if (!strcmp(key, "off"))
		g_off.store(value);
	else
		ZH_FAIL(ZEN_HIP_E_BAD_ARG, "blockrun_set: unknown key '%s' (run_len, min_items, off)", key);
	return ZEN_HIP_OK;
}

extern "C" int zen_hip_blockrun_stats(unsigned long long* routed, unsigned long long* forwarded)
{
	if (routed)
		*routed = g_routed.load();
	if (forwarded)
		*forwarded = g_forwarded.load();
	return ZEN_HIP_OK;
}
