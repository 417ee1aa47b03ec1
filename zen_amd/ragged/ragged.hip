// ragged.hip -- the C ABI of libzen_hip_ragged.so (zen_hip_ragged.h): HPRIOffline on a batch of clips of unequal length.
//
// Written on top of the engines' public C ABI (include/zen_hip.h): two zen_hip_hpr_t engines created as zen_hip_hpri_create
// creates its pair, driven through zen_hip_hpr_process on rows zero-padded to the longest clip, with the kernels of
// ragged_kernels.hip in front (pack), between (splice) and behind (trim).  The engines' sources are not touched by this.
// Compared with the fused equal-length path of csrc/hpri.hip (whose overlap-add kernels write every sample where it ends
// up) the intermediates exist in memory here: H1, P1, R1 and P2 are written by the engines and read back by splice / trim.
#include <hip/hip_runtime.h>

#include "zen_hip_ragged.h"

#include "../addon/hpri_pair.h"
#include "ragged_kernels.h"

using namespace zen_addon;
using zen_ragged::tab_t;

namespace {

constexpr int TAB_SLOTS = 4;
enum { K_PACK = 0, K_SPLICE = 1, K_TRIM = 2 };

// The per-clip table of one call: filled in pinned host memory, copied to its device image on the handle's stream.  A
// call that is queued while earlier ones have not run yet must not overwrite what their copies will read: the slots are
// used in turn, and a slot is filled again only after the event behind its previous copy has been reached.
struct TabSlot {
	tab_t *host = nullptr, *host_dev = nullptr, *dev = nullptr;
	hipEvent_t copied = nullptr;
	bool in_flight = false;
};

} // namespace

struct zen_hip_ragged : HpriPair {
	size_t hop_h = 0, hop_p = 0, n_clips = 0;
	hipStream_t stream = nullptr;
	// scratch, grown on demand: the zero-padded input rows, pass 1's outputs, pass 2's input and output
	float *staged = nullptr, *h1 = nullptr, *p1 = nullptr, *r1 = nullptr, *in2 = nullptr, *p2 = nullptr;
	size_t staged_cap = 0, h1_cap = 0, p1_cap = 0, r1_cap = 0, in2_cap = 0, p2_cap = 0; // floats
	TabSlot tab[TAB_SLOTS];
	unsigned next_slot = 0;
	Profiler<3> prof;
};

namespace {

int grow(zen_hip_ragged* h, float*& p, size_t& cap, size_t want)
{
	if (want <= cap)
		return ZEN_HIP_OK;
	ZA_HIP(hipStreamSynchronize(h->stream)); // queued calls may still use the buffer
	(void)zen_hip_free(p);
	p = nullptr; // a failed allocation below must not leave a freed pointer behind a stale capacity
	cap = 0;
	ZA_ZEN(zen_hip_malloc((void**)&p, sizeof(float) * want));
	cap = want;
	return ZEN_HIP_OK;
}

struct Plan {
	size_t max_len = 0, row1 = 0, row2 = 0; // the longest clip; the batch's padded pass-1 / pass-2 lengths (hps.cu:133-134, :180-181)
	const tab_t* tab_dev = nullptr;
	unsigned long long sum_len = 0, sum_q = 0; // samples of the clips; samples of P1 (and of R1) that splice reads
};

// lens -> the per-clip table on the device (asynchronous) and the batch's sizes.  padded1 is monotone in the length, so
// the longest clip has the most hops; the maxima are taken over the clips all the same.
int make_plan(zen_hip_ragged* h, const size_t* lens, Plan* pl)
{
	const size_t C = h->n_clips;
	for (size_t c = 0; c < C; ++c)
		if (lens[c] > pl->max_len)
			pl->max_len = lens[c];
	if (pl->max_len == 0)
		return ZEN_HIP_OK;
	TabSlot& t = h->tab[h->next_slot++ % TAB_SLOTS];
	if (!t.host) {
		ZA_ZEN(zen_hip_host_alloc_mapped(sizeof(tab_t) * 2 * C, 0, (void**)&t.host, (void**)&t.host_dev));
		ZA_ZEN(zen_hip_malloc((void**)&t.dev, sizeof(tab_t) * 2 * C));
		ZA_HIP(hipEventCreateWithFlags(&t.copied, hipEventDisableTiming));
	}
	if (t.in_flight)
		ZA_HIP(hipEventSynchronize(t.copied));
	t.in_flight = false;
	for (size_t c = 0; c < C; ++c) {
		const size_t n = lens[c];
		const size_t pad1 = n ? chunk_padder(n, h->hop_h, h->lag_h) : 0, pad2 = n ? chunk_padder(n, h->hop_p, h->lag_p) : 0;
		t.host[c] = (tab_t)n;
		t.host[C + c] = (tab_t)pad1;
		if (pad1 > pl->row1)
			pl->row1 = pad1;
		if (pad2 > pl->row2)
			pl->row2 = pad2;
	}
	if (pl->row1 == 0 || pl->row2 == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged: clip lengths out of range");
	for (size_t c = 0; c < C; ++c) {
		pl->sum_len += t.host[c];
		pl->sum_q += t.host[C + c] < pl->row2 ? t.host[C + c] : pl->row2;
	}
	ZA_HIP(hipMemcpyAsync(t.dev, t.host, sizeof(tab_t) * 2 * C, hipMemcpyHostToDevice, h->stream));
	ZA_HIP(hipEventRecord(t.copied, h->stream));
	t.in_flight = true;
	pl->tab_dev = t.dev;
	return ZEN_HIP_OK;
}

// Steps 1, 3, 4, 5 (and 6 where perc_dev is given) of a call, on rows that are already in h->staged.
// harm_dev / perc_dev: the caller's result rows or NULL; want_h1 / want_p2: H1 / P2 are wanted in scratch all the same (the
// host call copies the clips' results down from there).
int run_passes(zen_hip_ragged* h, const Plan& pl, float* harm_dev, float* perc_dev, size_t out_stride, bool want_h1, bool want_p2)
{
	const size_t C = h->n_clips, sh1 = h->lag_h * h->hop_h, sh2 = h->lag_p * h->hop_p;
	const bool harm = harm_dev || want_h1, perc = perc_dev || want_p2;
	if (!harm && !perc)
		return ZEN_HIP_OK;
	if (harm)
		ZA_TRY(grow(h, h->h1, h->h1_cap, C * pl.row1));
	if (perc) {
		ZA_TRY(grow(h, h->p1, h->p1_cap, C * pl.row1));
		ZA_TRY(grow(h, h->r1, h->r1_cap, C * pl.row1));
		ZA_TRY(grow(h, h->in2, h->in2_cap, C * pl.row2));
		ZA_TRY(grow(h, h->p2, h->p2_cap, C * pl.row2));
	}
	// pass 1: large hop over the longest clip's hop count (hps.cu:142-167)
	ZA_ZEN(zen_hip_hpr_process(h->e1, h->staged, pl.row1 / h->hop_h, pl.row1, harm ? h->h1 : nullptr, perc ? h->p1 : nullptr,
	                           perc ? h->r1 : nullptr, pl.row1));
	if (perc || harm_dev) {
		auto kt = h->prof.on_stream(h->stream);
		unsigned long long bytes = 0;
		if (perc)
			bytes += sizeof(float) * (2 * pl.sum_q + C * pl.row2);
		if (harm_dev)
			bytes += sizeof(float) * (pl.sum_len + C * pl.max_len);
		ZA_TRY(kt.begin(K_SPLICE, bytes));
		ZA_HIP(zen_ragged::launch_splice(h->h1, h->p1, h->r1, pl.row1, sh1, pl.tab_dev, C, perc ? h->in2 : nullptr, pl.row2, harm_dev,
		                                 out_stride, pl.max_len, h->stream));
		ZA_TRY(kt.end());
	}
	if (!perc)
		return ZEN_HIP_OK;
	// pass 2: small hop on the spliced sum, percussive only (hps.cu:185-205)
	ZA_ZEN(zen_hip_hpr_process(h->e2, h->in2, pl.row2 / h->hop_p, pl.row2, nullptr, h->p2, nullptr, pl.row2));
	if (perc_dev) {
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_TRIM, sizeof(float) * (pl.sum_len + C * pl.max_len)));
		ZA_HIP(zen_ragged::launch_trim(h->p2, pl.row2, sh2, pl.tab_dev, C, perc_dev, out_stride, pl.max_len, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

} // namespace

extern "C" {

const char* zen_hip_ragged_last_error(void) { return t_err; }
const char* zen_hip_ragged_version(void) { return "zen_hip_ragged 1 (gfx950)"; }

int zen_hip_ragged_create(float fs, size_t hop_h, size_t hop_p, float beta_h, float beta_p, int nocopybord, size_t n_clips,
                          zen_hip_ragged_t* h)
{
	if (!h || n_clips == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_create: null handle or zero clips");
	if (hop_p == 0 || hop_h % hop_p != 0) // hps.cu:33-36
		ZA_FAIL(ZEN_HIP_E_HOPS_NOT_DIVISIBLE, "hop_h and hop_p should be evenly divisible");
	zen_hip_ragged* o = new zen_hip_ragged;
	o->hop_h = hop_h;
	o->hop_p = hop_p;
	o->n_clips = n_clips;
	const int rc = pair_create(o, fs, hop_h, hop_p, beta_h, beta_p, nocopybord, n_clips);
	if (rc != ZEN_HIP_OK) {
		set_err("ragged_create: %s", zen_hip_last_error());
		pair_destroy(o);
		delete o;
		return rc;
	}
	*h = o;
	return ZEN_HIP_OK;
}

int zen_hip_ragged_destroy(zen_hip_ragged_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	pair_destroy(h);
	float* bufs[6] = {h->staged, h->h1, h->p1, h->r1, h->in2, h->p2};
	for (float* b : bufs)
		(void)zen_hip_free(b);
	for (TabSlot& t : h->tab) {
		if (t.host)
			(void)zen_hip_host_free(t.host);
		(void)zen_hip_free(t.dev);
		if (t.copied)
			(void)hipEventDestroy(t.copied);
	}
	h->prof.release();
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_ragged_set_stream(zen_hip_ragged_t h, void* stream)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_set_stream: null handle");
	ZA_TRY(pair_set_stream(h, stream));
	ZA_HIP(hipStreamSynchronize(h->stream));
	h->stream = (hipStream_t)stream;
	return ZEN_HIP_OK;
}

int zen_hip_ragged_use_sse_filter(zen_hip_ragged_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	return pair_use_sse_filter(h);
}

int zen_hip_ragged_use_soft_mask(zen_hip_ragged_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	return pair_use_soft_mask(h);
}

int zen_hip_ragged_hop_counts(zen_hip_ragged_t h, size_t max_len, size_t* n_hops_h, size_t* n_hops_p)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	if (n_hops_h)
		*n_hops_h = max_len ? chunk_padder(max_len, h->hop_h, h->lag_h) / h->hop_h : 0;
	if (n_hops_p)
		*n_hops_p = max_len ? chunk_padder(max_len, h->hop_p, h->lag_p) / h->hop_p : 0;
	return ZEN_HIP_OK;
}

int zen_hip_ragged_process_device(zen_hip_ragged_t h, const float* audio_dev, const size_t* lens, size_t stride, float* harm_dev,
                                  float* perc_dev, size_t out_stride)
{
	if (!h || !audio_dev || !lens)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_process_device: null argument");
	if (((uintptr_t)audio_dev & 3) || ((uintptr_t)harm_dev & 3) || ((uintptr_t)perc_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_process_device: float pointers need 4-byte alignment");
	size_t max_len = 0;
	for (size_t c = 0; c < h->n_clips; ++c)
		if (lens[c] > max_len)
			max_len = lens[c];
	if (stride < max_len || out_stride < max_len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_process_device: stride %zu / out_stride %zu below the longest clip (%zu samples)", stride,
		        out_stride, max_len);
	if (max_len == 0 || (!harm_dev && !perc_dev))
		return ZEN_HIP_OK; // empty clips: nothing to write
	Plan pl;
	ZA_TRY(make_plan(h, lens, &pl));
	ZA_TRY(grow(h, h->staged, h->staged_cap, h->n_clips * pl.row1));
	ZA_TRY(pair_reset_buffers(h)); // each call is a fresh pair of HPR objects' state
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_PACK, sizeof(float) * (pl.sum_len + h->n_clips * pl.row1)));
		ZA_HIP(zen_ragged::launch_pack(audio_dev, stride, pl.tab_dev, h->n_clips, h->staged, pl.row1, h->stream));
		ZA_TRY(kt.end());
	}
	return run_passes(h, pl, harm_dev, perc_dev, out_stride, false, false);
}

int zen_hip_ragged_process_host(zen_hip_ragged_t h, const float* const* clips, const size_t* lens, float* const* harm,
                                float* const* perc)
{
	if (!h || !clips || !lens)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_process_host: null argument");
	const size_t C = h->n_clips;
	bool want_h = false, want_p = false;
	for (size_t c = 0; c < C; ++c) {
		if (lens[c] && !clips[c])
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_process_host: clip %zu is null", c);
		want_h = want_h || (harm && harm[c] && lens[c]);
		want_p = want_p || (perc && perc[c] && lens[c]);
	}
	if (!want_h && !want_p)
		return ZEN_HIP_OK;
	Plan pl;
	ZA_TRY(make_plan(h, lens, &pl));
	ZA_TRY(grow(h, h->staged, h->staged_cap, C * pl.row1));
	ZA_TRY(pair_reset_buffers(h)); // each call is a fresh pair of HPR objects' state
	// every clip straight into its row, zeros behind it: no padded matrix on the host, no pack launch
	for (size_t c = 0; c < C; ++c) {
		float* row = h->staged + c * pl.row1;
		if (lens[c])
			ZA_HIP(hipMemcpyAsync(row, clips[c], sizeof(float) * lens[c], hipMemcpyHostToDevice, h->stream));
		if (lens[c] < pl.row1)
			ZA_HIP(hipMemsetAsync(row + lens[c], 0, sizeof(float) * (pl.row1 - lens[c]), h->stream));
	}
	int rc = run_passes(h, pl, nullptr, nullptr, 0, want_h, want_p);
	// the results come down from where the engines wrote them: harm_c = H1_c[sh1 ..], perc_c = P2_c[sh2 ..], lens[c] samples
	const size_t sh1 = h->lag_h * h->hop_h, sh2 = h->lag_p * h->hop_p;
	hipError_t e = hipSuccess;
	for (size_t c = 0; c < C && rc == ZEN_HIP_OK && e == hipSuccess; ++c) {
		if (!lens[c])
			continue;
		if (harm && harm[c])
			e = hipMemcpyAsync(harm[c], h->h1 + c * pl.row1 + sh1, sizeof(float) * lens[c], hipMemcpyDeviceToHost, h->stream);
		if (perc && perc[c] && e == hipSuccess)
			e = hipMemcpyAsync(perc[c], h->p2 + c * pl.row2 + sh2, sizeof(float) * lens[c], hipMemcpyDeviceToHost, h->stream);
	}
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(e);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_ragged_profile(zen_hip_ragged_t h, int enable)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	ZA_TRY(pair_profile(h, enable));
	h->prof.on = enable != 0;
	return ZEN_HIP_OK;
}

int zen_hip_ragged_profile_get(zen_hip_ragged_t h, double ms[3], unsigned long long bytes[3], unsigned long long launches[3])
{
	return profile_get(h, ms, bytes, launches, "ragged");
}

int zen_hip_ragged_profile_get_engine(zen_hip_ragged_t h, int pass, double ms[6], unsigned long long launches[6])
{
	if (!h || (pass != 1 && pass != 2))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "ragged_profile_get_engine: pass must be 1 or 2");
	return pair_profile_get_engine(h, pass, ms, launches);
}

} // extern "C"
