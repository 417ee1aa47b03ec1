// live.hip -- the C ABI of libzen_hip_live.so (zen_hip_live.h): HPRIOffline as a bounded-latency stream.
//
// Written on top of the engines' public C ABI (include/zen_hip.h), as ragged.hip is: two zen_hip_hpr_t engines created as
// zen_hip_hpri_create creates its pair, driven through zen_hip_hpr_process one slice of whole blocks at a time, with the
// kernels of live_kernels.hip in front (feed), between (mid) and behind (out).  The engines carry their own state from
// call to call; what this file carries is the partial block, the H1 delay, the dry ring and four counters.
//
// One slice (at most max_push new samples; s0 = the samples pass 1 has consumed so far, all streams in lock step):
//   feed   X = carry ++ new samples; b = |X| / hop_h whole blocks -> in1 rows, the rest -> the other carry buffer
//   pass 1 b blocks: H1 -> behind the history in the current H1 buffer, P1, R1            stream positions [s0, s0 + b*hop_h)
//   mid    in2 = (P1 + R1)[max(s0, sh1) ..]; the last samples of [history | H1] -> the other H1 buffer's history
//   pass 2 everything in in2                                                             in2 positions [t0, t0 + len2)
//   out    perc = P2[d + sh2], harm = H1[d + sh1] (sh2 samples back: the history), dry = ring[d]      d in [delivered, ...)
// finish is the same slice with zeros for new samples, run up to padded1 / padded2 with the reference's end mapping.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "zen_hip_live.h"

#include "../addon/hpri_pair.h"
#include "live_kernels.h"

using namespace zen_addon;

namespace {

enum { K_FEED = 0, K_MID = 1, K_OUT = 2 };

size_t round4(size_t x) { return (x + 3) & ~(size_t)3; }

unsigned long long max_samples(size_t hop_p) // zen_hip_live.h, "The bound"
{
	const unsigned long long two24 = 1ull << 24;
	if (hop_p && (hop_p & (hop_p - 1)) == 0 && hop_p < two24)
		return two24 * hop_p - 1;
	return two24;
}

} // namespace

struct zen_hip_live : HpriPair, Handle<3> {
	size_t hop_h = 0, hop_p = 0, S = 0, sh1 = 0, sh2 = 0, max_push = 0;
	// rows per stream (floats): pass 1's largest slice, pass 2's, the most one call delivers, the history in front of H1
	size_t cap1 = 0, cap2 = 0, ocap = 0, hoff = 0, row1 = 0, carry_row = 0, dry_len = 0;
	float *carry[2] = {nullptr, nullptr}, *in1 = nullptr, *h1[2] = {nullptr, nullptr}, *p1 = nullptr, *r1 = nullptr, *in2 = nullptr,
	      *p2 = nullptr, *dry = nullptr;
	float *stage_in = nullptr, *stage_out[3] = {nullptr, nullptr, nullptr}; // the host calls' device rows
	int cur_carry = 0, cur_h1 = 0;
	// the stream so far
	unsigned long long pushed = 0, delivered = 0, limit = 0;
	size_t c = 0; // samples in the carry: pushed % hop_h
};

namespace {

int alloc(zen_hip_live* h, float** p, size_t floats)
{
	return counted_malloc(&h->mem, (void**)p, sizeof(float) * floats, "zen_hip_malloc((void**)p, sizeof(float) * floats)");
}

unsigned long long delivered_after(const zen_hip_live* h, unsigned long long pushed)
{
	const unsigned long long done = pushed / h->hop_h * h->hop_h, lat = h->sh1 + h->sh2;
	return done > lat ? done - lat : 0;
}

int reset_session(zen_hip_live* h)
{
	ZA_TRY(pair_reset_buffers(h));
	h->pushed = h->delivered = 0;
	h->c = 0;
	return ZEN_HIP_OK;
}

// the source rows must hold every index the mapping names for positions [first, first + cnt)
bool covers(const zen_live::Shifted& q, size_t first, size_t cnt, size_t row_len)
{
	if (cnt == 0)
		return true;
	const size_t last = first + cnt - 1;
	auto ok = [&](size_t lo, size_t hi, long long off) { // positions [lo, hi] with this offset
		return (long long)lo + off >= 0 && (long long)hi + off < (long long)row_len;
	};
	if (first < q.shifted_end && !ok(first, last < q.shifted_end ? last : q.shifted_end - 1, q.off_shifted))
		return false;
	if (last >= q.shifted_end && first < q.stale_end) {
		const size_t lo = first > q.shifted_end ? first : q.shifted_end;
		if (lo < q.stale_end && !ok(lo, last < q.stale_end ? last : q.stale_end - 1, q.off_stale))
			return false;
	}
	return true;
}

// One slice: m new samples per stream at in_dev (finish: m == 0 and `fin`, the stream runs to its padded ends).  Writes
// *produced samples of each non-NULL output.  The counters are advanced only when everything has been queued.
int run_slice(zen_hip_live* h, const float* in_dev, size_t m, size_t in_stride, float* harm, float* perc, float* dry, size_t out_stride,
              bool fin, size_t* produced)
{
	const size_t H = h->hop_h, P = h->hop_p, sh1 = h->sh1, sh2 = h->sh2, S = h->S;
	const size_t NONE = SIZE_MAX;
	const unsigned long long n = h->pushed; // finish: the length of the stream
	const size_t s0 = (size_t)(h->pushed - h->c); // = blocks so far * hop_h
	size_t len1, c_next, pad1 = NONE, pad2 = NONE;
	if (fin) {
		pad1 = chunk_padder((size_t)n, H, h->lag_h);
		pad2 = chunk_padder((size_t)n, P, h->lag_p);
		if (pad1 < s0 + sh1 || pad1 - s0 > h->cap1)
			ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "live_finish: %llu samples: pass 1 would end at %zu, %zu are done", n, pad1, s0);
		len1 = pad1 - s0;
		c_next = 0;
	} else {
		len1 = (h->c + m) / H * H;
		c_next = h->c + m - len1;
	}
	const size_t s1 = s0 + len1;
	// pass 2's input: in2 positions [t0, t1)
	const size_t t0 = s0 > sh1 ? s0 - sh1 : 0;
	size_t t1 = fin ? pad2 : (s1 > sh1 ? s1 - sh1 : 0);
	if (t1 < t0)
		t1 = t0; // (finish of a stream whose pass 2 already is beyond padded2 cannot happen below the bound; checked by `covers`)
	const size_t len2 = t1 - t0;
	// what this slice delivers: positions [d0, d1)
	const size_t d0 = (size_t)h->delivered;
	const size_t d1 = fin ? (size_t)n : (size_t)delivered_after(h, h->pushed + m);
	const size_t cnt = d1 - d0;
	if (len2 > h->cap2 || cnt > h->ocap || len1 > h->cap1 || len2 % P != 0)
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "live: slice of %zu / %zu / %zu samples beyond the session's rows", len1, len2, cnt);

	float *hcur = h->h1[h->cur_h1], *hnext = h->h1[h->cur_h1 ^ 1];
	zen_live::Shifted q = {h->p1, h->row1, fin ? pad1 - sh1 : NONE, fin ? pad1 : NONE, (long long)sh1 - (long long)s0, -(long long)s0};
	zen_live::Shifted sp2 = {h->p2, h->cap2, fin ? (pad2 > sh2 ? pad2 - sh2 : 0) : NONE, fin ? pad2 : NONE,
	                         (long long)sh2 - (long long)t0, -(long long)t0};
	zen_live::Shifted sh = {hcur, h->row1, fin ? pad1 - sh1 : NONE, fin ? pad1 : NONE,
	                        (long long)sh1 - (long long)s0 + (long long)h->hoff, -(long long)s0 + (long long)h->hoff};
	if (!covers(q, t0, len2, len1) || !covers(sp2, d0, cnt, len2) || !covers(sh, d0, cnt, h->hoff + len1))
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "live: %llu samples: the end mapping leaves the rows of this slice", n);

	{
		zen_live::FeedArgs a = {};
		a.in = in_dev, a.in_stride = in_stride, a.m = m;
		a.carry_cur = h->carry[h->cur_carry], a.carry_next = h->carry[h->cur_carry ^ 1], a.carry_stride = h->carry_row;
		a.c = h->c, a.c_next = c_next;
		a.in1 = h->in1, a.in1_stride = h->cap1, a.len1 = len1;
		a.dry = h->dry, a.dry_stride = h->dry_len, a.dry_len = h->dry_len, a.dry_pos = (size_t)(h->pushed % h->dry_len);
		a.n_streams = S;
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_FEED, sizeof(float) * S * (h->c + 2 * m + len1 + c_next + m)));
		ZA_HIP(zen_live::launch_feed(a, h->stream));
		ZA_TRY(kt.end());
	}
	if (len1)
		ZA_ZEN(zen_hip_hpr_process(h->e1, h->in1, len1 / H, h->cap1, hcur + h->hoff, h->p1, h->r1, h->row1));
	if (len1 || len2) { // (len1 == 0 < len2: a finish whose pass 2 only has zeros left to read)
		zen_live::MidArgs a = {};
		a.p = q, a.r1 = h->r1;
		a.in2 = h->in2, a.in2_stride = h->cap2, a.len2 = len2, a.t0 = t0;
		a.hist_cur = hcur, a.hist_next = hnext, a.hist_stride = h->row1, a.hist_from = len1, a.hist_len = fin || !len1 ? 0 : h->hoff;
		a.n_streams = S;
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_MID, sizeof(float) * S * (3 * len2 + 2 * a.hist_len)));
		ZA_HIP(zen_live::launch_mid(a, h->stream));
		ZA_TRY(kt.end());
	}
	if (len2)
		ZA_ZEN(zen_hip_hpr_process(h->e2, h->in2, len2 / P, h->cap2, nullptr, h->p2, nullptr, h->cap2));
	if (cnt) {
		zen_live::OutArgs a = {};
		a.p2 = sp2, a.h1 = sh;
		a.dry = h->dry, a.dry_stride = h->dry_len, a.dry_len = h->dry_len, a.dry_pos = d0 % h->dry_len;
		a.harm_out = harm, a.perc_out = perc, a.dry_out = dry;
		a.out_stride = out_stride, a.cnt = cnt, a.d0 = d0;
		a.n_streams = S;
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_OUT, sizeof(float) * S * cnt * 2 * ((harm != nullptr) + (perc != nullptr) + (dry != nullptr))));
		ZA_HIP(zen_live::launch_out(a, h->stream));
		ZA_TRY(kt.end());
	}
	h->cur_carry ^= 1;
	if (len1)
		h->cur_h1 ^= 1;
	h->pushed += m;
	h->c = c_next;
	h->delivered = d1;
	*produced = cnt;
	return ZEN_HIP_OK;
}

int check_rows(const char* who, zen_hip_live_t h, const void* in, size_t m, size_t in_stride, const void* harm, const void* perc,
               const void* dry, size_t out_stride, size_t will_produce)
{
	if (m && !in)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input", who);
	if (((uintptr_t)in & 3) || ((uintptr_t)harm & 3) || ((uintptr_t)perc & 3) || ((uintptr_t)dry & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if (in_stride < m || ((harm || perc || dry) && out_stride < will_produce))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: in_stride %zu / out_stride %zu below the %zu samples pushed / %zu produced", who, in_stride,
		        out_stride, m, will_produce);
	if (h->pushed + m > h->limit)
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "%s: a stream of %llu samples is beyond the %llu the float padder of these hops supports", who,
		        h->pushed + (unsigned long long)m, h->limit);
	return ZEN_HIP_OK;
}

int push_device(zen_hip_live_t h, const float* in_dev, size_t m, size_t in_stride, float* harm, float* perc, float* dry,
                size_t out_stride, size_t* produced)
{
	size_t total = 0;
	size_t off = 0;
	do { // (a push of nothing is one empty slice)
		const size_t ms = m - off < h->max_push ? m - off : h->max_push;
		size_t got = 0;
		ZA_TRY(run_slice(h, ms ? in_dev + off : in_dev, ms, in_stride, harm ? harm + total : nullptr, perc ? perc + total : nullptr,
		                 dry ? dry + total : nullptr, out_stride, false, &got));
		total += got;
		off += ms;
	} while (off < m);
	if (produced)
		*produced = total;
	return ZEN_HIP_OK;
}

int finish_device(zen_hip_live_t h, float* harm, float* perc, float* dry, size_t out_stride, size_t* produced)
{
	size_t got = 0;
	if (h->pushed)
		ZA_TRY(run_slice(h, nullptr, 0, 0, harm, perc, dry, out_stride, true, &got));
	ZA_TRY(reset_session(h));
	if (produced)
		*produced = got;
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host memory (rows host_stride apart) and the staging rows (dev_stride apart)
int copy_rows(zen_hip_live* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, hipMemcpyKind kind)
{
	return h->copy_rows(dst, dst_stride, src, src_stride, cnt, h->S, kind);
}

} // namespace

extern "C" {

const char* zen_hip_live_last_error(void) { return t_err; }
const char* zen_hip_live_version(void) { return "zen_hip_live 1 (gfx950)"; }

int zen_hip_live_max_samples(size_t hop_h, size_t hop_p, unsigned long long* out)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_max_samples: null argument");
	if (hop_p == 0 || hop_h % hop_p != 0)
		ZA_FAIL(ZEN_HIP_E_HOPS_NOT_DIVISIBLE, "hop_h and hop_p should be evenly divisible");
	*out = max_samples(hop_p);
	return ZEN_HIP_OK;
}

int zen_hip_live_create(float fs, size_t hop_h, size_t hop_p, float beta_h, float beta_p, int nocopybord, size_t n_streams,
                        size_t max_push, zen_hip_live_t* out)
{
	if (!out || n_streams == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_create: null handle or zero streams");
	if (hop_p == 0 || hop_h % hop_p != 0) // hps.cu:33-36
		ZA_FAIL(ZEN_HIP_E_HOPS_NOT_DIVISIBLE, "hop_h and hop_p should be evenly divisible");
	zen_hip_live* h = new zen_hip_live;
	h->hop_h = hop_h;
	h->hop_p = hop_p;
	h->S = n_streams;
	h->max_push = max_push ? max_push : hop_h;
	h->limit = max_samples(hop_p);
	auto build = [&]() -> int {
		ZA_TRY(pair_create(h, fs, hop_h, hop_p, beta_h, beta_p, nocopybord, n_streams));
		h->sh1 = h->lag_h * hop_h;
		h->sh2 = h->lag_p * hop_p;
		const size_t lat = h->sh1 + h->sh2;
		size_t blocks = (h->max_push + hop_h - 1) / hop_h; // the carry holds at most hop_h - 1 samples
		if (blocks < h->lag_h + 1)
			blocks = h->lag_h + 1; // finish: up to ceil(n / hop_h) - n / hop_h + lag_h blocks
		h->cap1 = blocks * hop_h;
		h->cap2 = (lat + hop_h + hop_p + hop_p - 1) / hop_p * hop_p; // finish: fewer than sh1 + sh2 + hop_h + hop_p samples of in2
		if (h->cap2 < h->cap1)
			h->cap2 = h->cap1;
		h->ocap = h->cap1 > lat + hop_h ? h->cap1 : lat + hop_h;
		h->hoff = round4(h->sh2);
		h->row1 = h->hoff + h->cap1;
		h->carry_row = round4(hop_h);
		h->dry_len = round4(lat + hop_h + h->max_push);
		const size_t S = n_streams;
		ZA_TRY(alloc(h, &h->carry[0], S * h->carry_row));
		ZA_TRY(alloc(h, &h->carry[1], S * h->carry_row));
		ZA_TRY(alloc(h, &h->in1, S * h->cap1));
		ZA_TRY(alloc(h, &h->h1[0], S * h->row1));
		ZA_TRY(alloc(h, &h->h1[1], S * h->row1));
		ZA_TRY(alloc(h, &h->p1, S * h->row1));
		ZA_TRY(alloc(h, &h->r1, S * h->row1));
		ZA_TRY(alloc(h, &h->in2, S * h->cap2));
		ZA_TRY(alloc(h, &h->p2, S * h->cap2));
		ZA_TRY(alloc(h, &h->dry, S * h->dry_len));
		ZA_TRY(alloc(h, &h->stage_in, S * h->max_push));
		for (float*& p : h->stage_out)
			ZA_TRY(alloc(h, &p, S * h->ocap));
		// the engines' growth up front: each runs its largest block once, on zeros
		ZA_HIP(hipMemsetAsync(h->in1, 0, sizeof(float) * S * h->cap1, h->stream));
		ZA_HIP(hipMemsetAsync(h->in2, 0, sizeof(float) * S * h->cap2, h->stream));
		ZA_ZEN(zen_hip_hpr_process(h->e1, h->in1, h->cap1 / hop_h, h->cap1, h->h1[0] + h->hoff, h->p1, h->r1, h->row1));
		ZA_ZEN(zen_hip_hpr_process(h->e2, h->in2, h->cap2 / hop_p, h->cap2, nullptr, h->p2, nullptr, h->cap2));
		ZA_TRY(reset_session(h));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_live_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_live_destroy(zen_hip_live_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	pair_destroy(h);
	h->release({h->carry[0], h->carry[1], h->in1, h->h1[0], h->h1[1], h->p1, h->r1, h->in2, h->p2, h->dry, h->stage_in, h->stage_out[0],
	            h->stage_out[1], h->stage_out[2]});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_live_set_stream(zen_hip_live_t h, void* stream)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_set_stream: null handle");
	ZA_TRY(pair_set_stream(h, stream));
	ZA_HIP(hipStreamSynchronize(h->stream));
	h->stream = (hipStream_t)stream;
	return ZEN_HIP_OK;
}

int zen_hip_live_use_sse_filter(zen_hip_live_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	if (h->pushed)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_use_sse_filter: the stream has begun (%llu samples pushed)", h->pushed);
	return pair_use_sse_filter(h);
}

int zen_hip_live_use_soft_mask(zen_hip_live_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	if (h->pushed)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_use_soft_mask: the stream has begun (%llu samples pushed)", h->pushed);
	return pair_use_soft_mask(h);
}

int zen_hip_live_reset(zen_hip_live_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	return reset_session(h);
}

int zen_hip_live_latency(zen_hip_live_t h, size_t* samples)
{
	if (!h || !samples)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_latency: null argument");
	*samples = h->sh1 + h->sh2;
	return ZEN_HIP_OK;
}

int zen_hip_live_produces(zen_hip_live_t h, size_t m, size_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_produces: null argument");
	*out = (size_t)(delivered_after(h, h->pushed + m) - h->delivered);
	return ZEN_HIP_OK;
}

int zen_hip_live_pending(zen_hip_live_t h, size_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_pending: null argument");
	*out = (size_t)(h->pushed - h->delivered);
	return ZEN_HIP_OK;
}

int zen_hip_live_push_device(zen_hip_live_t h, const float* in_dev, size_t m, size_t in_stride, float* harm_dev, float* perc_dev,
                             float* dry_dev, size_t out_stride, size_t* produced)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_push_device: null handle");
	ZA_TRY(check_rows("live_push_device", h, in_dev, m, in_stride, harm_dev, perc_dev, dry_dev, out_stride,
	                  (size_t)(delivered_after(h, h->pushed + m) - h->delivered)));
	return push_device(h, in_dev, m, in_stride, harm_dev, perc_dev, dry_dev, out_stride, produced);
}

int zen_hip_live_finish_device(zen_hip_live_t h, float* harm_dev, float* perc_dev, float* dry_dev, size_t out_stride, size_t* produced)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_finish_device: null handle");
	ZA_TRY(check_rows("live_finish_device", h, nullptr, 0, 0, harm_dev, perc_dev, dry_dev, out_stride, (size_t)(h->pushed - h->delivered)));
	return finish_device(h, harm_dev, perc_dev, dry_dev, out_stride, produced);
}

int zen_hip_live_push_host(zen_hip_live_t h, const float* in_host, size_t m, size_t in_stride, float* harm_host, float* perc_host,
                           float* dry_host, size_t out_stride, size_t* produced)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_push_host: null handle");
	ZA_TRY(check_rows("live_push_host", h, in_host, m, in_stride, harm_host, perc_host, dry_host, out_stride,
	                  (size_t)(delivered_after(h, h->pushed + m) - h->delivered)));
	float* host[3] = {harm_host, perc_host, dry_host};
	size_t total = 0;
	int rc = ZEN_HIP_OK;
	size_t off = 0;
	do { // slice by slice through the staging rows
		const size_t ms = m - off < h->max_push ? m - off : h->max_push;
		size_t got = 0;
		rc = copy_rows(h, h->stage_in, h->max_push, in_host ? in_host + off : nullptr, in_stride, ms, hipMemcpyHostToDevice);
		if (rc == ZEN_HIP_OK)
			rc = run_slice(h, h->stage_in, ms, h->max_push, host[0] ? h->stage_out[0] : nullptr, host[1] ? h->stage_out[1] : nullptr,
			               host[2] ? h->stage_out[2] : nullptr, h->ocap, false, &got);
		for (int o = 0; o < 3 && rc == ZEN_HIP_OK; ++o)
			if (host[o])
				rc = copy_rows(h, host[o] + total, out_stride, h->stage_out[o], h->ocap, got, hipMemcpyDeviceToHost);
		// (the next slice overwrites the staging rows: stream order keeps that behind these copies)
		total += got;
		off += ms;
	} while (rc == ZEN_HIP_OK && off < m);
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	if (produced)
		*produced = total;
	return ZEN_HIP_OK;
}

int zen_hip_live_finish_host(zen_hip_live_t h, float* harm_host, float* perc_host, float* dry_host, size_t out_stride, size_t* produced)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_finish_host: null handle");
	ZA_TRY(check_rows("live_finish_host", h, nullptr, 0, 0, harm_host, perc_host, dry_host, out_stride, (size_t)(h->pushed - h->delivered)));
	float* host[3] = {harm_host, perc_host, dry_host};
	size_t got = 0;
	int rc = finish_device(h, host[0] ? h->stage_out[0] : nullptr, host[1] ? h->stage_out[1] : nullptr,
	                       host[2] ? h->stage_out[2] : nullptr, h->ocap, &got);
	for (int o = 0; o < 3 && rc == ZEN_HIP_OK; ++o)
		if (host[o])
			rc = copy_rows(h, host[o], out_stride, h->stage_out[o], h->ocap, got, hipMemcpyDeviceToHost);
	const hipError_t es = hipStreamSynchronize(h->stream);
	ZA_TRY(rc);
	ZA_HIP(es);
	if (produced)
		*produced = got;
	return ZEN_HIP_OK;
}

int zen_hip_live_stats(zen_hip_live_t h, zen_hip_live_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_stats: null argument");
	out->pushed = h->pushed;
	out->delivered = h->delivered;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_live_profile(zen_hip_live_t h, int enable)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	ZA_TRY(pair_profile(h, enable));
	h->prof.on = enable != 0;
	return ZEN_HIP_OK;
}

int zen_hip_live_profile_get(zen_hip_live_t h, double ms[3], unsigned long long bytes[3], unsigned long long launches[3])
{
	return profile_get(h, ms, bytes, launches, "live");
}

int zen_hip_live_profile_get_engine(zen_hip_live_t h, int pass, double ms[6], unsigned long long launches[6])
{
	if (!h || (pass != 1 && pass != 2))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "live_profile_get_engine: pass must be 1 or 2");
	return pair_profile_get_engine(h, pass, ms, launches);
}

} // extern "C"
