// beat.hip -- the C ABI of libzen_hip_beat.so (zen_hip_beat.h): the complex-domain onset function and the beat tracker
// on hops of device rows.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as pitch.hip is: the transform is
// zen_hip_fft_exec_batched on a 2 hop-point handle, memory comes from zen_hip_malloc, and the kernels of beat_kernels.hip
// stand in front (frame) and behind (csd, track).
//
// One slice (at most max_hops hops of every stream; spectrum group g = the n_streams rows of one frame):
//   frame    hop c and the hop in front of it, windowed and rotated -> group 2 + c
//   fft      N-point FFT of the groups 2 .. 2 + hops, in place, one batch
//   csd      groups c, c + 1, c + 2 -> the onset value of hop c
//   carry    the last two groups -> groups 0 and 1, the last hop of samples -> tail
//   track    one workgroup per stream walks the onset values of the slice -> the caller's rows
#include <hip/hip_runtime.h>

#include <cstdint>

#include "zen_hip_beat.h"

#include "../addon/addon_host.h"
#include "beat_kernels.h"
#include "beat_tables.h"

using namespace zen_addon;

namespace {

enum { K_FRAME = 0, K_FFT = 1, K_CSD = 2, K_TRACK = 3, K_COUNT = ZEN_HIP_BEAT_KERNELS };

} // namespace

struct zen_hip_beat : Handle<K_COUNT> {
	float fs = 0.f;
	size_t hop = 0, S = 0, max_hops = 0;
	int bp[zen_beat::TEMPI] = {};
	zen_hip_fft_t fft = nullptr; // 2 hop points
	float* rows = nullptr;     // (max_hops + 2) groups of S rows of 2 hop complex values
	float* tail = nullptr;     // S rows of hop samples: the hop in front of the next call
	float* odf = nullptr;      // S rows of max_hops onset values
	float* tables = nullptr;   // beat_tables.h's device copy
	float* state = nullptr;    // S * STATE_WORDS words
	float* stage_in = nullptr; // the host calls' device rows: S rows of max_hops * hop samples
	float* stage_out[4] = {nullptr, nullptr, nullptr, nullptr}; // S rows of max_hops results
	std::vector<float> state0; // the state of a fresh session (reset copies it up: it must outlive the copy)
	unsigned long long hops = 0, slices = 0;
};

namespace {

size_t group_floats(const zen_hip_beat* h) { return h->S * 4 * h->hop; }

// `cs` hops of every stream: `in` is the first of them, c0 its index in the caller's output rows
int run_slice(zen_hip_beat* h, const float* in, size_t in_stride, size_t c0, size_t cs, float* odf, float* score, float* beat, float* tempo,
              size_t out_stride)
{
	const size_t hop = h->hop, S = h->S, rows = S * cs, g = group_floats(h);
	const unsigned long long row_bytes = sizeof(float) * 4 * hop; // one spectrum row
	{
		zen_beat::FrameArgs a = {in, h->tail, h->tables + zen_beat::OFF_WINDOW, h->rows, in_stride, cs, S, (int)hop};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_FRAME, rows * (sizeof(float) * 2 * hop + row_bytes)));
		ZA_HIP(zen_beat::launch_frame(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_FFT, rows * 2 * row_bytes));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows + 2 * g, rows, 0, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_beat::CsdArgs a = {h->rows, h->odf, h->max_hops, cs, S, (int)hop};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_CSD, rows * (3 * row_bytes + sizeof(float))));
		ZA_HIP(zen_beat::launch_csd(a, h->stream));
		ZA_TRY(kt.end());
	}
	// what the next slice or call finds in front of it.  Two groups move down by cs groups: one copy where they do not
	// overlap their destination, group by group in stream order where cs is 1.
	if (cs >= 2) {
		ZA_ZEN(zen_hip_memcpy_d2d(h->rows, h->rows + cs * g, sizeof(float) * 2 * g, h->stream));
	} else {
		ZA_ZEN(zen_hip_memcpy_d2d(h->rows, h->rows + g, sizeof(float) * g, h->stream));
		ZA_ZEN(zen_hip_memcpy_d2d(h->rows + g, h->rows + 2 * g, sizeof(float) * g, h->stream));
	}
	ZA_HIP(hipMemcpy2DAsync(h->tail, sizeof(float) * hop, in + (cs - 1) * hop, sizeof(float) * in_stride, sizeof(float) * hop, S,
	                        hipMemcpyDeviceToDevice, h->stream));
	{
		zen_beat::TrackArgs a = {h->odf, h->max_hops, h->tables, h->state, odf, score, beat, tempo, out_stride, c0, cs, S};
		auto kt = h->prof.on_stream(h->stream);
		const int outs = (odf != nullptr) + (score != nullptr) + (beat != nullptr) + (tempo != nullptr);
		ZA_TRY(kt.begin(K_TRACK, rows * sizeof(float) * (1 + outs) + S * 2 * sizeof(float) * zen_beat::STATE_WORDS));
		ZA_HIP(zen_beat::launch_track(a, h->stream));
		ZA_TRY(kt.end());
	}
	h->hops += rows;
	h->slices += 1;
	return ZEN_HIP_OK;
}

int check_rows(const char* who, zen_hip_beat_t h, const void* in, size_t in_stride, size_t n_hops, const void* odf, const void* score,
               const void* beat, const void* tempo, size_t out_stride)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (n_hops && !in)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input", who);
	if (((uintptr_t)in & 3) || ((uintptr_t)odf & 3) || ((uintptr_t)score & 3) || ((uintptr_t)beat & 3) || ((uintptr_t)tempo & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if (n_hops > SIZE_MAX / sizeof(float) / h->hop || in_stride < n_hops * h->hop)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: in_stride %zu below the %zu hops of %zu samples of a row", who, in_stride, n_hops, h->hop);
	if ((odf || score || beat || tempo) && out_stride < n_hops)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu hops of a row", who, out_stride, n_hops);
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host and device memory
int copy_rows(zen_hip_beat* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, hipMemcpyKind kind)
{
	return h->copy_rows(dst, dst_stride, src, src_stride, cnt, h->S, kind);
}

// df = 1 at the multiples of the first period, cs = 0, prev = 1 | b, m0, bc, j, head
std::vector<float> fresh_state(const zen_hip_beat* h)
{
	using namespace zen_beat;
	std::vector<float> st(h->S * STATE_WORDS, 0.0f);
	const int b = h->bp[20], ints[5] = {b, 10, -1, 20, 0};
	for (size_t s = 0; s < h->S; ++s) {
		float* p = st.data() + s * STATE_WORDS;
		for (int i = 0; i < HISTORY; i += b)
			p[i] = 1.0f;
		for (int i = 0; i < TEMPI; ++i)
			p[2 * HISTORY + i] = 1.0f;
		memcpy(p + 2 * HISTORY + TEMPI, ints, sizeof(ints));
	}
	return st;
}

int reset(zen_hip_beat* h)
{
	ZA_HIP(hipMemsetAsync(h->rows, 0, sizeof(float) * 2 * group_floats(h), h->stream));
	ZA_HIP(hipMemsetAsync(h->tail, 0, sizeof(float) * h->S * h->hop, h->stream));
	ZA_HIP(hipMemcpyAsync(h->state, h->state0.data(), sizeof(float) * h->state0.size(), hipMemcpyHostToDevice, h->stream));
	return ZEN_HIP_OK;
}

} // namespace

extern "C" {

const char* zen_hip_beat_last_error(void) { return t_err; }
const char* zen_hip_beat_version(void) { return "zen_hip_beat 1 (gfx950)"; }

int zen_hip_beat_create(float fs, size_t hop, size_t n_streams, size_t max_hops, zen_hip_beat_t* out)
{
	if (!out || n_streams == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_create: null handle or zero streams");
	if (!zen_beat::is_pow2(hop) || hop < 64 || hop > 2048)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_create: hop %zu is not a power of two in 64..2048", hop);
	int bp[zen_beat::TEMPI];
	if (!zen_beat::periods(fs, hop, bp))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_create: at %g Hz and hop %zu the beat periods of 80..160 bpm do not lie in 4..128 hops", (double)fs, hop);
	if (max_hops == 0)
		max_hops = 4096;
	if (max_hops > ((size_t)1 << 20) || n_streams > ((size_t)1 << 20))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_create: max_hops %zu or n_streams %zu above 2^20", max_hops, n_streams);
	zen_hip_beat* h = new zen_hip_beat;
	h->fs = fs;
	h->hop = hop;
	h->S = n_streams;
	h->max_hops = max_hops;
	memcpy(h->bp, bp, sizeof(bp));
	auto build = [&]() -> int {
		const size_t rows = n_streams * max_hops;
		const std::vector<float> tab = zen_beat::device_tables(fs, hop, bp);
		h->state0 = fresh_state(h);
		ZA_ZEN(zen_hip_fft_create(2 * hop, &h->fft));
		ZA_TRY(h->alloc(&h->rows, (max_hops + 2) * group_floats(h)));
		ZA_TRY(h->alloc(&h->tail, n_streams * hop));
		ZA_TRY(h->alloc(&h->odf, rows));
		ZA_TRY(h->alloc(&h->tables, tab.size()));
		ZA_TRY(h->alloc(&h->state, h->state0.size()));
		ZA_TRY(h->alloc(&h->stage_in, rows * hop));
		for (float*& p : h->stage_out)
			ZA_TRY(h->alloc(&p, rows));
		ZA_ZEN(zen_hip_memcpy_h2d(h->tables, tab.data(), sizeof(float) * tab.size()));
		// whatever the transform allocates for its largest batch, up front: one run on zeros
		ZA_HIP(hipMemsetAsync(h->rows, 0, sizeof(float) * (max_hops + 2) * group_floats(h), h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows + 2 * group_floats(h), rows, 0, h->stream));
		ZA_TRY(reset(h));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_beat_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_beat_destroy(zen_hip_beat_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft);
	h->release({h->rows, h->tail, h->odf, h->tables, h->state, h->stage_in, h->stage_out[0], h->stage_out[1], h->stage_out[2], h->stage_out[3]});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_beat_reset(zen_hip_beat_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_reset: null handle");
	return reset(h);
}

int zen_hip_beat_set_stream(zen_hip_beat_t h, void* stream) { return set_stream(h, stream, "beat"); }

int zen_hip_beat_run_device(zen_hip_beat_t h, const float* in_dev, size_t in_stride, size_t n_hops, float* odf_dev, float* score_dev,
                            float* beat_dev, float* tempo_dev, size_t out_stride)
{
	ZA_TRY(check_rows("beat_run_device", h, in_dev, in_stride, n_hops, odf_dev, score_dev, beat_dev, tempo_dev, out_stride));
	for (size_t c0 = 0; c0 < n_hops; c0 += h->max_hops) {
		const size_t cs = n_hops - c0 < h->max_hops ? n_hops - c0 : h->max_hops;
		ZA_TRY(run_slice(h, in_dev + c0 * h->hop, in_stride, c0, cs, odf_dev, score_dev, beat_dev, tempo_dev, out_stride));
	}
	return ZEN_HIP_OK;
}

int zen_hip_beat_run_host(zen_hip_beat_t h, const float* in_host, size_t in_stride, size_t n_hops, float* odf_host, float* score_host,
                          float* beat_host, float* tempo_host, size_t out_stride)
{
	ZA_TRY(check_rows("beat_run_host", h, in_host, in_stride, n_hops, odf_host, score_host, beat_host, tempo_host, out_stride));
	const size_t hop = h->hop, stage_row = h->max_hops * hop;
	float* host[4] = {odf_host, score_host, beat_host, tempo_host};
	int rc = ZEN_HIP_OK;
	for (size_t c0 = 0; c0 < n_hops && rc == ZEN_HIP_OK; c0 += h->max_hops) {
		const size_t cs = n_hops - c0 < h->max_hops ? n_hops - c0 : h->max_hops;
		// Up: the hops of the slice.  Down: its results.  The next slice overwrites the staging rows: stream order keeps
		// that behind these copies.
		rc = copy_rows(h, h->stage_in, stage_row, in_host + c0 * hop, in_stride, cs * hop, hipMemcpyHostToDevice);
		if (rc == ZEN_HIP_OK)
			rc = run_slice(h, h->stage_in, stage_row, 0, cs, host[0] ? h->stage_out[0] : nullptr, host[1] ? h->stage_out[1] : nullptr,
			               host[2] ? h->stage_out[2] : nullptr, host[3] ? h->stage_out[3] : nullptr, h->max_hops);
		for (int o = 0; o < 4 && rc == ZEN_HIP_OK; ++o)
			if (host[o])
				rc = copy_rows(h, host[o] + c0, out_stride, h->stage_out[o], h->max_hops, cs, hipMemcpyDeviceToHost);
	}
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_beat_stats(zen_hip_beat_t h, zen_hip_beat_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_stats: null argument");
	out->hops = h->hops;
	out->slices = h->slices;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_beat_profile(zen_hip_beat_t h, int enable) { return profile(h, enable); }

int zen_hip_beat_profile_get(zen_hip_beat_t h, double ms[ZEN_HIP_BEAT_KERNELS], unsigned long long bytes[ZEN_HIP_BEAT_KERNELS],
                             unsigned long long launches[ZEN_HIP_BEAT_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "beat");
}

int zen_hip_beat_table(float fs, size_t hop, int which, size_t index, float* out, size_t cap)
{
	using namespace zen_beat;
	int bp[TEMPI];
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_table: null output");
	if (!periods(fs, hop, bp))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_table: (%g Hz, hop %zu) is not a pair create accepts", (double)fs, hop);
	bool is_period = false;
	for (int j = 0; j < TEMPI; ++j)
		is_period = is_period || (size_t)bp[j] == index;
	const int b = (int)(is_period ? index : 0);
	size_t len = 0;
	switch (which) {
	case ZEN_HIP_BEAT_TABLE_WINDOW: len = 2 * hop; break;
	case ZEN_HIP_BEAT_TABLE_PERIOD:
	case ZEN_HIP_BEAT_TABLE_TEMPO: len = TEMPI; break;
	case ZEN_HIP_BEAT_TABLE_PAST:
	case ZEN_HIP_BEAT_TABLE_FUTURE:
		if (!is_period)
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_table: %zu is none of the beat periods of (%g Hz, hop %zu)", index, (double)fs, hop);
		len = which == ZEN_HIP_BEAT_TABLE_PAST ? (size_t)(r2_of(b) - rh_of(b) + 1) : (size_t)b;
		break;
	case ZEN_HIP_BEAT_TABLE_RAYLEIGH: len = 128; break;
	case ZEN_HIP_BEAT_TABLE_TRANSITION:
		if (index >= (size_t)TEMPI)
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_table: row %zu of the 41 of the transition matrix", index);
		len = TEMPI;
		break;
	default: ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_table: unknown table %d", which);
	}
	if (cap < len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "beat_table: room for %zu floats, the table has %zu", cap, len);
	for (size_t i = 0; i < len; ++i) {
		switch (which) {
		case ZEN_HIP_BEAT_TABLE_WINDOW: out[i] = window_at(i, 2 * hop); break;
		case ZEN_HIP_BEAT_TABLE_PERIOD: out[i] = (float)bp[i]; break;
		case ZEN_HIP_BEAT_TABLE_TEMPO: out[i] = tempo_at(fs, hop, bp[i]); break;
		case ZEN_HIP_BEAT_TABLE_PAST: out[i] = past_at(b, (int)i); break;
		case ZEN_HIP_BEAT_TABLE_FUTURE: out[i] = future_at(b, (int)i); break;
		case ZEN_HIP_BEAT_TABLE_RAYLEIGH: out[i] = rayleigh_at((int)i); break;
		default: out[i] = transition_at((int)index, (int)i); break;
		}
	}
	return ZEN_HIP_OK;
}

} // extern "C"
