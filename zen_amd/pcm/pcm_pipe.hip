// pcm_pipe.hip -- the C ABI of libzen_hip_pcm.so (zen_hip_pcm.h): the kernels on device pointers, and the two
// host-to-host calls that put them between 2- or 3-byte copies and the float engines of libzen_hip.so.
//
// One pipeline, two callers.  run_pieces is the three-stream pattern of zen_hip_hpr_process_host / zen_hip_hpri_process
// (csrc/hpr.hip, csrc/hpri.hip) on top of the engines' public C ABI: piece k+1 goes up and is widened on the upload stream,
// piece k runs on the engine's stream, piece k-1 is narrowed and comes down on the download stream.  The two entry points
// check their arguments, size the pieces and supply what their engine differs in.  The engines' sources are not touched by
// this; folding this pipeline into theirs is left to a change that can carry a fuzz run.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "zen_hip_pcm.h"

#include "../addon/addon_host.h"
#include "../csrc/host_pipe.h" // host_pinned, Registered: shared with the float pipelines
#include "pcm_convert.h"
#include "pcm_kernels.h"

using namespace zen_addon;
using zen_hip_impl::Registered;

namespace {

thread_local zen_hip_pcm_host_stats t_stats = {};

double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

size_t ceil_div(size_t a, size_t b) { return (a + b - 1) / b; }

// ---- per-handle context ------------------------------------------------------------------------------------------------
enum { KIND_HPR = 0, KIND_HPRI = 1 };

struct Ctx {
	int kind = KIND_HPR;
	hipStream_t run = nullptr, s_in = nullptr, s_out = nullptr; // run: the stream the engine is put on
	uint8_t* inb = nullptr; // the input as it came up, in its format
	size_t inb_cap = 0;     // bytes
	float* fin = nullptr;
	size_t fin_cap = 0;
	float* fout[3] = {nullptr, nullptr, nullptr}; // harmonic, percussive, residual
	size_t fout_cap[3] = {0, 0, 0};
	uint8_t* outb[3] = {nullptr, nullptr, nullptr}; // the outputs in their format, on their way down
	size_t outb_cap[3] = {0, 0, 0};                 // bytes
	float* minmax = nullptr;                             // 3 x (min, max) on the device
	float *minmax_host = nullptr, *minmax_host_dev = nullptr; // their pinned landing place
	std::vector<hipEvent_t> ev;
};

std::mutex g_mu;
std::unordered_map<void*, Ctx*> g_ctx;

int ctx_for(void* handle, int kind, Ctx** out)
{
	std::lock_guard<std::mutex> lk(g_mu);
	Ctx*& c = g_ctx[handle];
	if (!c)
		c = new Ctx;
	c->kind = kind; // (a context left behind by a destroyed engine whose address a new handle took over serves that one)
	if (!c->run)
		ZA_HIP(hipStreamCreateWithFlags(&c->run, hipStreamNonBlocking));
	if (!c->s_in)
		ZA_HIP(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
	if (!c->s_out)
		ZA_HIP(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
	if (!c->minmax)
		ZA_ZEN(zen_hip_malloc((void**)&c->minmax, 6 * sizeof(float)));
	if (!c->minmax_host)
		ZA_ZEN(zen_hip_host_alloc_mapped(6 * sizeof(float), 0, (void**)&c->minmax_host, (void**)&c->minmax_host_dev));
	*out = c;
	return ZEN_HIP_OK;
}

int sync_all(Ctx* c)
{
	const hipError_t a = hipStreamSynchronize(c->s_out), b = hipStreamSynchronize(c->run), d = hipStreamSynchronize(c->s_in);
	ZA_HIP(a);
	ZA_HIP(b);
	ZA_HIP(d);
	return ZEN_HIP_OK;
}

template <typename T>
int grow(Ctx* c, T*& p, size_t& cap, size_t want)
{
	if (want <= cap)
		return ZEN_HIP_OK;
	ZA_TRY(sync_all(c));
	(void)zen_hip_free(p);
	p = nullptr; // a failed allocation below must not leave a freed pointer behind a stale capacity
	cap = 0;
	ZA_ZEN(zen_hip_malloc((void**)&p, sizeof(T) * want));
	cap = want;
	return ZEN_HIP_OK;
}

int need_events(Ctx* c, size_t n)
{
	while (c->ev.size() < n) {
		hipEvent_t e;
		ZA_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
		c->ev.push_back(e);
	}
	return ZEN_HIP_OK;
}

void free_ctx(Ctx* c)
{
	if (c->run)
		(void)hipStreamSynchronize(c->run);
	if (c->s_in)
		(void)hipStreamSynchronize(c->s_in);
	if (c->s_out)
		(void)hipStreamSynchronize(c->s_out);
	(void)zen_hip_free(c->inb);
	(void)zen_hip_free(c->fin);
	for (int o = 0; o < 3; ++o) {
		(void)zen_hip_free(c->fout[o]);
		(void)zen_hip_free(c->outb[o]);
	}
	(void)zen_hip_free(c->minmax);
	if (c->minmax_host)
		(void)zen_hip_host_free(c->minmax_host);
	for (hipEvent_t e : c->ev)
		(void)hipEventDestroy(e);
	if (c->run)
		(void)hipStreamDestroy(c->run);
	if (c->s_in)
		(void)hipStreamDestroy(c->s_in);
	if (c->s_out)
		(void)hipStreamDestroy(c->s_out);
	delete c;
}

struct Span {
	const char* p;
	size_t bytes;
};

bool any_overlap(const Span* s, int count)
{
	for (int i = 0; i < count; ++i)
		for (int j = i + 1; j < count; ++j)
			if (s[i].p && s[j].p && s[i].p < s[j].p + s[j].bytes && s[j].p < s[i].p + s[i].bytes)
				return true;
	return false;
}

// the never-written residual of HPRIOffline: zeros, by a few host threads beside the pipeline (as csrc/hpri.hip does)
void zero_host(uint8_t* dst, size_t bytes)
{
	const size_t n = bytes, piece = (size_t)64 << 20;
	unsigned k = (unsigned)(bytes / piece);
	const unsigned hw = std::thread::hardware_concurrency();
	if (k > 8)
		k = 8;
	if (hw && k > hw / 2)
		k = hw / 2;
	if (k < 2) {
		memset(dst, 0, bytes);
		return;
	}
	std::vector<std::thread> th;
	const size_t per = (n / k + 1023) & ~(size_t)1023;
	size_t done_to = 0; // a thread that cannot be started leaves its piece (and the rest) to this one
	for (unsigned i = 0; i < k; ++i) {
		const size_t a = (size_t)i * per, b = a + per < n ? a + per : n;
		if (a >= b)
			break;
		try {
			th.emplace_back([=] { memset(dst + a, 0, b - a); });
			done_to = b;
		}
		catch (...) {
			break;
		}
	}
	if (done_to < n)
		memset(dst + done_to, 0, n - done_to);
	for (auto& t : th)
		t.join();
}

int check_fmt(const char* who, const char* which, int fmt)
{
	if (!pcm_sample_bytes(fmt))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %s format must be ZEN_HIP_PCM_I16 or ZEN_HIP_PCM_I24 (got %d)", who, which, fmt);
	return ZEN_HIP_OK;
}

int check_mode_channels(const char* who, int channels, int mode)
{
	if (channels != 1 && channels != 2)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: channels must be 1 or 2 (got %d)", who, channels);
	if (mode != ZEN_HIP_PCM_PEAK && mode != ZEN_HIP_PCM_GAIN)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: mode must be ZEN_HIP_PCM_PEAK or ZEN_HIP_PCM_GAIN (got %d)", who, mode);
	return ZEN_HIP_OK;
}

// ---- the piece pipeline ----------------------------------------------------------------------------------------------------
struct Job {
	int in_fmt, out_fmt; // ZEN_HIP_PCM_I16 / _I24, each side on its own
	const uint8_t* in_host;
	int channels, mode;
	size_t n, piece;   // samples of the call and of a piece (the last piece may be shorter)
	uint8_t* hosts[3]; // harmonic, percussive, residual; NULL: not wanted, or not the pipeline's to write (HPRIOffline's residual)
	float gain, *peaks; // peaks: NULL, or where PEAK mode writes the three peaks
};

// Runs the job piece by piece: piece k+1 goes up and is widened on s_in, piece k runs on the engine's stream, piece k-1 is
// narrowed and comes down on s_out.  What the engines differ in comes as three calls into libzen_hip.so, each returning its
// code: bind(stream) puts the engine on the context's stream, in_end(b, e, &end) says how far the input must be up before
// piece [b, e) runs, engine(fin, b, e, out) runs it (fin: sample 0 of the call; out[o]: where sample b goes, or NULL).
template <class Bind, class InEnd, class Engine>
int run_pieces(void* h, int kind, const Job& j, Bind bind, InEnd in_end, Engine engine)
{
	const double t_start = now_ms();
	const size_t n = j.n, ch = (size_t)j.channels, n_pieces = ceil_div(n, j.piece);
	const size_t in_fb = (size_t)pcm_sample_bytes(j.in_fmt) * ch, out_sb = (size_t)pcm_sample_bytes(j.out_fmt); // bytes of an input frame, an output sample
	uint8_t* const* hosts = j.hosts;
	const bool peak_mode = j.mode == ZEN_HIP_PCM_PEAK;
	Ctx* c = nullptr;
	ZA_TRY(ctx_for(h, kind, &c));
	ZA_ZEN_AS(bind(c->run), "the engine's set_stream");
	ZA_TRY(grow(c, c->inb, c->inb_cap, n * in_fb));
	ZA_TRY(grow(c, c->fin, c->fin_cap, n));
	for (int o = 0; o < 3; ++o)
		if (hosts[o]) {
			ZA_TRY(grow(c, c->fout[o], c->fout_cap[o], n));
			ZA_TRY(grow(c, c->outb[o], c->outb_cap[o], n * out_sb));
		}
	// events: [k] piece k is up and widened, [n_pieces + k] piece k is through the engine (PEAK: and folded into min / max),
	// [2 n_pieces + k] PEAK: piece k is narrowed, [3 n_pieces] PEAK: the peaks are known
	ZA_TRY(need_events(c, 3 * n_pieces + 1));
	Registered reg_in, reg_out[3];
	reg_in.take(j.in_host, in_fb * n, true);
	for (int o = 0; o < 3; ++o)
		reg_out[o].take(hosts[o], out_sb * n, true);
	memset(&t_stats, 0, sizeof(t_stats));
	t_stats.n_pieces = n_pieces;
	t_stats.piece_frames = j.piece;
	t_stats.input_pinned = reg_in.pinned;
	t_stats.outputs_pinned = (!hosts[0] || reg_out[0].pinned) && (!hosts[1] || reg_out[1].pinned) && (!hosts[2] || reg_out[2].pinned);
	t_stats.setup_ms = now_ms() - t_start;
	auto span_of = [&](size_t k, size_t* b, size_t* e) {
		*b = k * j.piece;
		*e = *b + j.piece < n ? *b + j.piece : n;
	};
	size_t uploaded = 0;
	auto upload = [&](size_t k) -> int { // the samples piece k reads, beyond what is up already
		size_t b, e, end;
		span_of(k, &b, &e);
		ZA_ZEN_AS(in_end(b, e, &end), "the engine's range_halo");
		if (end > n)
			end = n;
		if (end > uploaded) {
			ZA_HIP(hipMemcpyAsync(c->inb + uploaded * in_fb, j.in_host + uploaded * in_fb, in_fb * (end - uploaded), hipMemcpyHostToDevice, c->s_in));
			ZA_HIP(zen_pcm::launch_unpack(j.in_fmt, c->inb + uploaded * in_fb, j.channels, end - uploaded, c->fin + uploaded, c->s_in));
			uploaded = end;
		}
		ZA_HIP(hipEventRecord(c->ev[k], c->s_in));
		return ZEN_HIP_OK;
	};
	auto download = [&](size_t k, hipStream_t narrow_on, hipEvent_t after) -> int { // narrow piece k behind `after`, bring it down
		size_t b, e;
		span_of(k, &b, &e);
		ZA_HIP(hipStreamWaitEvent(narrow_on, after, 0));
		for (int o = 0; o < 3; ++o)
			if (hosts[o])
				ZA_HIP(zen_pcm::launch_pack(j.out_fmt, c->fout[o] + b, e - b, j.mode, j.gain, c->minmax + 2 * o, c->outb[o] + b * out_sb, narrow_on));
		if (narrow_on != c->s_out) {
			ZA_HIP(hipEventRecord(c->ev[2 * n_pieces + k], narrow_on));
			ZA_HIP(hipStreamWaitEvent(c->s_out, c->ev[2 * n_pieces + k], 0));
		}
		for (int o = 0; o < 3; ++o)
			if (hosts[o])
				ZA_HIP(hipMemcpyAsync(hosts[o] + b * out_sb, c->outb[o] + b * out_sb, out_sb * (e - b), hipMemcpyDeviceToHost, c->s_out));
		return ZEN_HIP_OK;
	};
	bool tail_marked = false;
	auto feed = [&]() -> int {
		if (peak_mode)
			ZA_HIP(zen_pcm::launch_minmax_init(c->minmax, 3, c->run));
		ZA_TRY(upload(0));
		for (size_t k = 0; k < n_pieces; ++k) {
			size_t b, e;
			span_of(k, &b, &e);
			float* out[3];
			for (int o = 0; o < 3; ++o)
				out[o] = hosts[o] ? c->fout[o] + b : nullptr;
			ZA_HIP(hipStreamWaitEvent(c->run, c->ev[k], 0));
			ZA_ZEN_AS(engine(c->fin, b, e, out), "the engine's process call");
			if (peak_mode)
				for (int o = 0; o < 3; ++o)
					if (hosts[o])
						ZA_HIP(zen_pcm::launch_peak(out[o], e - b, c->minmax + 2 * o, c->run));
			ZA_HIP(hipEventRecord(c->ev[n_pieces + k], c->run));
			// (copies from / to memory that could not be pinned block this thread: piece k+1 goes up before piece k comes down,
			// so that the thread is never stuck behind kernels it has not fed yet)
			if (k + 1 < n_pieces)
				ZA_TRY(upload(k + 1));
			if (!peak_mode)
				ZA_TRY(download(k, c->s_out, c->ev[n_pieces + k]));
		}
		if (peak_mode) { // the peaks are known behind the last piece: narrow piece by piece on the engine's stream, each download under the next narrowing
			ZA_HIP(hipMemcpyAsync(c->minmax_host, c->minmax, 6 * sizeof(float), hipMemcpyDeviceToHost, c->run));
			ZA_HIP(hipEventRecord(c->ev[3 * n_pieces], c->run));
			tail_marked = true;
			for (size_t k = 0; k < n_pieces; ++k)
				ZA_TRY(download(k, c->run, c->ev[2 * n_pieces - 1]));
		}
		return ZEN_HIP_OK;
	};
	const int rc = feed();
	double t_tail = 0;
	if (tail_marked && hipEventSynchronize(c->ev[3 * n_pieces]) == hipSuccess)
		t_tail = now_ms();
	// nothing may be in flight when the caller's buffers are unregistered and handed back
	const int rc_sync = sync_all(c);
	ZA_TRY(rc);
	ZA_TRY(rc_sync);
	const double t_end = now_ms();
	if (peak_mode && j.peaks)
		for (int o = 0; o < 3; ++o)
			j.peaks[o] = hosts[o] ? pcm16_peak_of(c->minmax_host[2 * o], c->minmax_host[2 * o + 1]) : 0.f;
	t_stats.tail_ms = t_tail > 0 ? t_end - t_tail : 0;
	t_stats.total_ms = t_end - t_start;
	return ZEN_HIP_OK;
}

} // namespace

static_assert(ZEN_HIP_PCM_PEAK == ZEN_PCM_MODE_PEAK && ZEN_HIP_PCM_GAIN == ZEN_PCM_MODE_GAIN, "public and kernel-side mode values agree");
static_assert(ZEN_HIP_PCM_I16 == ZEN_PCM_FMT_I16 && ZEN_HIP_PCM_I24 == ZEN_PCM_FMT_I24, "public and kernel-side format values agree");

namespace {

// the bodies of the kernel entry points; `who`: the caller's name in the messages (the int16 calls keep theirs)
int unpack_dev(const char* who, int fmt, const void* src_dev, int channels, size_t n_frames, float* dst_dev, void* stream)
{
	ZA_TRY(check_fmt(who, "sample", fmt));
	if (channels != 1 && channels != 2)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: channels must be 1 or 2 (got %d)", who, channels);
	if (n_frames == 0)
		return ZEN_HIP_OK;
	if (!src_dev || !dst_dev)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	if ((fmt == ZEN_HIP_PCM_I16 && ((uintptr_t)src_dev & 1)) || ((uintptr_t)dst_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: int16_t pointers need 2-byte, float pointers 4-byte alignment", who);
	ZA_HIP(zen_pcm::launch_unpack(fmt, src_dev, channels, n_frames, dst_dev, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int pack_dev(const char* who, int fmt, const float* src_dev, size_t n, int mode, float gain, const float* minmax_dev, void* dst_dev, void* stream)
{
	ZA_TRY(check_fmt(who, "sample", fmt));
	if (mode != ZEN_HIP_PCM_PEAK && mode != ZEN_HIP_PCM_GAIN)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: mode must be ZEN_HIP_PCM_PEAK or ZEN_HIP_PCM_GAIN (got %d)", who, mode);
	if (n == 0)
		return ZEN_HIP_OK;
	if (!src_dev || !dst_dev || (mode == ZEN_HIP_PCM_PEAK && !minmax_dev))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	if (((uintptr_t)src_dev & 3) || (fmt == ZEN_HIP_PCM_I16 && ((uintptr_t)dst_dev & 1)) || ((uintptr_t)minmax_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: int16_t pointers need 2-byte, float pointers 4-byte alignment", who);
	ZA_HIP(zen_pcm::launch_pack(fmt, src_dev, n, mode, gain, minmax_dev, dst_dev, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int hpr_host(const char* who, zen_hip_hpr_t h, int in_fmt, const void* in_host, int channels, size_t n_hops, int out_fmt, void* harm, void* perc,
             void* resid, int mode, float gain, float peaks[3], size_t piece_hops);
int hpri_host(const char* who, zen_hip_hpri_t h, int in_fmt, const void* audio_host, int channels, size_t n_frames, int out_fmt, void* harm,
              void* perc, void* resid, int mode, float gain, float peaks[3], size_t range_samples);

} // namespace

extern "C" {

const char* zen_hip_pcm_last_error(void) { return t_err; }
const char* zen_hip_pcm_version(void) { return "zen_hip_pcm 1 (gfx950)"; }

size_t zen_hip_pcm_sample_bytes(int fmt) { return (size_t)pcm_sample_bytes(fmt); }

int zen_hip_pcm_to_float(const int16_t* src_dev, int channels, size_t n_frames, float* dst_dev, void* stream)
{
	return unpack_dev("pcm_to_float", ZEN_HIP_PCM_I16, src_dev, channels, n_frames, dst_dev, stream);
}

int zen_hip_pcm_unpack(int fmt, const void* src_dev, int channels, size_t n_frames, float* dst_dev, void* stream)
{
	return unpack_dev("pcm_unpack", fmt, src_dev, channels, n_frames, dst_dev, stream);
}

int zen_hip_pcm_peak(const float* src_dev, size_t n, float* minmax_dev, void* stream)
{
	if (n == 0)
		return ZEN_HIP_OK;
	if (!src_dev || !minmax_dev)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "pcm_peak: null argument");
	if (((uintptr_t)src_dev & 3) || ((uintptr_t)minmax_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "pcm_peak: float pointers need 4-byte alignment");
	ZA_HIP(zen_pcm::launch_peak(src_dev, n, minmax_dev, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_pcm_from_float(const float* src_dev, size_t n, int mode, float gain, const float* minmax_dev, int16_t* dst_dev,
                           void* stream)
{
	return pack_dev("pcm_from_float", ZEN_HIP_PCM_I16, src_dev, n, mode, gain, minmax_dev, dst_dev, stream);
}

int zen_hip_pcm_pack(int fmt, const float* src_dev, size_t n, int mode, float gain, const float* minmax_dev, void* dst_dev, void* stream)
{
	return pack_dev("pcm_pack", fmt, src_dev, n, mode, gain, minmax_dev, dst_dev, stream);
}

int zen_hip_pcm_host_stats_get(zen_hip_pcm_host_stats* out)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "pcm_host_stats_get: null argument");
	*out = t_stats;
	return ZEN_HIP_OK;
}

int zen_hip_pcm_release(void* engine_handle)
{
	Ctx* c = nullptr;
	{
		std::lock_guard<std::mutex> lk(g_mu);
		auto it = g_ctx.find(engine_handle);
		if (it == g_ctx.end())
			return ZEN_HIP_OK;
		c = it->second;
		g_ctx.erase(it);
	}
	int rc = ZEN_HIP_OK;
	if (c->run) { // the engine leaves the stream that is about to go (set_stream waits for it first)
		rc = c->kind == KIND_HPR ? zen_hip_hpr_set_stream((zen_hip_hpr_t)engine_handle, nullptr)
		                         : zen_hip_hpri_set_stream((zen_hip_hpri_t)engine_handle, nullptr);
		if (rc != ZEN_HIP_OK)
			set_err("pcm_release: %s", zen_hip_last_error());
	}
	free_ctx(c);
	return rc;
}

int zen_hip_pcm_release_all(void)
{
	std::unordered_map<void*, Ctx*> all;
	{
		std::lock_guard<std::mutex> lk(g_mu);
		all.swap(g_ctx);
	}
	for (auto& kv : all)
		free_ctx(kv.second);
	return ZEN_HIP_OK;
}

// ---- realtime block engine: pieces of hops, three outputs ------------------------------------------------------------------
int zen_hip_pcm_hpr_process_host(zen_hip_hpr_t h, const int16_t* in_host, int channels, size_t n_hops, int16_t* harm, int16_t* perc,
                                 int16_t* resid, int mode, float gain, float peaks[3], size_t piece_hops)
{
	return hpr_host("pcm_hpr_process_host", h, ZEN_HIP_PCM_I16, in_host, channels, n_hops, ZEN_HIP_PCM_I16, harm, perc, resid, mode, gain, peaks, piece_hops);
}

int zen_hip_pcm_hpr_process_host_fmt(zen_hip_hpr_t h, int in_fmt, const void* in_host, int channels, size_t n_hops, int out_fmt, void* harm,
                                     void* perc, void* resid, int mode, float gain, float peaks[3], size_t piece_hops)
{
	return hpr_host("pcm_hpr_process_host_fmt", h, in_fmt, in_host, channels, n_hops, out_fmt, harm, perc, resid, mode, gain, peaks, piece_hops);
}

int zen_hip_pcm_hpri_process(zen_hip_hpri_t h, const int16_t* audio_host, int channels, size_t n_frames, int16_t* harm, int16_t* perc,
                             int16_t* resid, int mode, float gain, float peaks[3], size_t range_samples)
{
	return hpri_host("pcm_hpri_process", h, ZEN_HIP_PCM_I16, audio_host, channels, n_frames, ZEN_HIP_PCM_I16, harm, perc, resid, mode, gain, peaks, range_samples);
}

int zen_hip_pcm_hpri_process_fmt(zen_hip_hpri_t h, int in_fmt, const void* audio_host, int channels, size_t n_frames, int out_fmt, void* harm,
                                 void* perc, void* resid, int mode, float gain, float peaks[3], size_t range_samples)
{
	return hpri_host("pcm_hpri_process_fmt", h, in_fmt, audio_host, channels, n_frames, out_fmt, harm, perc, resid, mode, gain, peaks, range_samples);
}

} // extern "C"

namespace {

int hpr_host(const char* who, zen_hip_hpr_t h, int in_fmt, const void* in_host, int channels, size_t n_hops, int out_fmt, void* harm, void* perc,
             void* resid, int mode, float gain, float peaks[3], size_t piece_hops)
{
	if (!h || !in_host)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	ZA_TRY(check_fmt(who, "input", in_fmt));
	ZA_TRY(check_fmt(who, "output", out_fmt));
	ZA_TRY(check_mode_channels(who, channels, mode));
	zen_hip_hpr_params P;
	ZA_ZEN(zen_hip_hpr_get_params(h, &P));
	if (P.n_streams != 1)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: one stream per engine (host blocks of several streams: one engine each)", who);
	if (n_hops == 0)
		return ZEN_HIP_OK;
	const size_t hop = P.hop, n = n_hops * hop, ch = (size_t)channels;
	const size_t in_sb = (size_t)pcm_sample_bytes(in_fmt), out_sb = (size_t)pcm_sample_bytes(out_fmt);
	{
		const Span s[4] = {{(const char*)in_host, in_sb * ch * n}, {(const char*)harm, out_sb * n}, {(const char*)perc, out_sb * n}, {(const char*)resid, out_sb * n}};
		if (any_overlap(s, 4))
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the host buffers must not overlap (pieces come down while later pieces go up)", who);
	}
	// default pieces: 4 Mi samples in GAIN mode -- 8 MiB on the link per piece and direction, the float path's rule in bytes --
	// and 8 Mi in PEAK mode, where nothing comes down inside the loop and the pieces only pace the uploads and the tail
	// (measured on the headline block, profiles/pcm16_piece_sweep.jsonl: GAIN 2.48 / 1.86 / 1.60 / 1.54 / 1.66 / 2.00 ms and
	// PEAK 4.22 / 3.32 / 2.84 / 2.49 / 2.39 / 2.37 ms at 0.5 / 1 / 2 / 4 / 8 / 12.6 Mi samples per piece)
	size_t piece = piece_hops ? piece_hops : ((size_t)(mode == ZEN_HIP_PCM_PEAK ? 8 : 4) << 20) / hop;
	piece = piece < 1 ? 1 : piece > n_hops ? n_hops : piece;
	const Job job = {in_fmt, out_fmt, (const uint8_t*)in_host, channels, mode, n, piece * hop, {(uint8_t*)harm, (uint8_t*)perc, (uint8_t*)resid}, gain, peaks};
	return run_pieces(
	    h, KIND_HPR, job, [&](hipStream_t run) { return zen_hip_hpr_set_stream(h, run); },
	    [](size_t, size_t e, size_t* end) { return *end = e, ZEN_HIP_OK; }, // a block reads no further than it writes
	    [&](const float* fin, size_t b, size_t e, float* const out[3]) { return zen_hip_hpr_process(h, fin + b, (e - b) / hop, e - b, out[0], out[1], out[2], e - b); });
}

// ---- offline two-pass engine: ranges of samples with their halos, two outputs and a zeroed residual -----------------------
int hpri_host(const char* who, zen_hip_hpri_t h, int in_fmt, const void* audio_host, int channels, size_t n_frames, int out_fmt, void* harm,
              void* perc, void* resid, int mode, float gain, float peaks[3], size_t range_samples)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	ZA_TRY(check_fmt(who, "input", in_fmt));
	ZA_TRY(check_fmt(who, "output", out_fmt));
	ZA_TRY(check_mode_channels(who, channels, mode));
	const size_t n = n_frames, ch = (size_t)channels;
	if (n == 0)
		return ZEN_HIP_OK; // the reference returns three empty vectors
	const size_t in_sb = (size_t)pcm_sample_bytes(in_fmt), out_sb = (size_t)pcm_sample_bytes(out_fmt);
	{
		const Span s[4] = {{(const char*)audio_host, in_sb * ch * n}, {(const char*)harm, out_sb * n}, {(const char*)perc, out_sb * n}, {(const char*)resid, out_sb * n}};
		if (any_overlap(s, 4))
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the host buffers must not overlap", who);
	}
	if (!audio_host)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	size_t a, b; // refusals of the engine (clip too short, a handle of several clips) before anything is touched
	ZA_ZEN(zen_hip_hpri_range_halo(h, n, 0, n, &a, &b));
	// ranges: the float path's rule (csrc/hpri.hip: shorter ranges cost more in warm-up halos and small grids than they hide in copies)
	size_t want = range_samples;
	if (want == 0) // 8 Mi samples from 32 Mi up, 4 Mi below, the whole clip below 8 Mi
		want = n >= ((size_t)1 << 25) ? (size_t)1 << 23 : n < ((size_t)1 << 23) ? n : (size_t)1 << 22;
	const size_t range = ceil_div(ceil_div(n, ceil_div(n, want)), 16384) * 16384;
	// the never-written residual: zeros, beside the pipeline.  Declared before the call that registers the caller's buffers, so
	// that on every path out they are unregistered (behind sync_all) first and the thread is joined last
	std::thread zero_thread;
	if (resid) {
		try {
			zero_thread = std::thread([=] { zero_host((uint8_t*)resid, n * out_sb); });
		}
		catch (...) { // no thread to be had: zeros written here, before the pipeline starts
			zero_host((uint8_t*)resid, n * out_sb);
		}
	}
	struct Joiner {
		std::thread& t;
		~Joiner()
		{
			if (t.joinable())
				t.join();
		}
	} joiner{zero_thread};
	const Job job = {in_fmt, out_fmt, (const uint8_t*)audio_host, channels, mode, n, range, {(uint8_t*)harm, (uint8_t*)perc, nullptr}, gain, peaks};
	return run_pieces(
	    h, KIND_HPRI, job, [&](hipStream_t run) { return zen_hip_hpri_set_stream(h, run); },
	    [&](size_t b, size_t e, size_t* end) { return zen_hip_hpri_range_halo(h, n, b, e, &b, end); }, // a range reads its halo
	    [&](const float* fin, size_t b, size_t e, float* const out[3]) { return zen_hip_hpri_process_range(h, fin, n, b, e, out[0], out[1]); });
}

} // namespace
