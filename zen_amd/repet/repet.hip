// repet.hip -- the C ABI of libzen_hip_repet.so (zen_hip_repet.h): REPET on clips in device memory.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as beat.hip is: the transforms are
// zen_hip_fft_exec_batched (one N-point handle for the frames, one handle per lag length 64..L of max_samples), memory comes
// from zen_hip_malloc, and the kernels of repet_kernels.hip stand between them.
//
// One call (n_clips clips of n samples, m frames each):
//   frame, fft, magnitude   every clip at once: the spectra X and the magnitudes V
//   per clip whose period is to be found: lag_rows, lag_fft (forward), power, lag_fft (inverse), braw;
//   then one copy of the beat spectra to the host, one wait, zen_hip_repet_find_period per clip
//   per clip: median -> S, mask (X in place), ifft, overlap_add -> the caller's rows
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "zen_hip_repet.h"

#include "../addon/stft_host.h"
#include "repet_kernels.h"

using namespace zen_addon;

namespace {

enum { K_FRAME = 0, K_FFT, K_MAG, K_LAG_ROWS, K_LAG_FFT, K_POWER, K_BRAW, K_MEDIAN, K_MASK, K_IFFT, K_OLA, K_COUNT };
static_assert(K_COUNT == ZEN_HIP_REPET_KERNELS, "the header names the kernels");
static_assert((int)zen_repet::MAX_SEGMENTS == ZEN_HIP_REPET_MAX_SEGMENTS && (int)zen_repet::REGISTER_SEGMENTS == ZEN_HIP_REPET_REGISTER_SEGMENTS,
              "the header states the kernels' limits");

constexpr size_t MIN_LAG = 64;

size_t lag_points(size_t m)
{
	size_t L = MIN_LAG;
	while (L < 2 * m)
		L *= 2;
	return L;
}

} // namespace

struct zen_hip_repet : Handle<K_COUNT> {
	float fs = 0.f;
	size_t N = 0, H = 0, bins = 0, v_stride = 0, C = 0, max_samples = 0, max_frames = 0, max_lag = 0;
	double tmin = 0.8, tmax = 8.0, highpass = 100.0;
	zen_hip_fft_t fft = nullptr;          // N points
	std::vector<zen_hip_fft_t> lag_fft;   // 64, 128, .., max_lag points
	float* rows = nullptr;      // C * max_frames rows of N complex values
	float* v = nullptr;         // C * max_frames rows of v_stride floats
	float* s = nullptr;         // max_frames rows of v_stride floats: the repeating segment of the clip at hand
	float* lag = nullptr;       // bins rows of max_lag complex values: the lag rows of the clip at hand
	float* braw = nullptr;      // C rows of max_frames floats
	float* tables = nullptr;    // the window (N), the divisor (H)
	float* stage_in = nullptr;  // the host calls' device rows: C rows of max_samples samples
	float* stage_out[2] = {nullptr, nullptr};
	std::vector<float> braw_host;   // C rows of max_frames floats
	std::vector<size_t> period;     // C
	unsigned long long calls = 0, clips = 0, searches = 0;
};

namespace {

zen_hip_fft_t lag_handle(const zen_hip_repet* h, size_t L)
{
	size_t i = 0;
	for (size_t l = MIN_LAG; l < L; l *= 2)
		++i;
	return h->lag_fft[i];
}

// steps 1-2 for every clip
int spectra(zen_hip_repet* h, const float* in, size_t in_stride, size_t n, size_t m)
{
	const FrameArgs a = {in, h->tables, h->rows, in_stride, n, m, h->C, (int)h->N};
	return zen_addon::spectra(h->prof, h->stream, h->fft, K_FRAME, K_FFT, K_MAG, zen_repet::launch_frame, zen_repet::launch_magnitude, a, h->v, h->v_stride);
}

// step 3 for clip c: braw_row receives m floats in device memory
int beat_spectrum(zen_hip_repet* h, size_t c, size_t m, float* braw_row)
{
	const size_t L = lag_points(m), bins = h->bins;
	const unsigned long long lag_bytes = sizeof(float) * 2 * bins * L;
	zen_hip_fft_t f = lag_handle(h, L);
	{
		zen_repet::LagArgs a = {h->v + c * m * h->v_stride, h->lag, h->v_stride, m, L, (int)bins};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_LAG_ROWS, sizeof(float) * m * bins + lag_bytes));
		ZA_HIP(zen_repet::launch_lag_rows(a, h->stream));
		ZA_TRY(kt.end());
	}
	for (int inverse = 0; inverse < 2; ++inverse) {
		{
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_LAG_FFT, 2 * lag_bytes));
			ZA_ZEN(zen_hip_fft_exec_batched(f, h->lag, bins, inverse, h->stream));
			ZA_TRY(kt.end());
		}
		if (inverse == 0) {
			zen_repet::PowerArgs a = {h->lag, bins * L};
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_POWER, 2 * lag_bytes));
			ZA_HIP(zen_repet::launch_power(a, h->stream));
			ZA_TRY(kt.end());
		}
	}
	{
		zen_repet::BrawArgs a = {h->lag, braw_row, m, L, (int)bins};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_BRAW, sizeof(float) * (2 * bins * m + m)));
		ZA_HIP(zen_repet::launch_braw(a, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

// steps 5-8 for clip c with period p (0: none)
int resynthesis(zen_hip_repet* h, size_t c, const float* in, size_t n, size_t m, size_t p, float* bg, float* fg)
{
	const size_t N = h->N, bins = h->bins;
	float* rows = h->rows + c * m * 2 * N;
	const float* v = h->v + c * m * h->v_stride;
	if (p) {
		{
			zen_repet::MedianArgs a = {v, h->s, h->v_stride, h->v_stride, m, bins, p};
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_MEDIAN, sizeof(float) * (m + p) * bins));
			ZA_HIP(zen_repet::launch_segment_median(a, h->stream));
			ZA_TRY(kt.end());
		}
		{
			double kc = h->highpass > 0 ? ceil(h->highpass * (double)N / (double)h->fs) : 0.0;
			if (!(kc < (double)(bins + 1)))
				kc = (double)(bins + 1);
			zen_repet::MaskArgs a = {rows, v, h->s, h->v_stride, m, p, (int)N, (int)kc};
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_MASK, sizeof(float) * m * (2 * bins + 4 * N)));
			ZA_HIP(zen_repet::launch_mask(a, h->stream));
			ZA_TRY(kt.end());
		}
		{
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_IFFT, sizeof(float) * m * 4 * N));
			ZA_ZEN(zen_hip_fft_exec_batched(h->fft, rows, m, 1, h->stream));
			ZA_TRY(kt.end());
		}
	}
	if (bg || fg) {
		zen_repet::OlaArgs a = {rows, in, h->tables + N, bg, fg, n, p, (int)N};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_OLA, sizeof(float) * n * ((p ? 3 : 1) + (bg != nullptr) + (fg != nullptr))));
		ZA_HIP(zen_repet::launch_overlap_add(a, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

int check_segments(const char* who, size_t c, size_t m, size_t p)
{
	const size_t r = (m + p - 1) / p;
	if (r < 2 || r > (size_t)ZEN_HIP_REPET_MAX_SEGMENTS)
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "%s: clip %zu: a period of %zu frames cuts its %zu frames into %zu segments, outside 2..%d", who, c, p, m, r,
		        (int)ZEN_HIP_REPET_MAX_SEGMENTS);
	return ZEN_HIP_OK;
}

int check_clips(const char* who, zen_hip_repet_t h, const void* in, size_t in_stride, size_t n)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (!in)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input", who);
	if ((uintptr_t)in & 3)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if (n == 0 || n > h->max_samples)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu samples per clip, the session takes 1..%zu", who, n, h->max_samples);
	if (in_stride < n)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: in_stride %zu below the %zu samples of a clip", who, in_stride, n);
	return ZEN_HIP_OK;
}

int check_separate(const char* who, zen_hip_repet_t h, const void* in, size_t in_stride, size_t n, const size_t* periods, const void* bg,
                   const void* fg, size_t out_stride, const void* braw, size_t braw_stride)
{
	ZA_TRY(check_clips(who, h, in, in_stride, n));
	if (((uintptr_t)bg & 3) || ((uintptr_t)fg & 3) || ((uintptr_t)braw & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if ((bg || fg) && out_stride < n)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu samples of a clip", who, out_stride, n);
	const size_t m = frames_of(n, h->H);
	if (braw && braw_stride < m)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: braw_stride %zu below the %zu frames of a clip", who, braw_stride, m);
	for (size_t c = 0; periods && c < h->C; ++c)
		if (periods[c])
			ZA_TRY(check_segments(who, c, m, periods[c]));
	return ZEN_HIP_OK;
}

void lag_range(const zen_hip_repet* h, size_t* jmin, size_t* jmax)
{
	const double per_frame = (double)h->fs / (double)h->H, cap = 1e15;
	const double lo = ceil(h->tmin * per_frame), hi = floor(h->tmax * per_frame);
	*jmin = lo < 2.0 ? 2 : lo > cap ? (size_t)cap : (size_t)lo;
	*jmax = hi < 0.0 ? 0 : hi > cap ? (size_t)cap : (size_t)hi;
}

// the arguments are checked; the outputs are device rows
int separate(const char* who, zen_hip_repet* h, const float* in, size_t in_stride, size_t n, const size_t* periods, float* bg, float* fg,
             size_t out_stride, size_t* periods_used, float* braw_out, size_t braw_stride)
{
	const size_t C = h->C, m = frames_of(n, h->H);
	ZA_TRY(spectra(h, in, in_stride, n, m));
	size_t searched = 0;
	for (size_t c = 0; c < C; ++c) {
		h->period[c] = periods ? periods[c] : 0;
		if (h->period[c] == 0) {
			ZA_TRY(beat_spectrum(h, c, m, h->braw + c * h->max_frames));
			++searched;
		}
	}
	if (searched) {
		ZA_HIP(hipMemcpyAsync(h->braw_host.data(), h->braw, sizeof(float) * C * h->max_frames, hipMemcpyDeviceToHost, h->stream));
		ZA_HIP(hipStreamSynchronize(h->stream));
		size_t jmin, jmax;
		lag_range(h, &jmin, &jmax);
		for (size_t c = 0; c < C; ++c) {
			if (periods && periods[c])
				continue;
			const float* row = h->braw_host.data() + c * h->max_frames;
			ZA_TRY(zen_hip_repet_find_period(row, m, jmin, jmax, &h->period[c], nullptr));
			if (h->period[c])
				ZA_TRY(check_segments(who, c, m, h->period[c]));
		}
		for (size_t c = 0; braw_out && c < C; ++c)
			if (!(periods && periods[c]))
				memcpy(braw_out + c * braw_stride, h->braw_host.data() + c * h->max_frames, sizeof(float) * m);
	}
	for (size_t c = 0; c < C; ++c)
		ZA_TRY(resynthesis(h, c, in + c * in_stride, n, m, h->period[c], bg ? bg + c * out_stride : nullptr, fg ? fg + c * out_stride : nullptr));
	for (size_t c = 0; periods_used && c < C; ++c)
		periods_used[c] = h->period[c];
	h->calls += 1;
	h->clips += C;
	h->searches += searched;
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host and device memory
int copy_rows(zen_hip_repet* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, hipMemcpyKind kind)
{
	return h->copy_rows(dst, dst_stride, src, src_stride, cnt, h->C, kind);
}

} // namespace

extern "C" {

const char* zen_hip_repet_last_error(void) { return t_err; }
const char* zen_hip_repet_version(void) { return "zen_hip_repet 1 (gfx950)"; }

int zen_hip_repet_create(float fs, size_t nfft, size_t n_clips, size_t max_samples, zen_hip_repet_t* out)
{
	if (!out || n_clips == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_create: null handle or zero clips");
	if (!frame_ok(nfft))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_create: frame %zu is not a power of two in 64..8192", nfft);
	if (!(fs > 0.0f) || !std::isfinite(fs))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_create: sample rate %g", (double)fs);
	const size_t H = nfft / 2;
	if (max_samples == 0 || max_samples > (size_t)ZEN_HIP_REPET_MAX_FRAMES * H || frames_of(max_samples, H) > (size_t)ZEN_HIP_REPET_MAX_FRAMES)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_create: max_samples %zu is not 1..%zu: a clip may have %d frames of %zu samples at the most", max_samples,
		        ((size_t)ZEN_HIP_REPET_MAX_FRAMES - 1) * H, (int)ZEN_HIP_REPET_MAX_FRAMES, H);
	if (n_clips > ((size_t)1 << 16))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_create: n_clips %zu above 2^16", n_clips);
	zen_hip_repet* h = new zen_hip_repet;
	h->fs = fs;
	h->N = nfft;
	h->H = H;
	h->bins = H + 1;
	h->v_stride = (h->bins + 3) & ~(size_t)3;
	h->C = n_clips;
	h->max_samples = max_samples;
	h->max_frames = frames_of(max_samples, H);
	h->max_lag = lag_points(h->max_frames);
	auto build = [&]() -> int {
		const size_t frames = n_clips * h->max_frames;
		const std::vector<float> tab = stft_tables(nfft);
		h->braw_host.assign(frames, 0.0f);
		h->period.assign(n_clips, 0);
		ZA_ZEN(zen_hip_fft_create(nfft, &h->fft));
		for (size_t L = MIN_LAG; L <= h->max_lag; L *= 2) {
			zen_hip_fft_t f = nullptr;
			ZA_ZEN(zen_hip_fft_create(L, &f));
			h->lag_fft.push_back(f);
		}
		ZA_TRY(h->alloc(&h->rows, frames * 2 * nfft));
		ZA_TRY(h->alloc(&h->v, frames * h->v_stride));
		ZA_TRY(h->alloc(&h->s, h->max_frames * h->v_stride));
		ZA_TRY(h->alloc(&h->lag, h->bins * 2 * h->max_lag));
		ZA_TRY(h->alloc(&h->braw, frames));
		ZA_TRY(h->alloc(&h->tables, tab.size()));
		ZA_TRY(h->alloc(&h->stage_in, n_clips * max_samples));
		for (float*& p : h->stage_out)
			ZA_TRY(h->alloc(&p, n_clips * max_samples));
		ZA_ZEN(zen_hip_memcpy_h2d(h->tables, tab.data(), sizeof(float) * tab.size()));
		// whatever the transforms allocate for their largest batches, up front: one run each on zeros
		ZA_HIP(hipMemsetAsync(h->rows, 0, sizeof(float) * frames * 2 * nfft, h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows, frames, 0, h->stream));
		ZA_HIP(hipMemsetAsync(h->lag, 0, sizeof(float) * h->bins * 2 * h->max_lag, h->stream));
		for (zen_hip_fft_t f : h->lag_fft)
			ZA_ZEN(zen_hip_fft_exec_batched(f, h->lag, h->bins, 0, h->stream));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_repet_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_repet_destroy(zen_hip_repet_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft);
	for (zen_hip_fft_t f : h->lag_fft)
		zen_hip_fft_destroy(f);
	h->release({h->rows, h->v, h->s, h->lag, h->braw, h->tables, h->stage_in, h->stage_out[0], h->stage_out[1]});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_repet_set_stream(zen_hip_repet_t h, void* stream) { return set_stream(h, stream, "repet"); }

int zen_hip_repet_set_params(zen_hip_repet_t h, double tmin_s, double tmax_s, double highpass_hz)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_set_params: null handle");
	if (!(tmin_s > 0.0) || !(tmax_s >= tmin_s) || !(highpass_hz >= 0.0) || !std::isfinite(tmax_s) || !std::isfinite(highpass_hz))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_set_params: periods of %g..%g s, high-pass %g Hz", tmin_s, tmax_s, highpass_hz);
	h->tmin = tmin_s;
	h->tmax = tmax_s;
	h->highpass = highpass_hz;
	return ZEN_HIP_OK;
}

int zen_hip_repet_separate_device(zen_hip_repet_t h, const float* in_dev, size_t in_stride, size_t n, const size_t* periods,
                                  float* background_dev, float* foreground_dev, size_t out_stride, size_t* periods_used, float* braw_host,
                                  size_t braw_stride)
{
	const char* who = "repet_separate_device";
	ZA_TRY(check_separate(who, h, in_dev, in_stride, n, periods, background_dev, foreground_dev, out_stride, braw_host, braw_stride));
	return separate(who, h, in_dev, in_stride, n, periods, background_dev, foreground_dev, out_stride, periods_used, braw_host, braw_stride);
}

int zen_hip_repet_separate_host(zen_hip_repet_t h, const float* in_host, size_t in_stride, size_t n, const size_t* periods,
                                float* background_host, float* foreground_host, size_t out_stride, size_t* periods_used, float* braw_host,
                                size_t braw_stride)
{
	const char* who = "repet_separate_host";
	ZA_TRY(check_separate(who, h, in_host, in_stride, n, periods, background_host, foreground_host, out_stride, braw_host, braw_stride));
	const size_t row = h->max_samples;
	float* host[2] = {background_host, foreground_host};
	int rc = copy_rows(h, h->stage_in, row, in_host, in_stride, n, hipMemcpyHostToDevice);
	if (rc == ZEN_HIP_OK)
		rc = separate(who, h, h->stage_in, row, n, periods, host[0] ? h->stage_out[0] : nullptr, host[1] ? h->stage_out[1] : nullptr, row,
		              periods_used, braw_host, braw_stride);
	for (int o = 0; o < 2 && rc == ZEN_HIP_OK; ++o)
		if (host[o])
			rc = copy_rows(h, host[o], out_stride, h->stage_out[o], row, n, hipMemcpyDeviceToHost);
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_repet_beat_spectrum_device(zen_hip_repet_t h, const float* in_dev, size_t in_stride, size_t n, float* braw_dev, size_t braw_stride)
{
	const char* who = "repet_beat_spectrum_device";
	ZA_TRY(check_clips(who, h, in_dev, in_stride, n));
	const size_t m = frames_of(n, h->H);
	if (!braw_dev || ((uintptr_t)braw_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned output", who);
	if (braw_stride < m)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: braw_stride %zu below the %zu frames of a clip", who, braw_stride, m);
	ZA_TRY(spectra(h, in_dev, in_stride, n, m));
	for (size_t c = 0; c < h->C; ++c)
		ZA_TRY(beat_spectrum(h, c, m, braw_dev + c * braw_stride));
	h->calls += 1;
	return ZEN_HIP_OK;
}

int zen_hip_repet_segment_median_device(const float* v_dev, size_t m, size_t bins, size_t v_stride, size_t period, float* s_dev, size_t s_stride,
                                        void* stream)
{
	const char* who = "repet_segment_median_device";
	if (!v_dev || !s_dev || ((uintptr_t)v_dev & 3) || ((uintptr_t)s_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned pointer", who);
	if (bins == 0 || bins > ((size_t)1 << 30) || v_stride < bins || s_stride < bins)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu bins in rows %zu and %zu floats apart", who, bins, v_stride, s_stride);
	if (period == 0 || m == 0)
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "%s: %zu frames at a period of %zu", who, m, period);
	ZA_TRY(check_segments(who, 0, m, period));
	if (period > 65535)
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "%s: a period of %zu frames, above 65535", who, period);
	zen_repet::MedianArgs a = {v_dev, s_dev, v_stride, s_stride, m, bins, period};
	ZA_HIP(zen_repet::launch_segment_median(a, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_repet_stats(zen_hip_repet_t h, zen_hip_repet_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_stats: null argument");
	out->calls = h->calls;
	out->clips = h->clips;
	out->searches = h->searches;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_repet_profile(zen_hip_repet_t h, int enable) { return profile(h, enable); }

int zen_hip_repet_profile_get(zen_hip_repet_t h, double ms[ZEN_HIP_REPET_KERNELS], unsigned long long bytes[ZEN_HIP_REPET_KERNELS],
                              unsigned long long launches[ZEN_HIP_REPET_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "repet");
}

int zen_hip_repet_find_period(const float* braw, size_t m, size_t jmin, size_t jmax, size_t* period, double* score)
{
	if (!period || (m && !braw))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_find_period: null argument");
	*period = 0;
	if (score)
		*score = 0.0;
	if (m == 0 || braw[0] == 0.0f || !std::isfinite(braw[0]))
		return ZEN_HIP_OK;
	std::vector<double> b(m);
	for (size_t j = 0; j < m; ++j)
		b[j] = (double)braw[j] / (double)braw[0];
	const auto first_max = [&b](size_t lo, size_t hi) {
		size_t h = lo;
		for (size_t i = lo + 1; i <= hi; ++i)
			if (b[i] > b[h])
				h = i;
		return h;
	};
	const size_t l = 3 * m / 4, last = jmax < l / 3 ? jmax : l / 3;
	size_t best = 0;
	double best_score = 0.0;
	for (size_t j = jmin < 2 ? 2 : jmin; j <= last; ++j) {
		const size_t delta = 3 * j / 4;
		double acc = 0.0;
		for (size_t i = j; i < l; i += j) {
			const size_t lo1 = i - 2 > 1 ? i - 2 : 1, hi1 = i + 2 < l - 1 ? i + 2 : l - 1; // j >= 2: i - 2 does not wrap
			const size_t lo = i - delta > 1 ? i - delta : 1, hi = i + delta < l - 1 ? i + delta : l - 1; // delta < j <= i
			const size_t h1 = first_max(lo1, hi1), h2 = first_max(lo, hi);
			if (h1 == h2) {
				double s = 0.0;
				for (size_t q = lo; q <= hi; ++q)
					s = s + b[q];
				acc = acc + (b[h1] - s / (double)(hi - lo + 1));
			}
		}
		const double J = acc / (double)(l / j);
		if (J > best_score) {
			best = j;
			best_score = J;
		}
	}
	*period = best;
	if (score)
		*score = best_score;
	return ZEN_HIP_OK;
}

int zen_hip_repet_table(size_t nfft, int which, float* out, size_t cap)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_table: null output");
	if (!frame_ok(nfft))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_table: frame %zu is not a power of two in 64..8192", nfft);
	if (which != ZEN_HIP_REPET_TABLE_WINDOW && which != ZEN_HIP_REPET_TABLE_DIVISOR)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_table: unknown table %d", which);
	const size_t len = which == ZEN_HIP_REPET_TABLE_WINDOW ? nfft : nfft / 2;
	if (cap < len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repet_table: room for %zu floats, the table has %zu", cap, len);
	for (size_t i = 0; i < len; ++i)
		out[i] = which == ZEN_HIP_REPET_TABLE_WINDOW ? window_at(i, nfft) : divisor_at(i, nfft);
	return ZEN_HIP_OK;
}

} // extern "C"
