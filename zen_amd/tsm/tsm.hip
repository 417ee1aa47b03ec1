// tsm.hip -- the C ABI of libzen_hip_tsm.so (zen_hip_tsm.h): time-scale modification of clips in device memory.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as repet.hip is: the transforms are
// zen_hip_fft_exec_batched (one N-point handle), memory comes from zen_hip_malloc, and the kernels of tsm_kernels.hip stand
// between them.
//
// One vocoder call (n_clips clips of n samples, M frames each), every step but one over all frames of all clips at once:
//   frame, fft, analysis    the spectra, their magnitudes and phases
//   peaks                   the owner of every bin and what the recurrence adds to it
//   walk                    the recurrence over the frames, one workgroup per clip
//   spectrum, ifft          the synthesis frames
//   overlap_add             the caller's rows; the overlap-add route of the other stems is a term of the same kernel
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>

#include "zen_hip_tsm.h"

#include "../addon/addon_host.h"
#include "tsm_kernels.h"

using namespace zen_addon;

namespace {

enum { K_FRAME = 0, K_FFT, K_ANALYSIS, K_PEAKS, K_WALK, K_SPECTRUM, K_IFFT, K_OLA, K_COUNT };
static_assert(K_COUNT == ZEN_HIP_TSM_KERNELS, "the header names the kernels");

constexpr double MIN_ALPHA = 0.25, MAX_ALPHA = 4.0;
constexpr int MAX_DEVICES = 64;

bool pv_frame_ok(size_t nfft) { return is_pow2(nfft) && nfft >= 64 && nfft <= 8192; }
bool ola_frame_ok(size_t nfft) { return is_pow2(nfft) && nfft >= 16 && nfft <= 4096; }
bool alpha_ok(double a) { return std::isfinite(a) && a >= MIN_ALPHA && a <= MAX_ALPHA; }

float window_at(size_t i, size_t N) { return (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)N)); }
float pv_divisor_at(size_t i, size_t N)
{
	double s = 0.0;
	for (size_t j = 0; j < 4; ++j) {
		const double w = (double)window_at(i + j * (N / 4), N);
		s += w * w;
	}
	return (float)((double)N * s);
}
float ola_divisor_at(size_t i, size_t N) { return (float)((double)window_at(i, N) + (double)window_at(i + N / 2, N)); }
void coarse_at(size_t a, float* cs)
{
	const double x = 2.0 * M_PI * (double)a / (double)zen_tsm::COARSE;
	cs[0] = (float)cos(x);
	cs[1] = (float)sin(x);
}
void fine_at(size_t b, float* cs)
{
	const double x = 2.0 * M_PI * (double)b / 4194304.0;
	cs[0] = (float)cos(x);
	cs[1] = (float)sin(x);
}
uint32_t atan_at(size_t i) { return (uint32_t)llround(atan((double)i / (double)zen_tsm::ATAN_STEPS) / (2.0 * M_PI) * 4294967296.0); }
float c3_const() { return (float)(1.0 / 3.0); }
float k_const() { return (float)(4294967296.0 / (2.0 * M_PI)); }

size_t samples_out(size_t n, double alpha) { return (size_t)floor((double)n * alpha); }
size_t frames_of(size_t n_out, size_t Hs, size_t V) { return (n_out - 1) / Hs + V; }
long long position_of(long long m, size_t Hs, size_t V, double alpha)
{
	return (long long)floor((double)((m - (long long)(V / 2) + 1) * (long long)Hs) / alpha);
}

// the code object's trigonometric tables, once per device
int ensure_tables()
{
	static std::mutex mu;
	static bool done[MAX_DEVICES] = {};
	int dev = 0;
	ZA_HIP(hipGetDevice(&dev));
	std::lock_guard<std::mutex> lock(mu);
	if (dev >= 0 && dev < MAX_DEVICES && done[dev])
		return ZEN_HIP_OK;
	std::vector<uint32_t> t(zen_tsm::ATAN_STEPS + 1);
	std::vector<float> a(2 * zen_tsm::COARSE), b(2 * zen_tsm::FINE);
	for (size_t i = 0; i < t.size(); ++i)
		t[i] = atan_at(i);
	for (size_t i = 0; i < (size_t)zen_tsm::COARSE; ++i)
		coarse_at(i, &a[2 * i]);
	for (size_t i = 0; i < (size_t)zen_tsm::FINE; ++i)
		fine_at(i, &b[2 * i]);
	ZA_HIP(zen_tsm::upload_tables(t.data(), a.data(), b.data(), c3_const(), k_const()));
	if (dev >= 0 && dev < MAX_DEVICES)
		done[dev] = true;
	return ZEN_HIP_OK;
}

} // namespace

struct zen_hip_tsm : Handle<K_COUNT> {
	float fs = 0.f;
	size_t N = 0, H = 0, bins = 0, stride = 0, Np = 0, C = 0, max_samples = 0, max_out = 0, max_frames = 0;
	double max_alpha = 0.0;
	zen_hip_fft_t fft = nullptr;
	float* rows = nullptr;      // C * max_frames rows of N complex values
	float* mag = nullptr;       // C * max_frames rows of stride floats
	uint32_t* theta = nullptr;  // the same shape, as e and psi
	uint32_t* e = nullptr;
	uint32_t* psi = nullptr;
	uint16_t* owner = nullptr;
	float* tables = nullptr;    // w (N), D (N / 4), wp (Np), d2 (Np / 2)
	float* stage_in[3] = {nullptr, nullptr, nullptr}; // the host call's device rows: C rows of max_samples samples each
	float* stage_out = nullptr;                       // C rows of max_out samples
	unsigned long long calls = 0, clips = 0;
};

namespace {

zen_tsm::Framing pv_framing(const zen_hip_tsm* h, double alpha) { return {alpha, (int)h->N, (int)(h->N / 4), 4}; }
zen_tsm::Framing ola_framing(const zen_hip_tsm* h, double alpha) { return {alpha, (int)h->Np, (int)(h->Np / 2), 2}; }

// steps 1-4 for every clip
int analyse(zen_hip_tsm* h, const float* in, size_t in_stride, size_t n, double alpha, size_t M)
{
	const size_t N = h->N, frames = h->C * M, S = h->stride;
	const zen_tsm::Framing fr = pv_framing(h, alpha);
	{
		zen_tsm::FrameArgs a = {in, h->tables, h->rows, in_stride, n, M, h->C, fr};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_FRAME, sizeof(float) * (h->C * n + frames * 2 * N)));
		ZA_HIP(zen_tsm::launch_frame(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_FFT, sizeof(float) * frames * 4 * N));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows, frames, 0, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_tsm::AnalysisArgs a = {h->rows, h->mag, h->theta, S, frames, (int)N};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_ANALYSIS, sizeof(float) * frames * (2 * h->bins + 2 * S)));
		ZA_HIP(zen_tsm::launch_analysis(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_tsm::PeakArgs a = {h->mag, h->theta, h->owner, h->e, S, M, frames, fr};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_PEAKS, frames * h->bins * (4 + 12 + 2 + 4)));
		ZA_HIP(zen_tsm::launch_peaks(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_tsm::WalkArgs a = {h->owner, h->e, h->psi, S, M, h->C, (int)h->bins};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_WALK, frames * h->bins * (2 + 4 + 4)));
		ZA_HIP(zen_tsm::launch_walk(a, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

// steps 5-6 up to the inverse transform
int synthesise(zen_hip_tsm* h, size_t M)
{
	const size_t N = h->N, frames = h->C * M;
	{
		zen_tsm::SpectrumArgs a = {h->rows, h->mag, h->psi, h->stride, frames, (int)N};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_SPECTRUM, sizeof(float) * frames * (2 * h->bins + 2 * N)));
		ZA_HIP(zen_tsm::launch_spectrum(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_IFFT, sizeof(float) * frames * 4 * N));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows, frames, 1, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

int check_call(const char* who, zen_hip_tsm_t h, const void* const* ins, int n_ins, size_t in_stride, size_t n, double alpha, const void* out,
               size_t out_stride, bool need_out)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	for (int i = 0; i < n_ins; ++i) {
		if (!ins[i])
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input", who);
		if ((uintptr_t)ins[i] & 3)
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	}
	if (need_out && !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null output", who);
	if ((uintptr_t)out & 3)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if (n == 0 || n > h->max_samples)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu samples per clip, the session takes 1..%zu", who, n, h->max_samples);
	if (in_stride < n)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: in_stride %zu below the %zu samples of a clip", who, in_stride, n);
	if (!alpha_ok(alpha))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a ratio of %g, outside 0.25..4", who, alpha);
	const size_t n_out = samples_out(n, alpha);
	if (n_out == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu samples at a ratio of %g leave no output sample", who, n, alpha);
	if (n_out > h->max_out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu output samples, the session was sized for %zu", who, n_out, h->max_out);
	if (need_out && out_stride < n_out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu output samples of a clip", who, out_stride, n_out);
	return ZEN_HIP_OK;
}

// the arguments are checked; harm and perc may each be NULL, not both
int stretch(zen_hip_tsm* h, const float* harm, const float* perc, const float* resid, size_t in_stride, size_t n, double alpha, float* out,
            size_t out_stride)
{
	const size_t n_out = samples_out(n, alpha), M = frames_of(n_out, h->N / 4, 4), N = h->N, Np = h->Np;
	if (harm) {
		ZA_TRY(analyse(h, harm, in_stride, n, alpha, M));
		ZA_TRY(synthesise(h, M));
	}
	const float* t = h->tables;
	zen_tsm::OutputArgs a = {harm ? h->rows : nullptr, t, t + N, M, (int)N, perc, resid, t + N + N / 4, t + N + N / 4 + Np, in_stride, n,
	                         ola_framing(h, alpha), out, out_stride, n_out, h->C};
	auto kt = h->prof.on_stream(h->stream);
	ZA_TRY(kt.begin(K_OLA, sizeof(float) * h->C * n_out * (1 + (harm ? 8 : 0) + (perc ? (resid ? 4 : 2) : 0))));
	ZA_HIP(zen_tsm::launch_output(a, h->stream));
	ZA_TRY(kt.end());
	h->calls += 1;
	h->clips += h->C;
	return ZEN_HIP_OK;
}

// inspect: `rows` rows of `cnt` words of `width` bytes from the handle's padded rows to the caller's packed ones, both in
// device memory, the pitches a frame's bins (16 KB at the most)
int pack_rows(zen_hip_tsm* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, size_t rows, size_t width)
{
	ZA_HIP(hipMemcpy2DAsync(dst, width * dst_stride, src, width * src_stride, width * cnt, rows, hipMemcpyDeviceToDevice, h->stream));
	return ZEN_HIP_OK;
}

} // namespace

extern "C" {

const char* zen_hip_tsm_last_error(void) { return t_err; }
const char* zen_hip_tsm_version(void) { return "zen_hip_tsm 1 (gfx950)"; }

int zen_hip_tsm_create(float fs, size_t nfft, size_t nfft_ola, size_t n_clips, size_t max_samples, double max_alpha, zen_hip_tsm_t* out)
{
	if (!out || n_clips == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_create: null handle or zero clips");
	if (!pv_frame_ok(nfft))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_create: frame %zu is not a power of two in 64..8192", nfft);
	if (!ola_frame_ok(nfft_ola))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_create: overlap-add frame %zu is not a power of two in 16..4096", nfft_ola);
	if (!(fs > 0.0f) || !std::isfinite(fs))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_create: sample rate %g", (double)fs);
	if (!alpha_ok(max_alpha))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_create: a largest ratio of %g, outside 0.25..4", max_alpha);
	if (n_clips > ((size_t)1 << 16))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_create: n_clips %zu above 2^16", n_clips);
	const size_t limit = (size_t)ZEN_HIP_TSM_MAX_FRAMES * 2048 * 4 + 4; // the output of a longer clip fits 16384 frames on no route, at no ratio
	const size_t max_out = max_samples == 0 || max_samples > limit ? 0 : samples_out(max_samples, max_alpha);
	if (max_samples == 0 || max_samples > limit || max_out == 0 || frames_of(max_out, nfft / 4, 4) > (size_t)ZEN_HIP_TSM_MAX_FRAMES ||
	    frames_of(max_out, nfft_ola / 2, 2) > (size_t)ZEN_HIP_TSM_MAX_FRAMES)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_create: max_samples %zu at a ratio of %g: an output may have 1 sample at the least and %d frames of %zu and of "
		                           "%zu samples at the most", max_samples, max_alpha, (int)ZEN_HIP_TSM_MAX_FRAMES, nfft / 4, nfft_ola / 2);
	zen_hip_tsm* h = new zen_hip_tsm;
	h->fs = fs;
	h->N = nfft;
	h->H = nfft / 2;
	h->bins = h->H + 1;
	h->stride = (h->bins + 3) & ~(size_t)3;
	h->Np = nfft_ola;
	h->C = n_clips;
	h->max_samples = max_samples;
	h->max_alpha = max_alpha;
	h->max_out = max_out;
	h->max_frames = frames_of(max_out, nfft / 4, 4);
	auto build = [&]() -> int {
		const size_t frames = n_clips * h->max_frames, S = h->stride;
		std::vector<float> tab(nfft + nfft / 4 + nfft_ola + nfft_ola / 2);
		float* t = tab.data();
		for (size_t i = 0; i < nfft; ++i)
			*t++ = window_at(i, nfft);
		for (size_t i = 0; i < nfft / 4; ++i)
			*t++ = pv_divisor_at(i, nfft);
		for (size_t i = 0; i < nfft_ola; ++i)
			*t++ = window_at(i, nfft_ola);
		for (size_t i = 0; i < nfft_ola / 2; ++i)
			*t++ = ola_divisor_at(i, nfft_ola);
		ZA_TRY(ensure_tables());
		ZA_ZEN(zen_hip_fft_create(nfft, &h->fft));
		ZA_TRY(h->alloc(&h->rows, frames * 2 * nfft));
		ZA_TRY(h->alloc(&h->mag, frames * S));
		ZA_TRY(h->alloc(&h->theta, frames * S));
		ZA_TRY(h->alloc(&h->e, frames * S));
		ZA_TRY(h->alloc(&h->psi, frames * S));
		ZA_TRY(h->alloc(&h->owner, frames * S));
		ZA_TRY(h->alloc(&h->tables, tab.size()));
		for (float*& p : h->stage_in)
			ZA_TRY(h->alloc(&p, n_clips * max_samples));
		ZA_TRY(h->alloc(&h->stage_out, n_clips * max_out));
		ZA_ZEN(zen_hip_memcpy_h2d(h->tables, tab.data(), sizeof(float) * tab.size()));
		// whatever the transform allocates for its largest batch, up front: one run on zeros
		ZA_HIP(hipMemsetAsync(h->rows, 0, sizeof(float) * frames * 2 * nfft, h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows, frames, 0, h->stream));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_tsm_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_tsm_destroy(zen_hip_tsm_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft);
	h->release({h->rows, h->mag, h->theta, h->e, h->psi, h->owner, h->tables, h->stage_in[0], h->stage_in[1], h->stage_in[2], h->stage_out});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_tsm_set_stream(zen_hip_tsm_t h, void* stream) { return set_stream(h, stream, "tsm"); }

int zen_hip_tsm_stretch_pv_device(zen_hip_tsm_t h, const float* in_dev, size_t in_stride, size_t n, double alpha, float* out_dev, size_t out_stride)
{
	const void* ins[] = {in_dev};
	ZA_TRY(check_call("tsm_stretch_pv_device", h, ins, 1, in_stride, n, alpha, out_dev, out_stride, true));
	return stretch(h, in_dev, nullptr, nullptr, in_stride, n, alpha, out_dev, out_stride);
}

int zen_hip_tsm_stretch_ola_device(zen_hip_tsm_t h, const float* perc_dev, const float* resid_dev, size_t in_stride, size_t n, double alpha,
                                   float* out_dev, size_t out_stride)
{
	const void* ins[] = {perc_dev, resid_dev};
	ZA_TRY(check_call("tsm_stretch_ola_device", h, ins, resid_dev ? 2 : 1, in_stride, n, alpha, out_dev, out_stride, true));
	return stretch(h, nullptr, perc_dev, resid_dev, in_stride, n, alpha, out_dev, out_stride);
}

int zen_hip_tsm_stretch_hp_device(zen_hip_tsm_t h, const float* harm_dev, const float* perc_dev, const float* resid_dev, size_t in_stride, size_t n,
                                  double alpha, float* out_dev, size_t out_stride)
{
	const void* ins[] = {harm_dev, perc_dev, resid_dev};
	ZA_TRY(check_call("tsm_stretch_hp_device", h, ins, resid_dev ? 3 : 2, in_stride, n, alpha, out_dev, out_stride, true));
	return stretch(h, harm_dev, perc_dev, resid_dev, in_stride, n, alpha, out_dev, out_stride);
}

int zen_hip_tsm_stretch_hp_host(zen_hip_tsm_t h, const float* harm_host, const float* perc_host, const float* resid_host, size_t in_stride, size_t n,
                                double alpha, float* out_host, size_t out_stride)
{
	const void* ins[] = {harm_host, perc_host, resid_host};
	ZA_TRY(check_call("tsm_stretch_hp_host", h, ins, resid_host ? 3 : 2, in_stride, n, alpha, out_host, out_stride, true));
	// the device rows lie tight, n and n_out words apart; the host rows are the caller's
	const size_t n_out = samples_out(n, alpha);
	int rc = ZEN_HIP_OK;
	for (int i = 0; i < (resid_host ? 3 : 2) && rc == ZEN_HIP_OK; ++i)
		rc = h->copy_rows_1d(h->stage_in[i], n, (const float*)ins[i], in_stride, n, h->C, hipMemcpyHostToDevice);
	if (rc == ZEN_HIP_OK)
		rc = stretch(h, h->stage_in[0], h->stage_in[1], resid_host ? h->stage_in[2] : nullptr, n, n, alpha, h->stage_out, n_out);
	if (rc == ZEN_HIP_OK)
		rc = h->copy_rows_1d(out_host, out_stride, h->stage_out, n_out, n_out, h->C, hipMemcpyDeviceToHost);
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_tsm_inspect_device(zen_hip_tsm_t h, const float* in_dev, size_t in_stride, size_t n, double alpha, float* mag_dev, unsigned* theta_dev,
                               unsigned short* owner_dev, unsigned* psi_dev)
{
	const char* who = "tsm_inspect_device";
	const void* ins[] = {in_dev};
	ZA_TRY(check_call(who, h, ins, 1, in_stride, n, alpha, nullptr, 0, false));
	if (((uintptr_t)mag_dev & 3) || ((uintptr_t)theta_dev & 3) || ((uintptr_t)psi_dev & 3) || ((uintptr_t)owner_dev & 1))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a misaligned output", who);
	const size_t M = frames_of(samples_out(n, alpha), h->N / 4, 4), frames = h->C * M;
	ZA_TRY(analyse(h, in_dev, in_stride, n, alpha, M));
	if (mag_dev)
		ZA_TRY(pack_rows(h, mag_dev, h->bins, h->mag, h->stride, h->bins, frames, sizeof(float)));
	if (theta_dev)
		ZA_TRY(pack_rows(h, theta_dev, h->bins, h->theta, h->stride, h->bins, frames, sizeof(uint32_t)));
	if (owner_dev)
		ZA_TRY(pack_rows(h, owner_dev, h->bins, h->owner, h->stride, h->bins, frames, sizeof(uint16_t)));
	if (psi_dev)
		ZA_TRY(pack_rows(h, psi_dev, h->bins, h->psi, h->stride, h->bins, frames, sizeof(uint32_t)));
	h->calls += 1;
	return ZEN_HIP_OK;
}

int zen_hip_tsm_phase_device(const float* re_im_dev, size_t count, unsigned* theta_dev, void* stream)
{
	if (!re_im_dev || !theta_dev || ((uintptr_t)re_im_dev & 3) || ((uintptr_t)theta_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_phase_device: null or misaligned pointer");
	if (count == 0)
		return ZEN_HIP_OK;
	ZA_TRY(ensure_tables());
	ZA_HIP(zen_tsm::launch_phase(re_im_dev, count, theta_dev, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_tsm_cs_device(const unsigned* psi_dev, size_t count, float* cos_sin_dev, void* stream)
{
	if (!psi_dev || !cos_sin_dev || ((uintptr_t)psi_dev & 3) || ((uintptr_t)cos_sin_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_cs_device: null or misaligned pointer");
	if (count == 0)
		return ZEN_HIP_OK;
	ZA_TRY(ensure_tables());
	ZA_HIP(zen_tsm::launch_cs(psi_dev, count, cos_sin_dev, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_tsm_stats(zen_hip_tsm_t h, zen_hip_tsm_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "tsm_stats: null argument");
	out->calls = h->calls;
	out->clips = h->clips;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_tsm_profile(zen_hip_tsm_t h, int enable) { return profile(h, enable); }

int zen_hip_tsm_profile_get(zen_hip_tsm_t h, double ms[ZEN_HIP_TSM_KERNELS], unsigned long long bytes[ZEN_HIP_TSM_KERNELS],
                            unsigned long long launches[ZEN_HIP_TSM_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "tsm");
}

int zen_hip_tsm_positions(size_t n, size_t frame, size_t overlap, double alpha, size_t* n_out, size_t* frames, long long* a_out, size_t cap)
{
	const char* who = "tsm_positions";
	if (!n_out || !frames)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	if (!is_pow2(frame) || frame < 16 || frame > 8192 || (overlap != 2 && overlap != 4))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a frame of %zu samples (a power of two in 16..8192) at an overlap of %zu (2 or 4)", who, frame, overlap);
	if (!alpha_ok(alpha))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a ratio of %g, outside 0.25..4", who, alpha);
	if (n == 0 || n > ((size_t)1 << 40))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu samples", who, n);
	const size_t Hs = frame / overlap, out = samples_out(n, alpha);
	if (out == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu samples at a ratio of %g leave no output sample", who, n, alpha);
	const size_t M = frames_of(out, Hs, overlap);
	if (a_out && cap < M)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: room for %zu positions, the clip has %zu frames", who, cap, M);
	*n_out = out;
	*frames = M;
	for (size_t m = 0; a_out && m < M; ++m)
		a_out[m] = position_of((long long)m, Hs, overlap, alpha);
	return ZEN_HIP_OK;
}

int zen_hip_tsm_table(size_t nfft, int which, void* out, size_t cap)
{
	const char* who = "tsm_table";
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null output", who);
	size_t len = 0;
	bool frame_ok = true;
	switch (which) {
	case ZEN_HIP_TSM_TABLE_WINDOW:
		frame_ok = is_pow2(nfft) && nfft >= 16 && nfft <= 8192;
		len = nfft;
		break;
	case ZEN_HIP_TSM_TABLE_PV_DIVISOR:
		frame_ok = pv_frame_ok(nfft);
		len = nfft / 4;
		break;
	case ZEN_HIP_TSM_TABLE_OLA_DIVISOR:
		frame_ok = ola_frame_ok(nfft);
		len = nfft / 2;
		break;
	case ZEN_HIP_TSM_TABLE_COARSE:
		len = 2 * (size_t)zen_tsm::COARSE;
		break;
	case ZEN_HIP_TSM_TABLE_FINE:
		len = 2 * (size_t)zen_tsm::FINE;
		break;
	case ZEN_HIP_TSM_TABLE_ATAN:
		len = (size_t)zen_tsm::ATAN_STEPS + 1;
		break;
	case ZEN_HIP_TSM_TABLE_CONSTANTS:
		len = 2;
		break;
	default:
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: unknown table %d", who, which);
	}
	if (!frame_ok)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: frame %zu is outside the range of table %d", who, nfft, which);
	if (cap < len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: room for %zu words, the table has %zu", who, cap, len);
	float* f = (float*)out;
	uint32_t* u = (uint32_t*)out;
	for (size_t i = 0; i < len; ++i) {
		switch (which) {
		case ZEN_HIP_TSM_TABLE_WINDOW:
			f[i] = window_at(i, nfft);
			break;
		case ZEN_HIP_TSM_TABLE_PV_DIVISOR:
			f[i] = pv_divisor_at(i, nfft);
			break;
		case ZEN_HIP_TSM_TABLE_OLA_DIVISOR:
			f[i] = ola_divisor_at(i, nfft);
			break;
		case ZEN_HIP_TSM_TABLE_COARSE:
			if (i % 2 == 0)
				coarse_at(i / 2, f + i);
			break;
		case ZEN_HIP_TSM_TABLE_FINE:
			if (i % 2 == 0)
				fine_at(i / 2, f + i);
			break;
		case ZEN_HIP_TSM_TABLE_ATAN:
			u[i] = atan_at(i);
			break;
		default:
			f[i] = i == 0 ? c3_const() : k_const();
		}
	}
	return ZEN_HIP_OK;
}

} // extern "C"
