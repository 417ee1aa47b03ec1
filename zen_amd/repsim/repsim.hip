// repsim.hip -- the C ABI of libzen_hip_repsim.so (zen_hip_repsim.h): REPET-SIM on clips in device memory.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as repet.hip is: the transforms are
// zen_hip_fft_exec_batched (one N-point handle), memory comes from zen_hip_malloc, and the kernels of repsim_kernels.hip
// stand between them.
//
// One call (n_clips clips of n samples, m frames each):
//   frame, fft, magnitude   every clip at once: the spectra X and the magnitudes V
//   per clip, a band of rows at a time: similarity -> the band of S, select -> idx and counts of the band's frames
//   per clip: gather_median -> U, mask (X in place), ifft, overlap_add -> the caller's rows
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "zen_hip_repsim.h"

#include "../addon/stft_host.h"
#include "repsim_kernels.h"

using namespace zen_addon;

namespace {

enum { K_FRAME = 0, K_FFT, K_MAG, K_SIM_MFMA, K_SIM_VALU, K_SELECT, K_MEDIAN, K_MASK, K_IFFT, K_OLA, K_COUNT };
static_assert(K_COUNT == ZEN_HIP_REPSIM_KERNELS, "the header names the kernels");
static_assert((int)zen_repsim::MAX_NEIGHBOURS == ZEN_HIP_REPSIM_MAX_NEIGHBOURS && (int)zen_repsim::REGISTER_NEIGHBOURS == ZEN_HIP_REPSIM_REGISTER_NEIGHBOURS &&
                  (int)zen_repsim::MAX_FRAMES == ZEN_HIP_REPSIM_MAX_FRAMES,
              "the header states the kernels' limits");

constexpr size_t KMAX = ZEN_HIP_REPSIM_MAX_NEIGHBOURS, TILE = zen_repsim::SIM_TILE;
// The route of ZEN_HIP_REPSIM_ROUTE_DEFAULT.
constexpr bool DEFAULT_MFMA = true;

size_t round_up(size_t v, size_t q) { return (v + q - 1) / q * q; }

} // namespace

struct zen_hip_repsim : Handle<K_COUNT> {
	float fs = 0.f;
	size_t N = 0, H = 0, bins = 0, v_stride = 0, C = 0, max_samples = 0, max_frames = 0, band = 0, s_stride = 0;
	double threshold = 0.0, distance = 1.0, highpass = 100.0;
	size_t number = 100;
	bool mfma = DEFAULT_MFMA;
	zen_hip_fft_t fft = nullptr; // N points
	float* rows = nullptr;      // C * max_frames rows of N complex values
	float* v = nullptr;         // C * max_frames rows of v_stride floats
	float* u = nullptr;         // max_frames rows of v_stride floats: the repeating spectrogram of the clip at hand
	float* sband = nullptr;     // band rows of s_stride floats: the rows of S at hand
	int* idx = nullptr;         // C * max_frames rows of up to 256 (a call packs them k apart)
	int* counts = nullptr;      // C * max_frames
	float* tables = nullptr;    // the window (N), the divisor (H)
	float* stage_in = nullptr;  // the host calls' device rows: C rows of max_samples samples
	float* stage_out[2] = {nullptr, nullptr};
	unsigned long long calls = 0, clips = 0, bands = 0;
};

namespace {

// steps 1-2 for every clip
int spectra(zen_hip_repsim* h, const float* in, size_t in_stride, size_t n, size_t m)
{
	const FrameArgs a = {in, h->tables, h->rows, in_stride, n, m, h->C, (int)h->N};
	return zen_addon::spectra(h->prof, h->stream, h->fft, K_FRAME, K_FFT, K_MAG, zen_repsim::launch_frame, zen_repsim::launch_magnitude, a, h->v,
	                          h->v_stride);
}

size_t distance_frames(const zen_hip_repsim* h, size_t m)
{
	const double d = ceil(h->distance * (double)h->fs / (double)h->H);
	return d < 1.0 ? 1 : d > (double)m ? m : (size_t)d;
}

// steps 3-4 for clip c: idx and counts of its m frames, a band of rows of S at a time
int neighbours(zen_hip_repsim* h, size_t c, size_t m, int* idx, int* counts)
{
	const float* v = h->v + c * m * h->v_stride;
	const size_t k = h->number, dd = distance_frames(h, m);
	for (size_t a0 = 0; a0 < m; a0 += h->band) {
		const size_t rows = m - a0 < h->band ? m - a0 : h->band;
		{
			zen_repsim::SimArgs a = {v + a0 * h->v_stride, v, h->sband, h->v_stride, h->s_stride, rows, m, h->bins};
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(h->mfma ? K_SIM_MFMA : K_SIM_VALU, sizeof(float) * (m * h->bins + rows * m)));
			ZA_HIP(zen_repsim::launch_similarity(a, h->mfma, h->stream));
			ZA_TRY(kt.end());
		}
		{
			zen_repsim::SelectArgs a = {h->sband, idx + a0 * k, counts + a0, h->s_stride, rows, m, (float)h->threshold, (int)dd, (int)k};
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_SELECT, sizeof(float) * rows * (m + k + 1)));
			ZA_HIP(zen_repsim::launch_select(a, h->stream));
			ZA_TRY(kt.end());
		}
		h->bands += 1;
	}
	return ZEN_HIP_OK;
}

// steps 5-7 for clip c
int resynthesis(zen_hip_repsim* h, size_t c, const float* in, size_t n, size_t m, const int* idx, const int* counts, float* bg, float* fg)
{
	const size_t N = h->N, bins = h->bins;
	float* rows = h->rows + c * m * 2 * N;
	const float* v = h->v + c * m * h->v_stride;
	if (!bg && !fg)
		return ZEN_HIP_OK;
	{
		zen_repsim::GatherArgs a = {v, idx, counts, h->u, h->v_stride, h->v_stride, m, m, bins, (int)h->number};
		auto kt = h->prof.on_stream(h->stream);
		// what the kernel moves if every frame has its k neighbours; V itself is far smaller and is read out of the cache
		ZA_TRY(kt.begin(K_MEDIAN, sizeof(float) * m * (bins * (h->number + 1) + h->number + 1)));
		ZA_HIP(zen_repsim::launch_gather_median(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		double kc = h->highpass > 0 ? ceil(h->highpass * (double)N / (double)h->fs) : 0.0;
		if (!(kc < (double)(bins + 1)))
			kc = (double)(bins + 1);
		zen_repsim::MaskArgs a = {rows, v, h->u, h->v_stride, m, (int)N, (int)kc};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_MASK, sizeof(float) * m * (2 * bins + 4 * N)));
		ZA_HIP(zen_repsim::launch_mask(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_IFFT, sizeof(float) * m * 4 * N));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, rows, m, 1, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_repsim::OlaArgs a = {rows, in, h->tables + N, bg, fg, n, (int)N};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_OLA, sizeof(float) * n * (3 + (bg != nullptr) + (fg != nullptr))));
		ZA_HIP(zen_repsim::launch_overlap_add(a, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

int check_separate(const char* who, zen_hip_repsim_t h, const void* in, size_t in_stride, size_t n, const void* bg, const void* fg, size_t out_stride,
                   const void* counts, const void* indices)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (!in)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input", who);
	if (misaligned(in) || misaligned(bg) || misaligned(fg) || misaligned(counts) || misaligned(indices))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float and int32 pointers need 4-byte alignment", who);
	if (n == 0 || n > h->max_samples)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu samples per clip, the session takes 1..%zu", who, n, h->max_samples);
	if (in_stride < n)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: in_stride %zu below the %zu samples of a clip", who, in_stride, n);
	if ((bg || fg) && out_stride < n)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu samples of a clip", who, out_stride, n);
	return ZEN_HIP_OK;
}

// the arguments are checked; the outputs are device rows.  idx and counts of the call stay in the handle, packed k apart.
int separate(zen_hip_repsim* h, const float* in, size_t in_stride, size_t n, float* bg, float* fg, size_t out_stride)
{
	const size_t C = h->C, m = frames_of(n, h->H), k = h->number;
	ZA_TRY(spectra(h, in, in_stride, n, m));
	for (size_t c = 0; c < C; ++c) {
		int* idx = h->idx + c * m * k;
		int* counts = h->counts + c * m;
		ZA_TRY(neighbours(h, c, m, idx, counts));
		ZA_TRY(resynthesis(h, c, in + c * in_stride, n, m, idx, counts, bg ? bg + c * out_stride : nullptr, fg ? fg + c * out_stride : nullptr));
	}
	h->calls += 1;
	h->clips += C;
	return ZEN_HIP_OK;
}

int copy_selection(zen_hip_repsim* h, size_t n, int* counts, int* indices, hipMemcpyKind kind)
{
	const size_t frames = h->C * frames_of(n, h->H);
	if (counts)
		ZA_HIP(hipMemcpyAsync(counts, h->counts, sizeof(int) * frames, kind, h->stream));
	if (indices)
		ZA_HIP(hipMemcpyAsync(indices, h->idx, sizeof(int) * frames * h->number, kind, h->stream));
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host and device memory
int copy_rows(zen_hip_repsim* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, hipMemcpyKind kind)
{
	return h->copy_rows(dst, dst_stride, src, src_stride, cnt, h->C, kind);
}

int check_matrix(const char* who, const void* p, const void* q, size_t m)
{
	if (!p || !q || misaligned(p) || misaligned(q))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned pointer", who);
	if (m == 0 || m > (size_t)ZEN_HIP_REPSIM_MAX_FRAMES)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu frames, outside 1..%d", who, m, (int)ZEN_HIP_REPSIM_MAX_FRAMES);
	return ZEN_HIP_OK;
}

} // namespace

extern "C" {

const char* zen_hip_repsim_last_error(void) { return t_err; }
const char* zen_hip_repsim_version(void) { return "zen_hip_repsim 1 (gfx950)"; }

int zen_hip_repsim_create(float fs, size_t nfft, size_t n_clips, size_t max_samples, zen_hip_repsim_t* out)
{
	if (!out || n_clips == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_create: null handle or zero clips");
	if (!frame_ok(nfft))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_create: frame %zu is not a power of two in 64..8192", nfft);
	if (!(fs > 0.0f) || !std::isfinite(fs))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_create: sample rate %g", (double)fs);
	const size_t H = nfft / 2;
	if (max_samples == 0 || max_samples > (size_t)ZEN_HIP_REPSIM_MAX_FRAMES * H || frames_of(max_samples, H) > (size_t)ZEN_HIP_REPSIM_MAX_FRAMES)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_create: max_samples %zu is not 1..%zu: a clip may have %d frames of %zu samples at the most", max_samples,
		        ((size_t)ZEN_HIP_REPSIM_MAX_FRAMES - 1) * H, (int)ZEN_HIP_REPSIM_MAX_FRAMES, H);
	if (n_clips > ((size_t)1 << 16))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_create: n_clips %zu above 2^16", n_clips);
	zen_hip_repsim* h = new zen_hip_repsim;
	h->fs = fs;
	h->N = nfft;
	h->H = H;
	h->bins = H + 1;
	h->v_stride = (h->bins + 3) & ~(size_t)3;
	h->C = n_clips;
	h->max_samples = max_samples;
	h->max_frames = frames_of(max_samples, H);
	h->s_stride = round_up(h->max_frames, 4);
	const size_t fit = ZEN_HIP_REPSIM_BAND_BYTES / (sizeof(float) * h->s_stride) / TILE * TILE, all = round_up(h->max_frames, TILE);
	h->band = fit < TILE ? TILE : fit;
	if (h->band > all)
		h->band = all;
	const char* env = getenv("ZEN_HIP_REPSIM");
	if (env && strstr(env, "mfma=0"))
		h->mfma = false;
	else if (env && strstr(env, "mfma=1"))
		h->mfma = true;
	if (const char* b = env ? strstr(env, "band=") : nullptr) { // fewer rows per band than the scratch would hold
		const size_t rows = round_up((size_t)strtoull(b + 5, nullptr, 10), TILE);
		if (rows >= TILE && rows < h->band)
			h->band = rows;
	}
	auto build = [&]() -> int {
		const size_t frames = n_clips * h->max_frames;
		const std::vector<float> tab = stft_tables(nfft);
		ZA_ZEN(zen_hip_fft_create(nfft, &h->fft));
		ZA_TRY(h->alloc(&h->rows, frames * 2 * nfft));
		ZA_TRY(h->alloc(&h->v, frames * h->v_stride));
		ZA_TRY(h->alloc(&h->u, h->max_frames * h->v_stride));
		ZA_TRY(h->alloc(&h->sband, h->band * h->s_stride));
		ZA_TRY(h->alloc(&h->idx, frames * KMAX));
		ZA_TRY(h->alloc(&h->counts, frames));
		ZA_TRY(h->alloc(&h->tables, tab.size()));
		ZA_TRY(h->alloc(&h->stage_in, n_clips * max_samples));
		for (float*& p : h->stage_out)
			ZA_TRY(h->alloc(&p, n_clips * max_samples));
		ZA_ZEN(zen_hip_memcpy_h2d(h->tables, tab.data(), sizeof(float) * tab.size()));
		// whatever the transform allocates for its largest batch, up front: one run on zeros
		ZA_HIP(hipMemsetAsync(h->rows, 0, sizeof(float) * frames * 2 * nfft, h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows, frames, 0, h->stream));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_repsim_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_repsim_destroy(zen_hip_repsim_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft);
	h->release({h->rows, h->v, h->u, h->sband, h->idx, h->counts, h->tables, h->stage_in, h->stage_out[0], h->stage_out[1]});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_repsim_set_stream(zen_hip_repsim_t h, void* stream) { return set_stream(h, stream, "repsim"); }

int zen_hip_repsim_set_params(zen_hip_repsim_t h, double threshold, double distance_s, size_t number, double highpass_hz)
{
	if (!(threshold >= 0.0) || !(threshold < 1.0) || !(distance_s >= 0.0) || !std::isfinite(distance_s) || !(highpass_hz >= 0.0) ||
	    !std::isfinite(highpass_hz) || number < 1 || number > KMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_set_params: threshold %g outside [0, 1), distance %g s, %zu frames outside 1..%zu or high-pass %g Hz",
		        threshold, distance_s, number, KMAX, highpass_hz);
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_set_params: null handle");
	h->threshold = threshold;
	h->distance = distance_s;
	h->number = number;
	h->highpass = highpass_hz;
	return ZEN_HIP_OK;
}

int zen_hip_repsim_separate_device(zen_hip_repsim_t h, const float* in_dev, size_t in_stride, size_t n, float* background_dev,
                                   float* foreground_dev, size_t out_stride, int* counts_dev, int* indices_dev)
{
	ZA_TRY(check_separate("repsim_separate_device", h, in_dev, in_stride, n, background_dev, foreground_dev, out_stride, counts_dev, indices_dev));
	ZA_TRY(separate(h, in_dev, in_stride, n, background_dev, foreground_dev, out_stride));
	return copy_selection(h, n, counts_dev, indices_dev, hipMemcpyDeviceToDevice);
}

int zen_hip_repsim_separate_host(zen_hip_repsim_t h, const float* in_host, size_t in_stride, size_t n, float* background_host,
                                 float* foreground_host, size_t out_stride, int* counts_host, int* indices_host)
{
	ZA_TRY(check_separate("repsim_separate_host", h, in_host, in_stride, n, background_host, foreground_host, out_stride, counts_host, indices_host));
	const size_t row = h->max_samples;
	float* host[2] = {background_host, foreground_host};
	int rc = copy_rows(h, h->stage_in, row, in_host, in_stride, n, hipMemcpyHostToDevice);
	if (rc == ZEN_HIP_OK)
		rc = separate(h, h->stage_in, row, n, host[0] ? h->stage_out[0] : nullptr, host[1] ? h->stage_out[1] : nullptr, row);
	for (int o = 0; o < 2 && rc == ZEN_HIP_OK; ++o)
		if (host[o])
			rc = copy_rows(h, host[o], out_stride, h->stage_out[o], row, n, hipMemcpyDeviceToHost);
	if (rc == ZEN_HIP_OK)
		rc = copy_selection(h, n, counts_host, indices_host, hipMemcpyDeviceToHost);
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_repsim_similarity_device(const float* v_dev, size_t m, size_t bins, size_t v_stride, float* s_dev, size_t s_stride, int route,
                                     void* stream)
{
	const char* who = "repsim_similarity_device";
	ZA_TRY(check_matrix(who, v_dev, s_dev, m));
	if (bins == 0 || bins > ((size_t)1 << 30) || v_stride < bins || s_stride < m)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu bins in rows %zu floats apart, %zu frames in rows %zu floats apart", who, bins, v_stride, m, s_stride);
	if (route != ZEN_HIP_REPSIM_ROUTE_DEFAULT && route != ZEN_HIP_REPSIM_ROUTE_MFMA && route != ZEN_HIP_REPSIM_ROUTE_VALU)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: unknown route %d", who, route);
	const bool mfma = route == ZEN_HIP_REPSIM_ROUTE_DEFAULT ? DEFAULT_MFMA : route == ZEN_HIP_REPSIM_ROUTE_MFMA;
	zen_repsim::SimArgs a = {v_dev, v_dev, s_dev, v_stride, s_stride, m, m, bins};
	ZA_HIP(zen_repsim::launch_similarity(a, mfma, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_repsim_select_device(const float* s_dev, size_t m, size_t s_stride, float threshold, size_t distance, size_t number, int* idx_dev,
                                 int* counts_dev, void* stream)
{
	const char* who = "repsim_select_device";
	ZA_TRY(check_matrix(who, s_dev, idx_dev, m));
	if (!counts_dev || misaligned(counts_dev))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned pointer", who);
	if (s_stride < m)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu frames in rows %zu floats apart", who, m, s_stride);
	if (threshold != threshold || distance < 1 || number < 1 || number > KMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: threshold %g, a distance of %zu frames, %zu frames outside 1..%zu", who, (double)threshold, distance, number, KMAX);
	zen_repsim::SelectArgs a = {s_dev, idx_dev, counts_dev, s_stride, m, m, threshold, (int)(distance > m ? m : distance), (int)number};
	ZA_HIP(zen_repsim::launch_select(a, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_repsim_gather_median_device(const float* v_dev, size_t m, size_t bins, size_t v_stride, const int* idx_dev, const int* counts_dev,
                                        size_t rows, size_t number, float* u_dev, size_t u_stride, void* stream)
{
	const char* who = "repsim_gather_median_device";
	ZA_TRY(check_matrix(who, v_dev, u_dev, m));
	if (!idx_dev || !counts_dev || misaligned(idx_dev) || misaligned(counts_dev))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned pointer", who);
	if (bins == 0 || bins > ((size_t)1 << 30) || v_stride < bins || u_stride < bins)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu bins in rows %zu and %zu floats apart", who, bins, v_stride, u_stride);
	if (rows < 1 || rows > (size_t)ZEN_HIP_REPSIM_MAX_FRAMES || number < 1 || number > KMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu rows outside 1..%d or %zu frames outside 1..%zu", who, rows, (int)ZEN_HIP_REPSIM_MAX_FRAMES, number, KMAX);
	zen_repsim::GatherArgs a = {v_dev, idx_dev, counts_dev, u_dev, v_stride, u_stride, m, rows, bins, (int)number};
	ZA_HIP(zen_repsim::launch_gather_median(a, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_repsim_stats(zen_hip_repsim_t h, zen_hip_repsim_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_stats: null argument");
	out->calls = h->calls;
	out->clips = h->clips;
	out->bands = h->bands;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_repsim_profile(zen_hip_repsim_t h, int enable) { return profile(h, enable); }

int zen_hip_repsim_profile_get(zen_hip_repsim_t h, double ms[ZEN_HIP_REPSIM_KERNELS], unsigned long long bytes[ZEN_HIP_REPSIM_KERNELS],
                               unsigned long long launches[ZEN_HIP_REPSIM_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "repsim");
}

int zen_hip_repsim_table(size_t nfft, int which, float* out, size_t cap)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_table: null output");
	if (!frame_ok(nfft))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_table: frame %zu is not a power of two in 64..8192", nfft);
	if (which != ZEN_HIP_REPSIM_TABLE_WINDOW && which != ZEN_HIP_REPSIM_TABLE_DIVISOR)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_table: unknown table %d", which);
	const size_t len = which == ZEN_HIP_REPSIM_TABLE_WINDOW ? nfft : nfft / 2;
	if (cap < len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "repsim_table: room for %zu floats, the table has %zu", cap, len);
	for (size_t i = 0; i < len; ++i)
		out[i] = which == ZEN_HIP_REPSIM_TABLE_WINDOW ? window_at(i, nfft) : divisor_at(i, nfft);
	return ZEN_HIP_OK;
}

} // extern "C"
