// nmf.hip -- the C ABI of libzen_hip_nmf.so (zen_hip_nmf.h): supervised NMF of the magnitude spectrogram on clips in device
// memory.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as repsim.hip is: the transforms are
// zen_hip_fft_exec_batched (one N-point handle), memory comes from zen_hip_malloc, and the kernels of nmf_kernels.hip stand
// between them.
//
// One call (n_clips clips of n samples, m frames each):
//   frame, fft, magnitude   every clip at once: the spectra X and the magnitudes V
//   per clip, per iteration: ratio -> Q, update_h (H in place), and where a spectrum is free ratio again and update_w (W in
//   place)
//   per group and clip: mask (X through L_g / L into a copy), ifft, overlap_add -> the caller's row
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "zen_hip_nmf.h"

#include "../addon/stft_host.h"
#include "nmf_kernels.h"

using namespace zen_addon;

namespace {

enum { K_FRAME = 0, K_FFT, K_MAG, K_RATIO_MFMA, K_RATIO_VALU, K_UPH_MFMA, K_UPH_VALU, K_UPW_MFMA, K_UPW_VALU, K_MASK, K_IFFT, K_OLA, K_COUNT };
static_assert(K_COUNT == ZEN_HIP_NMF_KERNELS, "the header names the kernels");
static_assert((int)zen_nmf::MAX_COMPONENTS == ZEN_HIP_NMF_MAX_COMPONENTS && (int)zen_nmf::MAX_FRAMES == ZEN_HIP_NMF_MAX_FRAMES &&
                  (int)zen_nmf::SEGMENT == ZEN_HIP_NMF_SEGMENT,
              "the header states the kernels' limits");

constexpr size_t KMAX = ZEN_HIP_NMF_MAX_COMPONENTS, MMAX = ZEN_HIP_NMF_MAX_FRAMES;
// The route of ZEN_HIP_NMF_ROUTE_DEFAULT.
constexpr bool DEFAULT_MFMA = true;

} // namespace

struct zen_hip_nmf : Handle<K_COUNT> {
	float fs = 0.f;
	size_t N = 0, H = 0, bins = 0, v_stride = 0, K = 0, C = 0, max_samples = 0, max_frames = 0;
	bool mfma = DEFAULT_MFMA;
	zen_hip_fft_t fft = nullptr; // N points
	float* rows = nullptr;      // C * max_frames rows of N complex values: X
	float* masked = nullptr;    // max_frames rows of N complex values: one clip through one group's mask
	float* v = nullptr;         // C * max_frames rows of v_stride floats
	float* q = nullptr;         // max_frames rows of v_stride floats: Q of the clip at hand
	float* tables = nullptr;    // the window (N), the divisor (H)
	float* stage_in = nullptr;  // the host calls' device rows: C rows of max_samples samples
	float* stage_out = nullptr; // one group's stems: C rows of max_samples
	float* stage_w = nullptr;   // C dictionaries of K rows of v_stride floats
	float* stage_h = nullptr;   // C times K rows of max_frames floats
	float* part = nullptr;      // the segments' sums of a split update: part_floats floats, and K per segment behind them
	size_t part_floats = 0;
	unsigned long long calls = 0, clips = 0, iterations = 0;
};

namespace {

// steps 1-2 for every clip
int spectra(zen_hip_nmf* h, const float* in, size_t in_stride, size_t n, size_t m)
{
	const FrameArgs a = {in, h->tables, h->rows, in_stride, n, m, h->C, (int)h->N};
	return zen_addon::spectra(h->prof, h->stream, h->fft, K_FRAME, K_FFT, K_MAG, zen_nmf::launch_frame, zen_nmf::launch_magnitude, a, h->v, h->v_stride);
}

struct Matrices { // one clip's W and H as the caller laid them out
	float* w;
	float* hm;
	size_t w_stride, h_stride;
};

size_t segments_of(size_t L) { return (L + ZEN_HIP_NMF_SEGMENT - 1) / ZEN_HIP_NMF_SEGMENT; }

// An update whose reduction has more than one segment is split by segments over workgroups where the segments' sums fit the
// session's scratch (K x F or K x m outputs are few tiles for 256 compute units); the bits are the same either way.
int product(zen_hip_nmf* h, zen_nmf::Product which, zen_nmf::ProductArgs a, int slot)
{
	const size_t seg = segments_of(a.L);
	const bool split = which != zen_nmf::RATIO && seg > 1 && seg * a.I * a.J <= h->part_floats;
	auto kt = h->prof.on_stream(h->stream);
	ZA_TRY(kt.begin(slot + (h->mfma ? 0 : 1), sizeof(float) * (a.I * a.L + a.L * a.J + 2 * a.I * a.J + (split ? 2 * seg * a.I * a.J : 0))));
	if (split) {
		a.part = h->part;
		a.part_rs = h->part + h->part_floats;
		ZA_HIP(zen_nmf::launch_product_split(which, a, h->mfma, h->stream));
	} else {
		ZA_HIP(zen_nmf::launch_product(which, a, h->mfma, h->stream));
	}
	ZA_TRY(kt.end());
	return ZEN_HIP_OK;
}

// steps 3-5 for one clip, `iterations` times; W and H in place
int fit(zen_hip_nmf* h, const float* v, size_t m, const Matrices& x, size_t fixed, int iterations)
{
	const size_t K = h->K, F = h->bins, vs = h->v_stride;
	const zen_nmf::ProductArgs ratio = {x.hm, x.w, v, h->q, nullptr, x.h_stride, x.w_stride, vs, vs, 0, m, F, K};
	const zen_nmf::ProductArgs up_h = {x.w, h->q, x.hm, x.hm, nullptr, x.w_stride, vs, x.h_stride, x.h_stride, 0, K, m, F};
	float* wf = x.w + fixed * x.w_stride;
	const zen_nmf::ProductArgs up_w = {x.hm + fixed * x.h_stride, h->q, wf, wf, nullptr, x.h_stride, vs, x.w_stride, x.w_stride, 0, K - fixed, F, m};
	for (int it = 0; it < iterations; ++it) {
		ZA_TRY(product(h, zen_nmf::RATIO, ratio, K_RATIO_MFMA));
		ZA_TRY(product(h, zen_nmf::UPDATE_H, up_h, K_UPH_MFMA));
		if (fixed < K) {
			ZA_TRY(product(h, zen_nmf::RATIO, ratio, K_RATIO_MFMA));
			ZA_TRY(product(h, zen_nmf::UPDATE_W, up_w, K_UPW_MFMA));
		}
	}
	h->iterations += (unsigned long long)iterations;
	return ZEN_HIP_OK;
}

// the stem of group g of clip c into `out`
int stem(zen_hip_nmf* h, size_t c, size_t n, size_t m, const Matrices& x, const int* groups, int g, float* out)
{
	const size_t N = h->N;
	zen_nmf::StemArgs a = {h->rows + c * m * 2 * N, h->masked, x.w, x.hm, x.w_stride, x.h_stride, m, (int)N, (int)h->K, {}};
	for (size_t k = 0; k < h->K; ++k)
		if (groups[k] == g)
			a.member[k >> 5] |= 1u << (k & 31);
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_MASK, sizeof(float) * (m * 4 * N + h->K * (m + h->bins))));
		ZA_HIP(zen_nmf::launch_stem_mask(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_IFFT, sizeof(float) * m * 4 * N));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->masked, m, 1, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_nmf::OlaArgs o = {h->masked, h->tables + N, out, n, (int)N};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_OLA, sizeof(float) * n * 4));
		ZA_HIP(zen_nmf::launch_overlap_add(o, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

int check_process(const char* who, zen_hip_nmf_t h, const void* in, size_t in_stride, size_t n, const void* w, size_t w_stride, size_t w_clip_stride,
                  const void* hm, size_t h_stride, size_t h_clip_stride, size_t fixed, int iterations, const int* groups, size_t n_groups,
                  const void* stems, size_t out_stride)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (!in || !w || !hm)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input, dictionary or activations", who);
	if (misaligned(in) || misaligned(w) || misaligned(hm) || (groups && misaligned(stems)))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if (n == 0 || n > h->max_samples)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu samples per clip, the session takes 1..%zu", who, n, h->max_samples);
	if (in_stride < n)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: in_stride %zu below the %zu samples of a clip", who, in_stride, n);
	const size_t m = frames_of(n, h->H), K = h->K, F = h->bins;
	if (fixed > K)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu spectra held, the session has %zu components", who, fixed, K);
	if (iterations < 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %d iterations", who, iterations);
	if (w_stride < F || h_stride < m)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: w_stride %zu below the %zu bins or h_stride %zu below the %zu frames", who, w_stride, F, h_stride, m);
	if (w_clip_stride == 0 && fixed < K)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: one dictionary for every clip (w_clip_stride 0) with %zu of %zu spectra held: the clips would race on W", who,
		        fixed, K);
	if ((w_clip_stride != 0 && w_clip_stride < (K - 1) * w_stride + F) || h_clip_stride < (K - 1) * h_stride + m)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: w_clip_stride %zu or h_clip_stride %zu below a clip's %zu rows", who, w_clip_stride, h_clip_stride, K);
	if (groups) {
		if (n_groups < 1 || n_groups > K)
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu groups outside 1..%zu", who, n_groups, K);
		for (size_t k = 0; k < K; ++k)
			if (groups[k] < -1 || groups[k] >= (int)n_groups)
				ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: group %d of component %zu outside -1..%zu", who, groups[k], k, n_groups - 1);
		if (!stems)
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: groups without a place for the stems", who);
		if (out_stride < n)
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu samples of a clip", who, out_stride, n);
	}
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host and device memory
int check_alone(const char* who, const void* const* ptrs, int count, size_t K, size_t F, size_t m, int route)
{
	for (int i = 0; i < count; ++i)
		if (!ptrs[i] || misaligned(ptrs[i]))
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned pointer", who);
	if (K < 1 || K > KMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu components, outside 1..%zu", who, K, KMAX);
	if (m < 1 || m > MMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu frames, outside 1..%zu", who, m, MMAX);
	if (F < 1 || F > MMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu bins, outside 1..%zu", who, F, MMAX);
	if (route != ZEN_HIP_NMF_ROUTE_DEFAULT && route != ZEN_HIP_NMF_ROUTE_MFMA && route != ZEN_HIP_NMF_ROUTE_VALU)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: unknown route %d", who, route);
	return ZEN_HIP_OK;
}

bool route_mfma(int route) { return route == ZEN_HIP_NMF_ROUTE_DEFAULT ? DEFAULT_MFMA : route == ZEN_HIP_NMF_ROUTE_MFMA; }

} // namespace

extern "C" {

const char* zen_hip_nmf_last_error(void) { return t_err; }
const char* zen_hip_nmf_version(void) { return "zen_hip_nmf 1 (gfx950)"; }

int zen_hip_nmf_create(float fs, size_t nfft, size_t components, size_t n_clips, size_t max_samples, zen_hip_nmf_t* out)
{
	if (!out || n_clips == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_create: null handle or zero clips");
	if (!frame_ok(nfft))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_create: frame %zu is not a power of two in 64..8192", nfft);
	if (!(fs > 0.0f) || !std::isfinite(fs))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_create: sample rate %g", (double)fs);
	if (components < 1 || components > KMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_create: %zu components, outside 1..%zu", components, KMAX);
	const size_t H = nfft / 2;
	if (max_samples == 0 || max_samples > MMAX * H || frames_of(max_samples, H) > MMAX)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_create: max_samples %zu is not 1..%zu: a clip may have %zu frames of %zu samples at the most", max_samples,
		        (MMAX - 1) * H, MMAX, H);
	if (n_clips > ((size_t)1 << 16))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_create: n_clips %zu above 2^16", n_clips);
	zen_hip_nmf* h = new zen_hip_nmf;
	h->fs = fs;
	h->N = nfft;
	h->H = H;
	h->bins = H + 1;
	h->v_stride = (h->bins + 3) & ~(size_t)3;
	h->K = components;
	h->C = n_clips;
	h->max_samples = max_samples;
	h->max_frames = frames_of(max_samples, H);
	const char* env = getenv("ZEN_HIP_NMF");
	if (env && strstr(env, "mfma=0"))
		h->mfma = false;
	else if (env && strstr(env, "mfma=1"))
		h->mfma = true;
	auto build = [&]() -> int {
		const size_t frames = n_clips * h->max_frames;
		const std::vector<float> tab = stft_tables(nfft);
		ZA_ZEN(zen_hip_fft_create(nfft, &h->fft));
		ZA_TRY(h->alloc(&h->rows, frames * 2 * nfft));
		ZA_TRY(h->alloc(&h->masked, h->max_frames * 2 * nfft));
		ZA_TRY(h->alloc(&h->v, frames * h->v_stride));
		ZA_TRY(h->alloc(&h->q, h->max_frames * h->v_stride));
		ZA_TRY(h->alloc(&h->tables, tab.size()));
		ZA_TRY(h->alloc(&h->stage_in, n_clips * max_samples));
		ZA_TRY(h->alloc(&h->stage_out, n_clips * max_samples));
		ZA_TRY(h->alloc(&h->stage_w, n_clips * components * h->v_stride));
		ZA_TRY(h->alloc(&h->stage_h, n_clips * components * h->max_frames));
		// the larger of the two updates' segment sums, as far as SPLIT_BYTES go: a longer one walks its segments in sequence
		const size_t need_h = segments_of(h->bins) * components * h->max_frames, need_w = segments_of(h->max_frames) * components * h->bins;
		const size_t cap = ZEN_HIP_NMF_SPLIT_BYTES / sizeof(float);
		h->part_floats = std::max(need_h <= cap ? need_h : 0, need_w <= cap ? need_w : 0);
		ZA_TRY(h->alloc(&h->part, h->part_floats + (size_t)(ZEN_HIP_NMF_MAX_FRAMES / ZEN_HIP_NMF_SEGMENT) * components));
		ZA_ZEN(zen_hip_memcpy_h2d(h->tables, tab.data(), sizeof(float) * tab.size()));
		// whatever the transform allocates for its largest batch, up front: one run on zeros
		ZA_HIP(hipMemsetAsync(h->rows, 0, sizeof(float) * frames * 2 * nfft, h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->rows, frames, 0, h->stream));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_nmf_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_nmf_destroy(zen_hip_nmf_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft);
	h->release({h->rows, h->masked, h->v, h->q, h->tables, h->stage_in, h->stage_out, h->stage_w, h->stage_h, h->part});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_nmf_set_stream(zen_hip_nmf_t h, void* stream) { return set_stream(h, stream, "nmf"); }

int zen_hip_nmf_process_device(zen_hip_nmf_t h, const float* in_dev, size_t in_stride, size_t n, float* w_dev, size_t w_stride,
                               size_t w_clip_stride, float* h_dev, size_t h_stride, size_t h_clip_stride, size_t fixed, int iterations,
                               const int* groups_host, size_t n_groups, float* stems_dev, size_t out_stride)
{
	ZA_TRY(check_process("nmf_process_device", h, in_dev, in_stride, n, w_dev, w_stride, w_clip_stride, h_dev, h_stride, h_clip_stride, fixed,
	                     iterations, groups_host, n_groups, stems_dev, out_stride));
	const size_t m = frames_of(n, h->H);
	ZA_TRY(spectra(h, in_dev, in_stride, n, m));
	for (size_t c = 0; c < h->C; ++c) {
		const Matrices x = {w_dev + c * w_clip_stride, h_dev + c * h_clip_stride, w_stride, h_stride};
		ZA_TRY(fit(h, h->v + c * m * h->v_stride, m, x, fixed, iterations));
	}
	if (groups_host)
		for (size_t g = 0; g < n_groups; ++g)
			for (size_t c = 0; c < h->C; ++c) {
				const Matrices x = {w_dev + c * w_clip_stride, h_dev + c * h_clip_stride, w_stride, h_stride};
				ZA_TRY(stem(h, c, n, m, x, groups_host, (int)g, stems_dev + (g * h->C + c) * out_stride));
			}
	h->calls += 1;
	h->clips += h->C;
	return ZEN_HIP_OK;
}

int zen_hip_nmf_process_host(zen_hip_nmf_t h, const float* in_host, size_t in_stride, size_t n, float* w_host, size_t w_stride,
                             size_t w_clip_stride, float* h_host, size_t h_stride, size_t h_clip_stride, size_t fixed, int iterations,
                             const int* groups_host, size_t n_groups, float* stems_host, size_t out_stride)
{
	ZA_TRY(check_process("nmf_process_host", h, in_host, in_stride, n, w_host, w_stride, w_clip_stride, h_host, h_stride, h_clip_stride, fixed,
	                     iterations, groups_host, n_groups, stems_host, out_stride));
	const size_t C = h->C, K = h->K, F = h->bins, m = frames_of(n, h->H), row = h->max_samples, ws = h->v_stride, hs = h->max_frames;
	const size_t wcs = w_clip_stride ? K * ws : 0, hcs = K * hs, dicts = w_clip_stride ? C : 1;
	auto run = [&]() -> int {
		ZA_TRY(h->copy_rows(h->stage_in, row, in_host, in_stride, n, C, hipMemcpyHostToDevice));
		for (size_t c = 0; c < dicts; ++c)
			ZA_TRY(h->copy_rows(h->stage_w + c * wcs, ws, w_host + c * w_clip_stride, w_stride, F, K, hipMemcpyHostToDevice));
		for (size_t c = 0; c < C; ++c)
			ZA_TRY(h->copy_rows(h->stage_h + c * hcs, hs, h_host + c * h_clip_stride, h_stride, m, K, hipMemcpyHostToDevice));
		ZA_TRY(spectra(h, h->stage_in, row, n, m));
		for (size_t c = 0; c < C; ++c) {
			const Matrices x = {h->stage_w + c * wcs, h->stage_h + c * hcs, ws, hs};
			ZA_TRY(fit(h, h->v + c * m * h->v_stride, m, x, fixed, iterations));
		}
		if (fixed < K) // held spectra are what the caller has
			for (size_t c = 0; c < dicts; ++c)
				ZA_TRY(h->copy_rows(w_host + c * w_clip_stride + fixed * w_stride, w_stride, h->stage_w + c * wcs + fixed * ws, ws, F, K - fixed,
				                 hipMemcpyDeviceToHost));
		for (size_t c = 0; c < C; ++c)
			ZA_TRY(h->copy_rows(h_host + c * h_clip_stride, h_stride, h->stage_h + c * hcs, hs, m, K, hipMemcpyDeviceToHost));
		if (groups_host)
			for (size_t g = 0; g < n_groups; ++g) { // one group's rows at a time through the stage
				for (size_t c = 0; c < C; ++c) {
					const Matrices x = {h->stage_w + c * wcs, h->stage_h + c * hcs, ws, hs};
					ZA_TRY(stem(h, c, n, m, x, groups_host, (int)g, h->stage_out + c * row));
				}
				ZA_TRY(h->copy_rows(stems_host + g * C * out_stride, out_stride, h->stage_out, row, n, C, hipMemcpyDeviceToHost));
			}
		return ZEN_HIP_OK;
	};
	const int rc = run();
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	h->calls += 1;
	h->clips += C;
	return ZEN_HIP_OK;
}

int zen_hip_nmf_ratio_device(const float* v_dev, size_t v_stride, const float* w_dev, size_t w_stride, const float* h_dev, size_t h_stride,
                             size_t components, size_t bins, size_t frames, float* q_dev, size_t q_stride, float* lam_dev, size_t lam_stride,
                             int route, void* stream)
{
	const char* who = "nmf_ratio_device";
	const void* ptrs[] = {v_dev, w_dev, h_dev, q_dev};
	ZA_TRY(check_alone(who, ptrs, 4, components, bins, frames, route));
	if (misaligned(lam_dev))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned pointer", who);
	if (v_stride < bins || w_stride < bins || q_stride < bins || h_stride < frames || (lam_dev && lam_stride < bins))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a stride below its row: %zu bins in rows %zu (V), %zu (W), %zu (Q), %zu (L) floats apart, %zu frames in rows %zu",
		        who, bins, v_stride, w_stride, q_stride, lam_stride, frames, h_stride);
	const zen_nmf::ProductArgs a = {h_dev, w_dev, v_dev, q_dev, lam_dev, h_stride, w_stride, v_stride, q_stride, lam_stride, frames, bins, components};
	ZA_HIP(zen_nmf::launch_product(zen_nmf::RATIO, a, route_mfma(route), (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_nmf_update_h_device(const float* w_dev, size_t w_stride, const float* q_dev, size_t q_stride, const float* h_dev, size_t h_stride,
                                size_t components, size_t bins, size_t frames, float* out_dev, size_t out_stride, int route, void* stream)
{
	const char* who = "nmf_update_h_device";
	const void* ptrs[] = {w_dev, q_dev, h_dev, out_dev};
	ZA_TRY(check_alone(who, ptrs, 4, components, bins, frames, route));
	if (w_stride < bins || q_stride < bins || h_stride < frames || out_stride < frames)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a stride below its row: %zu bins in rows %zu (W), %zu (Q) floats apart, %zu frames in rows %zu (H), %zu (out)", who,
		        bins, w_stride, q_stride, frames, h_stride, out_stride);
	const zen_nmf::ProductArgs a = {w_dev, q_dev, h_dev, out_dev, nullptr, w_stride, q_stride, h_stride, out_stride, 0, components, frames, bins};
	ZA_HIP(zen_nmf::launch_product(zen_nmf::UPDATE_H, a, route_mfma(route), (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_nmf_update_w_device(const float* h_dev, size_t h_stride, const float* q_dev, size_t q_stride, const float* w_dev, size_t w_stride,
                                size_t components, size_t bins, size_t frames, size_t fixed, float* out_dev, size_t out_stride, int route,
                                void* stream)
{
	const char* who = "nmf_update_w_device";
	const void* ptrs[] = {h_dev, q_dev, w_dev, out_dev};
	ZA_TRY(check_alone(who, ptrs, 4, components, bins, frames, route));
	if (fixed > components)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu spectra held of %zu components", who, fixed, components);
	if (w_stride < bins || q_stride < bins || h_stride < frames || out_stride < bins)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a stride below its row: %zu bins in rows %zu (W), %zu (Q), %zu (out) floats apart, %zu frames in rows %zu (H)", who,
		        bins, w_stride, q_stride, out_stride, frames, h_stride);
	if (fixed == components)
		return ZEN_HIP_OK;
	const zen_nmf::ProductArgs a = {h_dev + fixed * h_stride, q_dev,  w_dev + fixed * w_stride, out_dev + fixed * out_stride, nullptr, h_stride,
	                                q_stride, w_stride, out_stride, 0, components - fixed, bins, frames};
	ZA_HIP(zen_nmf::launch_product(zen_nmf::UPDATE_W, a, route_mfma(route), (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_nmf_stats(zen_hip_nmf_t h, zen_hip_nmf_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_stats: null argument");
	out->calls = h->calls;
	out->clips = h->clips;
	out->iterations = h->iterations;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_nmf_profile(zen_hip_nmf_t h, int enable) { return profile(h, enable); }

int zen_hip_nmf_profile_get(zen_hip_nmf_t h, double ms[ZEN_HIP_NMF_KERNELS], unsigned long long bytes[ZEN_HIP_NMF_KERNELS],
                            unsigned long long launches[ZEN_HIP_NMF_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "nmf");
}

int zen_hip_nmf_init(unsigned long long seed, size_t count, float* out)
{
	if (!out && count)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_init: null output");
	if (misaligned(out))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_init: misaligned output");
	for (size_t i = 0; i < count; ++i) {
		unsigned long long z = seed + (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull;
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		z ^= z >> 31;
		out[i] = (float)((z >> 40) + 1) * 0x1p-24f; // at most 2^24: exact
	}
	return ZEN_HIP_OK;
}

int zen_hip_nmf_table(size_t nfft, int which, float* out, size_t cap)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_table: null output");
	if (!frame_ok(nfft))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_table: frame %zu is not a power of two in 64..8192", nfft);
	if (which != ZEN_HIP_NMF_TABLE_WINDOW && which != ZEN_HIP_NMF_TABLE_DIVISOR)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_table: unknown table %d", which);
	const size_t len = which == ZEN_HIP_NMF_TABLE_WINDOW ? nfft : nfft / 2;
	if (cap < len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "nmf_table: room for %zu floats, the table has %zu", cap, len);
	for (size_t i = 0; i < len; ++i)
		out[i] = which == ZEN_HIP_NMF_TABLE_WINDOW ? window_at(i, nfft) : divisor_at(i, nfft);
	return ZEN_HIP_OK;
}

} // extern "C"
