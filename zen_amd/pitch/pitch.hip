// pitch.hip -- the C ABI of libzen_hip_pitch.so (zen_hip_pitch.h): the McLeod pitch method on chunks of device rows.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as live.hip and ragged.hip are: the two transforms
// are zen_hip_fft_exec_batched on a 2n-point handle, memory comes from zen_hip_malloc, and the kernels of pitch_kernels.hip
// stand in front (pad), between (power) and behind (pick).
//
// One slice (at most max_chunks chunks of every stream; workspace row w = s * chunks + c):
//   pad      chunk -> (x, 0) ++ zeros in z[w], the double prefix of the squares in prefix[w]
//   forward  2n-point FFT of every row of z, in place
//   power    z = (re^2 + im^2, 0)
//   inverse  2n-point inverse FFT, in place: the autocorrelation in the real parts
//   pick     NSDF, key maxima, the chosen peak -> the caller's rows
#include <hip/hip_runtime.h>

#include <cstdint>

#include "zen_hip_pitch.h"

#include "../addon/addon_host.h"
#include "pitch_kernels.h"

using namespace zen_addon;

namespace {

enum { K_PAD = 0, K_FWD = 1, K_POWER = 2, K_INV = 3, K_PICK = 4, K_COUNT = ZEN_HIP_PITCH_KERNELS };

} // namespace

struct zen_hip_pitch : Handle<K_COUNT> {
	float fs = 0.f;
	size_t n = 0, S = 0, max_chunks = 0;
	zen_hip_fft_t fft = nullptr; // 2n points
	float* z = nullptr;        // S * max_chunks rows of 2n complex values
	double* prefix = nullptr;  // S * max_chunks rows of n + 1 doubles
	float* stage_in = nullptr; // the host calls' device rows: S rows of max_chunks * n samples
	float* stage_out[3] = {nullptr, nullptr, nullptr}; // S rows of max_chunks results
	float* stage_nsdf = nullptr;                       // S rows of max_chunks * n
	size_t stage_in_row = 0;
	unsigned long long chunks = 0;
};

namespace {

// `cs` chunks of every stream from chunk c0 of the call on
int run_slice(zen_hip_pitch* h, const float* in_dev, size_t in_stride, size_t step, size_t c0, size_t cs, float* pitch, float* period,
              float* clarity, float* nsdf, size_t out_stride)
{
	const size_t n = h->n, S = h->S, rows = S * cs;
	const unsigned long long row_bytes = sizeof(float) * 4 * n; // one row of z
	{
		zen_pitch::PadArgs a = {in_dev, in_stride, step, c0, h->z, h->prefix, cs, S, (int)n};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_PAD, rows * (sizeof(float) * n + row_bytes + sizeof(double) * 3 * (n + 1))));
		ZA_HIP(zen_pitch::launch_pad(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_FWD, rows * 2 * row_bytes));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->z, rows, 0, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_POWER, rows * 2 * row_bytes));
		ZA_HIP(zen_pitch::launch_power(h->z, rows * 2 * n, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_INV, rows * 2 * row_bytes));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->z, rows, 1, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_pitch::PickArgs a = {h->z, h->prefix, pitch, period, clarity, nsdf, out_stride, c0, cs, S, (int)n, h->fs};
		auto kt = h->prof.on_stream(h->stream);
		// the first half of every row of z (real and imaginary parts share the 64-byte sectors), the prefix twice, the results
		ZA_TRY(kt.begin(K_PICK, rows * (row_bytes / 2 + sizeof(double) * 2 * (n + 1) + sizeof(float) * (nsdf ? n : 0)
		                                + sizeof(float) * ((pitch != nullptr) + (period != nullptr) + (clarity != nullptr)))));
		ZA_HIP(zen_pitch::launch_pick(a, h->stream));
		ZA_TRY(kt.end());
	}
	h->chunks += rows;
	return ZEN_HIP_OK;
}

int check_rows(const char* who, zen_hip_pitch_t h, const void* in, size_t n_chunks, size_t step, const void* pitch, const void* period,
               const void* clarity, const void* nsdf, size_t out_stride)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (n_chunks && !in)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input", who);
	if (step == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: step must be at least 1", who);
	if (((uintptr_t)in & 3) || ((uintptr_t)pitch & 3) || ((uintptr_t)period & 3) || ((uintptr_t)clarity & 3) || ((uintptr_t)nsdf & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if ((pitch || period || clarity || nsdf) && out_stride < n_chunks)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu chunks of a row", who, out_stride, n_chunks);
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host and device memory, one per stream
int copy_rows(zen_hip_pitch* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, hipMemcpyKind kind)
{
	return h->copy_rows(dst, dst_stride, src, src_stride, cnt, h->S, kind);
}

} // namespace

extern "C" {

const char* zen_hip_pitch_last_error(void) { return t_err; }
const char* zen_hip_pitch_version(void) { return "zen_hip_pitch 1 (gfx950)"; }

int zen_hip_pitch_create(float fs, size_t n, size_t n_streams, size_t max_chunks, zen_hip_pitch_t* out)
{
	if (!out || n_streams == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_create: null handle or zero streams");
	if (!is_pow2(n) || n < 32 || n > 16384)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_create: chunk length %zu is not a power of two in 32..16384", n);
	if (!(fs > 0.f))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_create: sample rate %g", (double)fs);
	if (max_chunks == 0) {
		max_chunks = ((size_t)1 << 23) / n / n_streams;
		max_chunks = max_chunks < 1 ? 1 : max_chunks > 65536 ? 65536 : max_chunks;
	}
	zen_hip_pitch* h = new zen_hip_pitch;
	h->fs = fs;
	h->n = n;
	h->S = n_streams;
	h->max_chunks = max_chunks;
	auto build = [&]() -> int {
		const size_t rows = n_streams * max_chunks;
		ZA_ZEN(zen_hip_fft_create(2 * n, &h->fft));
		ZA_HIP(zen_pitch::prepare_pick((int)n));
		ZA_TRY(h->alloc(&h->z, rows * 4 * n));
		ZA_TRY(h->alloc(&h->prefix, rows * (n + 1)));
		h->stage_in_row = max_chunks * n;
		ZA_TRY(h->alloc(&h->stage_in, n_streams * h->stage_in_row));
		for (float*& p : h->stage_out)
			ZA_TRY(h->alloc(&p, rows));
		ZA_TRY(h->alloc(&h->stage_nsdf, rows * n));
		// whatever the transform allocates for its largest batch, up front: one run on zeros
		ZA_HIP(hipMemsetAsync(h->z, 0, sizeof(float) * rows * 4 * n, h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft, h->z, rows, 0, h->stream));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_pitch_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_destroy(zen_hip_pitch_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft);
	h->release({h->z, h->prefix, h->stage_in, h->stage_out[0], h->stage_out[1], h->stage_out[2], h->stage_nsdf});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_set_stream(zen_hip_pitch_t h, void* stream) { return set_stream(h, stream, "pitch"); }

int zen_hip_pitch_run_device(zen_hip_pitch_t h, const float* in_dev, size_t in_stride, size_t n_chunks, size_t step, float* pitch_dev,
                             float* period_dev, float* clarity_dev, float* nsdf_dev, size_t out_stride)
{
	ZA_TRY(check_rows("pitch_run_device", h, in_dev, n_chunks, step, pitch_dev, period_dev, clarity_dev, nsdf_dev, out_stride));
	for (size_t c0 = 0; c0 < n_chunks; c0 += h->max_chunks) {
		const size_t cs = n_chunks - c0 < h->max_chunks ? n_chunks - c0 : h->max_chunks;
		ZA_TRY(run_slice(h, in_dev, in_stride, step, c0, cs, pitch_dev, period_dev, clarity_dev, nsdf_dev, out_stride));
	}
	return ZEN_HIP_OK;
}

int zen_hip_pitch_run_host(zen_hip_pitch_t h, const float* in_host, size_t in_stride, size_t n_chunks, size_t step, float* pitch_host,
                           float* period_host, float* clarity_host, float* nsdf_host, size_t out_stride)
{
	ZA_TRY(check_rows("pitch_run_host", h, in_host, n_chunks, step, pitch_host, period_host, clarity_host, nsdf_host, out_stride));
	const size_t n = h->n;
	float* host[3] = {pitch_host, period_host, clarity_host};
	int rc = ZEN_HIP_OK;
	for (size_t c0 = 0; c0 < n_chunks && rc == ZEN_HIP_OK; c0 += h->max_chunks) {
		const size_t cs = n_chunks - c0 < h->max_chunks ? n_chunks - c0 : h->max_chunks;
		// Up: the span of the slice where its chunks touch or overlap, chunk by chunk (packed) where they leave gaps.  Down:
		// the results of the slice.  The next slice overwrites the staging rows: stream order keeps that behind these copies.
		size_t dev_step = step;
		if (step <= n) {
			rc = copy_rows(h, h->stage_in, h->stage_in_row, in_host + c0 * step, in_stride, (cs - 1) * step + n, hipMemcpyHostToDevice);
		} else {
			dev_step = n;
			for (size_t c = 0; c < cs && rc == ZEN_HIP_OK; ++c)
				rc = copy_rows(h, h->stage_in + c * n, h->stage_in_row, in_host + (c0 + c) * step, in_stride, n, hipMemcpyHostToDevice);
		}
		if (rc == ZEN_HIP_OK)
			rc = run_slice(h, h->stage_in, h->stage_in_row, dev_step, 0, cs, host[0] ? h->stage_out[0] : nullptr,
			               host[1] ? h->stage_out[1] : nullptr, host[2] ? h->stage_out[2] : nullptr, nsdf_host ? h->stage_nsdf : nullptr,
			               h->max_chunks);
		for (int o = 0; o < 3 && rc == ZEN_HIP_OK; ++o)
			if (host[o])
				rc = copy_rows(h, host[o] + c0, out_stride, h->stage_out[o], h->max_chunks, cs, hipMemcpyDeviceToHost);
		if (nsdf_host && rc == ZEN_HIP_OK)
			rc = copy_rows(h, nsdf_host + c0 * n, out_stride * n, h->stage_nsdf, h->max_chunks * n, cs * n, hipMemcpyDeviceToHost);
	}
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_pitch_stats(zen_hip_pitch_t h, zen_hip_pitch_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_stats: null argument");
	out->chunks = h->chunks;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_profile(zen_hip_pitch_t h, int enable) { return profile(h, enable); }

int zen_hip_pitch_profile_get(zen_hip_pitch_t h, double ms[ZEN_HIP_PITCH_KERNELS], unsigned long long bytes[ZEN_HIP_PITCH_KERNELS],
                              unsigned long long launches[ZEN_HIP_PITCH_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "pitch");
}

} // extern "C"
