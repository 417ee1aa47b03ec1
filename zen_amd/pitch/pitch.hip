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

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "zen_hip_pitch.h"

#include "pitch_kernels.h"

namespace {

thread_local char t_err[512] = "";

void set_err(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(t_err, sizeof(t_err), fmt, ap);
	va_end(ap);
}

#define PT_FAIL(code, ...)    \
	do {                      \
		set_err(__VA_ARGS__); \
		return (code);        \
	} while (0)
#define PT_HIP(call)                                                                            \
	do {                                                                                        \
		hipError_t e__ = (call);                                                                \
		if (e__ != hipSuccess) {                                                                \
			set_err("%s:%d: %s failed: %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
			return ZEN_HIP_E_HIP;                                                               \
		}                                                                                       \
	} while (0)
// a call into libzen_hip.so: its message becomes ours
#define PT_ZEN(call)                                        \
	do {                                                    \
		int rc__ = (call);                                  \
		if (rc__ != ZEN_HIP_OK) {                           \
			set_err("%s: %s", #call, zen_hip_last_error()); \
			return rc__;                                    \
		}                                                   \
	} while (0)
#define PT_TRY(expr)            \
	do {                        \
		int rc__ = (expr);      \
		if (rc__ != ZEN_HIP_OK) \
			return rc__;        \
	} while (0)

enum { K_PAD = 0, K_FWD = 1, K_POWER = 2, K_INV = 3, K_PICK = 4, K_COUNT = ZEN_HIP_PITCH_KERNELS };

struct Timed {
	int kernel;
	hipEvent_t e0, e1;
};

} // namespace

struct zen_hip_pitch {
	float fs = 0.f;
	size_t n = 0, S = 0, max_chunks = 0;
	zen_hip_fft_t fft = nullptr; // 2n points
	hipStream_t stream = nullptr;
	float* z = nullptr;        // S * max_chunks rows of 2n complex values
	double* prefix = nullptr;  // S * max_chunks rows of n + 1 doubles
	float* stage_in = nullptr; // the host calls' device rows: S rows of max_chunks * n samples
	float* stage_out[3] = {nullptr, nullptr, nullptr}; // S rows of max_chunks results
	float* stage_nsdf = nullptr;                       // S rows of max_chunks * n
	size_t stage_in_row = 0;
	unsigned long long chunks = 0, device_bytes = 0, allocations = 0;
	bool profile = false;
	std::vector<Timed> timed;
	double prof_ms[K_COUNT] = {};
	unsigned long long prof_bytes[K_COUNT] = {}, prof_launches[K_COUNT] = {};
};

namespace {

template <class T>
int alloc(zen_hip_pitch* h, T** p, size_t count)
{
	PT_ZEN(zen_hip_malloc((void**)p, sizeof(T) * count));
	h->device_bytes += sizeof(T) * count;
	h->allocations += 1;
	return ZEN_HIP_OK;
}

struct KernelTimer { // HIP events around one launch while profiling is on
	zen_hip_pitch* h;
	Timed t = {0, nullptr, nullptr};
	int begin(int kernel, unsigned long long bytes)
	{
		if (!h->profile)
			return ZEN_HIP_OK;
		t.kernel = kernel;
		PT_HIP(hipEventCreate(&t.e0));
		PT_HIP(hipEventCreate(&t.e1));
		PT_HIP(hipEventRecord(t.e0, h->stream));
		h->prof_bytes[kernel] += bytes;
		h->prof_launches[kernel] += 1;
		return ZEN_HIP_OK;
	}
	int end()
	{
		if (!h->profile)
			return ZEN_HIP_OK;
		PT_HIP(hipEventRecord(t.e1, h->stream));
		h->timed.push_back(t);
		return ZEN_HIP_OK;
	}
};

// `cs` chunks of every stream from chunk c0 of the call on
int run_slice(zen_hip_pitch* h, const float* in_dev, size_t in_stride, size_t step, size_t c0, size_t cs, float* pitch, float* period,
              float* clarity, float* nsdf, size_t out_stride)
{
	const size_t n = h->n, S = h->S, rows = S * cs;
	const unsigned long long row_bytes = sizeof(float) * 4 * n; // one row of z
	{
		zen_pitch::PadArgs a = {in_dev, in_stride, step, c0, h->z, h->prefix, cs, S, (int)n};
		KernelTimer kt{h};
		PT_TRY(kt.begin(K_PAD, rows * (sizeof(float) * n + row_bytes + sizeof(double) * 3 * (n + 1))));
		PT_HIP(zen_pitch::launch_pad(a, h->stream));
		PT_TRY(kt.end());
	}
	{
		KernelTimer kt{h};
		PT_TRY(kt.begin(K_FWD, rows * 2 * row_bytes));
		PT_ZEN(zen_hip_fft_exec_batched(h->fft, h->z, rows, 0, h->stream));
		PT_TRY(kt.end());
	}
	{
		KernelTimer kt{h};
		PT_TRY(kt.begin(K_POWER, rows * 2 * row_bytes));
		PT_HIP(zen_pitch::launch_power(h->z, rows * 2 * n, h->stream));
		PT_TRY(kt.end());
	}
	{
		KernelTimer kt{h};
		PT_TRY(kt.begin(K_INV, rows * 2 * row_bytes));
		PT_ZEN(zen_hip_fft_exec_batched(h->fft, h->z, rows, 1, h->stream));
		PT_TRY(kt.end());
	}
	{
		zen_pitch::PickArgs a = {h->z, h->prefix, pitch, period, clarity, nsdf, out_stride, c0, cs, S, (int)n, h->fs};
		KernelTimer kt{h};
		// the first half of every row of z (real and imaginary parts share the 64-byte sectors), the prefix twice, the results
		PT_TRY(kt.begin(K_PICK, rows * (row_bytes / 2 + sizeof(double) * 2 * (n + 1) + sizeof(float) * (nsdf ? n : 0)
		                                + sizeof(float) * ((pitch != nullptr) + (period != nullptr) + (clarity != nullptr)))));
		PT_HIP(zen_pitch::launch_pick(a, h->stream));
		PT_TRY(kt.end());
	}
	h->chunks += rows;
	return ZEN_HIP_OK;
}

int check_rows(const char* who, zen_hip_pitch_t h, const void* in, size_t n_chunks, size_t step, const void* pitch, const void* period,
               const void* clarity, const void* nsdf, size_t out_stride)
{
	if (!h)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (n_chunks && !in)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null input", who);
	if (step == 0)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "%s: step must be at least 1", who);
	if (((uintptr_t)in & 3) || ((uintptr_t)pitch & 3) || ((uintptr_t)period & 3) || ((uintptr_t)clarity & 3) || ((uintptr_t)nsdf & 3))
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if ((pitch || period || clarity || nsdf) && out_stride < n_chunks)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu chunks of a row", who, out_stride, n_chunks);
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host and device memory
int copy_rows(zen_hip_pitch* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, hipMemcpyKind kind)
{
	if (cnt)
		PT_HIP(hipMemcpy2DAsync(dst, sizeof(float) * dst_stride, src, sizeof(float) * src_stride, sizeof(float) * cnt, h->S, kind, h->stream));
	return ZEN_HIP_OK;
}

bool is_pow2(size_t x) { return x && (x & (x - 1)) == 0; }

} // namespace

extern "C" {

const char* zen_hip_pitch_last_error(void) { return t_err; }
const char* zen_hip_pitch_version(void) { return "zen_hip_pitch 1 (gfx950)"; }

int zen_hip_pitch_create(float fs, size_t n, size_t n_streams, size_t max_chunks, zen_hip_pitch_t* out)
{
	if (!out || n_streams == 0)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_create: null handle or zero streams");
	if (!is_pow2(n) || n < 32 || n > 16384)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_create: chunk length %zu is not a power of two in 32..16384", n);
	if (!(fs > 0.f))
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_create: sample rate %g", (double)fs);
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
		PT_ZEN(zen_hip_fft_create(2 * n, &h->fft));
		PT_HIP(zen_pitch::prepare_pick((int)n));
		PT_TRY(alloc(h, &h->z, rows * 4 * n));
		PT_TRY(alloc(h, &h->prefix, rows * (n + 1)));
		h->stage_in_row = max_chunks * n;
		PT_TRY(alloc(h, &h->stage_in, n_streams * h->stage_in_row));
		for (float*& p : h->stage_out)
			PT_TRY(alloc(h, &p, rows));
		PT_TRY(alloc(h, &h->stage_nsdf, rows * n));
		// whatever the transform allocates for its largest batch, up front: one run on zeros
		PT_HIP(hipMemsetAsync(h->z, 0, sizeof(float) * rows * 4 * n, h->stream));
		PT_ZEN(zen_hip_fft_exec_batched(h->fft, h->z, rows, 0, h->stream));
		PT_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	const int rc = build();
	if (rc != ZEN_HIP_OK) {
		char keep[sizeof(t_err)];
		memcpy(keep, t_err, sizeof(keep));
		zen_hip_pitch_destroy(h);
		memcpy(t_err, keep, sizeof(keep));
		return rc;
	}
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_destroy(zen_hip_pitch_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft);
	void* bufs[] = {h->z, h->prefix, h->stage_in, h->stage_out[0], h->stage_out[1], h->stage_out[2], h->stage_nsdf};
	for (void* b : bufs)
		(void)zen_hip_free(b);
	for (Timed& t : h->timed) {
		(void)hipEventDestroy(t.e0);
		(void)hipEventDestroy(t.e1);
	}
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_set_stream(zen_hip_pitch_t h, void* stream)
{
	if (!h)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_set_stream: null handle");
	PT_HIP(hipStreamSynchronize(h->stream));
	h->stream = (hipStream_t)stream;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_run_device(zen_hip_pitch_t h, const float* in_dev, size_t in_stride, size_t n_chunks, size_t step, float* pitch_dev,
                             float* period_dev, float* clarity_dev, float* nsdf_dev, size_t out_stride)
{
	PT_TRY(check_rows("pitch_run_device", h, in_dev, n_chunks, step, pitch_dev, period_dev, clarity_dev, nsdf_dev, out_stride));
	for (size_t c0 = 0; c0 < n_chunks; c0 += h->max_chunks) {
		const size_t cs = n_chunks - c0 < h->max_chunks ? n_chunks - c0 : h->max_chunks;
		PT_TRY(run_slice(h, in_dev, in_stride, step, c0, cs, pitch_dev, period_dev, clarity_dev, nsdf_dev, out_stride));
	}
	return ZEN_HIP_OK;
}

int zen_hip_pitch_run_host(zen_hip_pitch_t h, const float* in_host, size_t in_stride, size_t n_chunks, size_t step, float* pitch_host,
                           float* period_host, float* clarity_host, float* nsdf_host, size_t out_stride)
{
	PT_TRY(check_rows("pitch_run_host", h, in_host, n_chunks, step, pitch_host, period_host, clarity_host, nsdf_host, out_stride));
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
	PT_TRY(rc);
	PT_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_pitch_stats(zen_hip_pitch_t h, zen_hip_pitch_stats_t* out)
{
	if (!h || !out)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_stats: null argument");
	out->chunks = h->chunks;
	out->device_bytes = h->device_bytes;
	out->allocations = h->allocations;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_profile(zen_hip_pitch_t h, int enable)
{
	if (!h)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	h->profile = enable != 0;
	return ZEN_HIP_OK;
}

int zen_hip_pitch_profile_get(zen_hip_pitch_t h, double ms[ZEN_HIP_PITCH_KERNELS], unsigned long long bytes[ZEN_HIP_PITCH_KERNELS],
                              unsigned long long launches[ZEN_HIP_PITCH_KERNELS])
{
	if (!h || !ms || !bytes || !launches)
		PT_FAIL(ZEN_HIP_E_BAD_ARG, "pitch_profile_get: null argument");
	hipError_t e = hipSuccess;
	for (Timed& t : h->timed) {
		float v = 0.f;
		if (e == hipSuccess)
			e = hipEventSynchronize(t.e1);
		if (e == hipSuccess)
			e = hipEventElapsedTime(&v, t.e0, t.e1);
		h->prof_ms[t.kernel] += v;
		(void)hipEventDestroy(t.e0);
		(void)hipEventDestroy(t.e1);
	}
	h->timed.clear();
	for (int k = 0; k < K_COUNT; ++k) {
		ms[k] = h->prof_ms[k];
		bytes[k] = h->prof_bytes[k];
		launches[k] = h->prof_launches[k];
		h->prof_ms[k] = 0;
		h->prof_bytes[k] = h->prof_launches[k] = 0;
	}
	PT_HIP(e);
	return ZEN_HIP_OK;
}

} // extern "C"
