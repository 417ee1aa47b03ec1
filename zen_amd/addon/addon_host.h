// addon_host.h -- what the host sources of the add-on libraries share (zen_amd/pcm, ragged, live, pitch and every add-on
// since: each a library of its own on top of libzen_hip.so's C ABI, include/zen_hip.h): the thread's error message and the
// macros that set it, the per-kernel profile, the counting allocator, the base of a handle that owns both with its stream
// and its row copies, the bodies of the calls every library exports around it, and the roll-back of a create function.  What the
// spectrogram add-ons share beyond that is stft_host.h and, on the device side, stft_kernels.h and median_select.h.
//
// Header-only, and everything in it has internal linkage (the anonymous namespace): the libraries are routinely loaded into
// one process, and a symbol of default visibility would be resolved to whichever of them was loaded first -- one library's
// message in another library's buffer.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "zen_hip.h"

namespace zen_addon {
namespace {

thread_local char t_err[512] = "";

void set_err(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(t_err, sizeof(t_err), fmt, ap);
	va_end(ap);
}

#define ZA_FAIL(code, ...)               \
	do {                                 \
		zen_addon::set_err(__VA_ARGS__); \
		return (code);                   \
	} while (0)
// `what`: the text of the call in the message, for code that moved here and keeps the words its library's message had
#define ZA_HIP_AS(call, what)                                                                             \
	do {                                                                                                  \
		hipError_t e__ = (call);                                                                          \
		if (e__ != hipSuccess) {                                                                          \
			zen_addon::set_err("%s:%d: %s failed: %s", __FILE__, __LINE__, what, hipGetErrorString(e__)); \
			return ZEN_HIP_E_HIP;                                                                         \
		}                                                                                                 \
	} while (0)
#define ZA_HIP(call) ZA_HIP_AS(call, #call)
// a call into libzen_hip.so: its message becomes ours
#define ZA_ZEN_AS(call, what)                                         \
	do {                                                              \
		int rc__ = (call);                                            \
		if (rc__ != ZEN_HIP_OK) {                                     \
			zen_addon::set_err("%s: %s", what, zen_hip_last_error()); \
			return rc__;                                              \
		}                                                             \
	} while (0)
#define ZA_ZEN(call) ZA_ZEN_AS(call, #call)
#define ZA_TRY(expr)            \
	do {                        \
		int rc__ = (expr);      \
		if (rc__ != ZEN_HIP_OK) \
			return rc__;        \
	} while (0)

// The profile of a handle with K kernels: while it is on, HIP events around every launch, and per kernel the bytes the
// caller states and the launches; drain() turns the events into milliseconds.
template <int K>
struct Profiler {
	struct Timed {
		int kernel;
		hipEvent_t e0, e1;
	};
	bool on = false;
	std::vector<Timed> timed;
	double ms[K] = {};
	unsigned long long bytes[K] = {}, launches[K] = {};

	struct Timer { // one launch: begin, the launch on `stream`, end
		Profiler* p;
		hipStream_t stream;
		Timed t;
		int begin(int kernel, unsigned long long nbytes)
		{
			if (!p->on)
				return ZEN_HIP_OK;
			t.kernel = kernel;
			ZA_HIP(hipEventCreate(&t.e0));
			ZA_HIP(hipEventCreate(&t.e1));
			ZA_HIP_AS(hipEventRecord(t.e0, stream), "hipEventRecord(t.e0, h->stream)");
			p->bytes[kernel] += nbytes;
			p->launches[kernel] += 1;
			return ZEN_HIP_OK;
		}
		int end()
		{
			if (!p->on)
				return ZEN_HIP_OK;
			ZA_HIP_AS(hipEventRecord(t.e1, stream), "hipEventRecord(t.e1, h->stream)");
			p->timed.push_back(t);
			return ZEN_HIP_OK;
		}
	};
	Timer on_stream(hipStream_t stream) { return Timer{this, stream, {0, nullptr, nullptr}}; }

	// Waits for every timed launch, hands out what has accumulated since the last call and starts again from zero.  A HIP
	// error is reported last: the events are gone and the counters are zero all the same.
	int drain(double* ms_out, unsigned long long* bytes_out, unsigned long long* launches_out)
	{
		hipError_t e = hipSuccess;
		for (Timed& t : timed) {
			float v = 0.f;
			if (e == hipSuccess)
				e = hipEventSynchronize(t.e1);
			if (e == hipSuccess)
				e = hipEventElapsedTime(&v, t.e0, t.e1);
			ms[t.kernel] += v;
			(void)hipEventDestroy(t.e0);
			(void)hipEventDestroy(t.e1);
		}
		timed.clear();
		for (int k = 0; k < K; ++k) {
			ms_out[k] = ms[k];
			bytes_out[k] = bytes[k];
			launches_out[k] = launches[k];
			ms[k] = 0;
			bytes[k] = launches[k] = 0;
		}
		ZA_HIP(e);
		return ZEN_HIP_OK;
	}

	void release() // destroy: the events that were never drained
	{
		for (Timed& t : timed) {
			(void)hipEventDestroy(t.e0);
			(void)hipEventDestroy(t.e1);
		}
		timed.clear();
	}
};

// What a handle has taken from zen_hip_malloc, for its stats.
struct DeviceTally {
	unsigned long long device_bytes = 0, allocations = 0;
};

// `what`: the text of the allocation in the caller's message (inline: not every library allocates through it)
inline int counted_malloc(DeviceTally* t, void** p, size_t bytes, const char* what)
{
	ZA_ZEN_AS(zen_hip_malloc(p, bytes), what);
	t->device_bytes += bytes;
	t->allocations += 1;
	return ZEN_HIP_OK;
}

inline bool is_pow2(size_t v) { return v && !(v & (v - 1)); }

// What a library's handle struct inherits: the stream its work goes to, what it has allocated, the profile of its K kernels,
// and the copies between the caller's rows and its own.
template <int K>
struct Handle {
	hipStream_t stream = nullptr;
	DeviceTally mem;
	Profiler<K> prof;

	template <class T>
	int alloc(T** p, size_t count)
	{
		return counted_malloc(&mem, (void**)p, sizeof(T) * count, "zen_hip_malloc((void**)p, sizeof(T) * count)");
	}

	// `rows` rows of `cnt` floats between host and device memory, as one two-dimensional copy
	int copy_rows(void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, size_t rows, hipMemcpyKind kind)
	{
		if (cnt)
			ZA_HIP_AS(hipMemcpy2DAsync(dst, sizeof(float) * dst_stride, src, sizeof(float) * src_stride, sizeof(float) * cnt, rows, kind, stream),
			          "hipMemcpy2DAsync(dst, sizeof(float) * dst_stride, src, sizeof(float) * src_stride, sizeof(float) * cnt, rows, kind, h->stream)");
		return ZEN_HIP_OK;
	}

	// The same rows as one-dimensional copies, for callers whose rows are long and few: one copy where both sides are
	// tight, one per row otherwise.  No two-dimensional copy crosses the link.
	int copy_rows_1d(float* dst, size_t dst_stride, const float* src, size_t src_stride, size_t cnt, size_t rows, hipMemcpyKind kind)
	{
		if (dst_stride == cnt && src_stride == cnt) {
			ZA_HIP_AS(hipMemcpyAsync(dst, src, sizeof(float) * cnt * rows, kind, stream),
			          "hipMemcpyAsync(dst, src, sizeof(float) * cnt * rows, kind, h->stream)");
			return ZEN_HIP_OK;
		}
		for (size_t r = 0; r < rows; ++r)
			ZA_HIP_AS(hipMemcpyAsync(dst + r * dst_stride, src + r * src_stride, sizeof(float) * cnt, kind, stream),
			          "hipMemcpyAsync(dst + r * dst_stride, src + r * src_stride, sizeof(float) * cnt, kind, h->stream)");
		return ZEN_HIP_OK;
	}

	// the tail of a destroy function, behind the wait for the stream: these buffers go, and the events never drained
	void release(std::initializer_list<void*> bufs)
	{
		for (void* b : bufs)
			(void)zen_hip_free(b);
		prof.release();
	}
};

// The bodies of three functions every library exports; `h` is whatever the caller handed in, null included, and `name` the
// library's, for the message.
template <class H>
int set_stream(H* h, void* stream, const char* name)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s_set_stream: null handle", name);
	ZA_HIP_AS(hipStreamSynchronize(h->stream), "hipStreamSynchronize(h->stream)");
	h->stream = (hipStream_t)stream;
	return ZEN_HIP_OK;
}

template <class H>
int profile(H* h, int enable)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "null handle");
	h->prof.on = enable != 0;
	return ZEN_HIP_OK;
}

template <class H>
int profile_get(H* h, double* ms, unsigned long long* bytes, unsigned long long* launches, const char* name)
{
	if (!h || !ms || !bytes || !launches)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s_profile_get: null argument", name);
	return h->prof.drain(ms, bytes, launches);
}

// The second half of a create function: where `build` fails, `destroy` takes the half-built handle apart, and the message
// of the failure outlives whatever that writes.
template <class Build, class Destroy>
int build_or_destroy(Build build, Destroy destroy)
{
	const int rc = build();
	if (rc != ZEN_HIP_OK) {
		char keep[sizeof(t_err)];
		memcpy(keep, t_err, sizeof(keep));
		destroy();
		memcpy(t_err, keep, sizeof(keep));
	}
	return rc;
}

} // namespace
} // namespace zen_addon
