// addon_host.h -- what the host sources of the add-on libraries share (zen_amd/pcm, ragged, live, pitch and every add-on
// since: each a library of its own on top of libzen_hip.so's C ABI, include/zen_hip.h): the thread's error message and the
// macros that set it, the per-kernel profile, the counting allocator and the roll-back of a create function.  What the
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
