// fake_zen_hip.cpp -- a test double of the C-ABI (include/zen_hip.h) for zen_amd/libzen/hps.cpp: plain C++, no HIP, no device.
// It defines exactly the zen_hip_* symbols the host mirror references, so that hps.cpp can run -- under sanitizers too -- on a
// machine without a GPU (tests/cpp/test_hps_host.cpp, tests/test_host_threads.py).
//   offline pair : harm[i] = 0.5f * x[i], perc[i] = x[i] - harm[i]
//   sink form    : the contract of zen_hip.h (zen_hip_hpri_process_sink): one thread per wanted output, ascending ranges of
//                  fake_zen_hip_range_samples samples handed over from a staging buffer that is overwritten with NaN after
//                  every call of the sink (a sink that keeps the pointer is caught); both threads joined before the return
//   realtime     : fixed parameters, process_* copy the input through; "device" memory is host memory
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>

#include <zen_hip.h>

extern "C" {
// what only the fake exports: set between calls, read by the sink threads
std::size_t fake_zen_hip_range_samples = (std::size_t)4 << 20;
int fake_zen_hip_misbehave = 0; // 1: the first two ranges of each output change places; 2: the last range is left out
}

struct zen_hip_hpr {
	std::size_t hop;
	std::vector<float> last; // the hop(s) of the last process call
};
struct zen_hip_hpri {
	zen_hip_hpri_host_stats stats;
};

namespace {
void deliver(int output, const float* x, std::size_t n, zen_hip_hpri_sink_fn sink, void* user)
{
	const std::size_t len = fake_zen_hip_range_samples;
	std::vector<std::size_t> begins;
	for (std::size_t b = 0; b < n; b += len)
		begins.push_back(b);
	if (fake_zen_hip_misbehave == 1 && begins.size() >= 2)
		std::swap(begins[0], begins[1]);
	if (fake_zen_hip_misbehave == 2)
		begins.pop_back();
	std::vector<float> staging(len < n ? len : n);
	for (std::size_t b : begins) {
		const std::size_t count = n - b < len ? n - b : len;
		for (std::size_t i = 0; i < count; ++i) {
			const float harm = 0.5f * x[b + i];
			staging[i] = output == 0 ? harm : x[b + i] - harm;
		}
		sink(user, output, b, staging.data(), count);
		for (float& s : staging)
			s = std::numeric_limits<float>::quiet_NaN();
	}
}
} // namespace

extern "C" {

const char* zen_hip_last_error(void) { return "fake_zen_hip: no error text"; }
int zen_hip_synchronize(void*) { return ZEN_HIP_OK; }

int zen_hip_malloc(void** dev, size_t bytes)
{
	*dev = std::malloc(bytes ? bytes : 1);
	return *dev ? ZEN_HIP_OK : ZEN_HIP_E_HIP;
}
int zen_hip_free(void* dev)
{
	std::free(dev);
	return ZEN_HIP_OK;
}
int zen_hip_memset(void* dev, int value, size_t bytes, void*)
{
	std::memset(dev, value, bytes);
	return ZEN_HIP_OK;
}
int zen_hip_memcpy_h2d(void* dev, const void* host, size_t bytes)
{
	std::memcpy(dev, host, bytes);
	return ZEN_HIP_OK;
}
int zen_hip_memcpy_d2h(void* host, const void* dev, size_t bytes)
{
	std::memcpy(host, dev, bytes);
	return ZEN_HIP_OK;
}
int zen_hip_host_alloc_mapped(size_t bytes, int, void** host, void** dev)
{
	*host = *dev = std::calloc(bytes ? bytes : 1, 1);
	return *host ? ZEN_HIP_OK : ZEN_HIP_E_HIP;
}
int zen_hip_host_free(void* host)
{
	std::free(host);
	return ZEN_HIP_OK;
}

// ---- HPR / HPRRealtime: minimal ------------------------------------------------------------------
int zen_hip_hpr_create(float, size_t hop, float, unsigned, int, int, size_t, size_t, zen_hip_hpr_t* h)
{
	*h = new zen_hip_hpr{hop, std::vector<float>(hop, 0.0f)};
	return ZEN_HIP_OK;
}
int zen_hip_hpr_destroy(zen_hip_hpr_t h)
{
	delete h;
	return ZEN_HIP_OK;
}
int zen_hip_hpr_get_params(zen_hip_hpr_t h, zen_hip_hpr_params* p)
{
	*p = zen_hip_hpr_params{};
	p->hop = h->hop;
	p->nwin = 2 * h->hop;
	p->nfft = 4 * h->hop;
	p->stft_width = 9;
	p->l_harm = 9;
	p->l_perc = 9;
	p->lag = 4;
	p->time_len = 9;
	p->freq_len = 9;
	p->cola_factor = 1.0f;
	p->n_streams = 1;
	p->max_hops_per_chunk = 1;
	return ZEN_HIP_OK;
}
int zen_hip_hpr_use_sse_filter(zen_hip_hpr_t) { return ZEN_HIP_OK; }
int zen_hip_hpr_use_soft_mask(zen_hip_hpr_t) { return ZEN_HIP_OK; }
int zen_hip_hpr_reset_buffers(zen_hip_hpr_t) { return ZEN_HIP_OK; }
int zen_hip_hpr_set_resident(zen_hip_hpr_t, int) { return ZEN_HIP_OK; }
int zen_hip_hpr_process_next_hop(zen_hip_hpr_t h, const float* in_dev)
{
	h->last.assign(in_dev, in_dev + h->hop);
	return ZEN_HIP_OK;
}
int zen_hip_hpr_copy_output(zen_hip_hpr_t h, unsigned, float* out_dev)
{
	std::memcpy(out_dev, h->last.data(), h->hop * sizeof(float));
	return ZEN_HIP_OK;
}
int zen_hip_hpr_process(zen_hip_hpr_t h, const float* in_dev, size_t n_hops, size_t, float* harm, float* perc, float* resid,
                        size_t)
{
	for (float* out : {harm, perc, resid})
		if (out)
			std::memcpy(out, in_dev, n_hops * h->hop * sizeof(float));
	return ZEN_HIP_OK;
}
int zen_hip_hpr_process_host(zen_hip_hpr_t h, const float* in_host, size_t n_hops, float* harm, float* perc, float* resid)
{
	return zen_hip_hpr_process(h, in_host, n_hops, 0, harm, perc, resid, 0);
}

// ---- HPRIOffline ---------------------------------------------------------------------------------
int zen_hip_hpri_create(float, size_t hop_h, size_t hop_p, float, float, int, size_t, zen_hip_hpri_t* h)
{
	if (hop_p == 0 || hop_h % hop_p != 0)
		return ZEN_HIP_E_HOPS_NOT_DIVISIBLE;
	*h = new zen_hip_hpri{};
	return ZEN_HIP_OK;
}
int zen_hip_hpri_destroy(zen_hip_hpri_t h)
{
	delete h;
	return ZEN_HIP_OK;
}
int zen_hip_hpri_use_sse_filter(zen_hip_hpri_t) { return ZEN_HIP_OK; }
int zen_hip_hpri_use_soft_mask(zen_hip_hpri_t) { return ZEN_HIP_OK; }
int zen_hip_hpri_host_stats_get(zen_hip_hpri_t h, zen_hip_hpri_host_stats* out)
{
	*out = h->stats;
	return ZEN_HIP_OK;
}
int zen_hip_hpri_process(zen_hip_hpri_t h, const float* x, size_t n, float* harm, float* perc, float* resid)
{
	for (std::size_t i = 0; i < n; ++i) {
		const float hv = 0.5f * x[i];
		if (harm)
			harm[i] = hv;
		if (perc)
			perc[i] = x[i] - hv;
		if (resid)
			resid[i] = 0.0f;
	}
	h->stats = zen_hip_hpri_host_stats{};
	h->stats.n_ranges = 1;
	h->stats.range_samples = n;
	return ZEN_HIP_OK;
}
int zen_hip_hpri_process_sink(zen_hip_hpri_t h, const float* x, size_t n, int want_harm, int want_perc, zen_hip_hpri_sink_fn sink,
                              void* user)
{
	if (!sink || fake_zen_hip_range_samples == 0)
		return ZEN_HIP_E_BAD_ARG;
	std::thread th[2];
	const int want[2] = {want_harm, want_perc};
	for (int o = 0; o < 2; ++o)
		if (want[o])
			th[o] = std::thread(deliver, o, x, n, sink, user);
	for (std::thread& t : th)
		if (t.joinable())
			t.join();
	h->stats = zen_hip_hpri_host_stats{};
	h->stats.n_ranges = (n + fake_zen_hip_range_samples - 1) / fake_zen_hip_range_samples;
	h->stats.range_samples = fake_zen_hip_range_samples;
	return ZEN_HIP_OK;
}

} // extern "C"
