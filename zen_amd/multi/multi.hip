// multi.hip -- the C ABI of libzen_hip_multi.so (zen_hip_multi.h): interleaved multichannel audio through the engines' rows.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as the other add-ons are: the engines are a
// zen_hip_hpri_t with n_clips = channels and a causal zen_hip_hpr_t with n_streams = channels, memory comes from
// zen_hip_malloc, and the kernels of multi_kernels.hip stand in front (split) and behind (peak, join).
//
//   offline   split -> zen_hip_hpri_process_device -> [minmax init -> peak per stem] -> join per stem -> peaks
//   realtime  per slice of at most max_hops hops: split -> zen_hip_hpr_process -> join per output
// all on the handle's stream; the host calls put plain copies around the same sequence and wait once at the end.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "zen_hip_multi.h"

#include "../addon/addon_host.h"
#include "multi_kernels.h"

using namespace zen_addon;

struct zen_hip_multi_offline {
	int C = 0;
	zen_hip_hpri_t eng = nullptr;
	hipStream_t stream = nullptr;
	float* rows = nullptr;   // 3 sets (input, harmonic, percussive) of C rows, `stride` floats apart
	size_t stride = 0;       // a multiple of 4: every row starts on a 16-byte boundary
	float* minmax = nullptr; // [0..3] min / max of the two stems, [4..5] their peaks
	char* io = nullptr;      // the host calls' interleaved buffers: input, harmonic, percussive
	size_t io_each = 0;      // bytes of each, a multiple of 16
	unsigned long long calls = 0;
	DeviceTally mem;
};

struct zen_hip_multi_realtime {
	int C = 0;
	size_t hop = 0, max_hops = 0, stride = 0;
	unsigned flags = 0;
	zen_hip_hpr_t eng = nullptr;
	hipStream_t stream = nullptr;
	float* rows = nullptr; // 4 sets (input, harmonic, percussive, residual) of C rows of max_hops * hop floats
	char* io = nullptr;    // the host calls' interleaved buffers of a slice: input and the three outputs, as floats
	size_t io_each = 0;
	DeviceTally mem;
};

namespace {

size_t sample_bytes(int fmt) { return fmt == ZEN_HIP_MULTI_I16 ? 2 : 4; }
size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

int check_format(const char* who, int fmt, int channels)
{
	if (channels < 1 || channels > ZEN_HIP_MULTI_MAX_CHANNELS)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: channels must be 1..%d (got %d)", who, (int)ZEN_HIP_MULTI_MAX_CHANNELS, channels);
	if (fmt != ZEN_HIP_MULTI_I16 && fmt != ZEN_HIP_MULTI_F32)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the format must be ZEN_HIP_MULTI_I16 or ZEN_HIP_MULTI_F32 (got %d)", who, fmt);
	return ZEN_HIP_OK;
}

int check_mode(const char* who, int mode)
{
	if (mode != ZEN_HIP_MULTI_PEAK && mode != ZEN_HIP_MULTI_GAIN)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the mode must be ZEN_HIP_MULTI_PEAK or ZEN_HIP_MULTI_GAIN (got %d)", who, mode);
	return ZEN_HIP_OK;
}

// n_frames * channels samples of either format fit a size_t
int check_count(const char* who, size_t n_frames, int channels)
{
	if (n_frames > SIZE_MAX / 16 / (size_t)channels)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu frames of %d channels do not fit the address space", who, n_frames, channels);
	return ZEN_HIP_OK;
}

int check_rows(const char* who, const void* rows, size_t n_frames, size_t row_stride)
{
	if (!rows)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null rows", who);
	if ((uintptr_t)rows & 3)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if (row_stride < n_frames)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: row_stride %zu below the %zu frames of a row", who, row_stride, n_frames);
	return ZEN_HIP_OK;
}

int check_interleaved(const char* who, int fmt, const void* p)
{
	if (!p)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null interleaved buffer", who);
	if ((uintptr_t)p & (sample_bytes(fmt) - 1))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: interleaved samples need %zu-byte alignment", who, sample_bytes(fmt));
	return ZEN_HIP_OK;
}

// no two of the (up to four) buffers of `bytes` bytes overlap; null ones are absent
int check_apart(const char* who, const void* const* bufs, int count, size_t bytes)
{
	for (int i = 0; i < count; ++i)
		for (int j = i + 1; j < count; ++j) {
			const uintptr_t a = (uintptr_t)bufs[i], b = (uintptr_t)bufs[j];
			if (a && b && a < b + bytes && b < a + bytes)
				ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: buffers %d and %d overlap", who, i, j);
		}
	return ZEN_HIP_OK;
}

// ---- offline ------------------------------------------------------------------------------------------------------------

// the staging rows hold n_frames; growing waits for the stream, frees and allocates anew (nothing in them outlives a call)
int offline_rows(zen_hip_multi_offline* h, size_t n_frames)
{
	if (n_frames <= h->stride)
		return ZEN_HIP_OK;
	ZA_HIP(hipStreamSynchronize(h->stream));
	ZA_ZEN(zen_hip_free(h->rows));
	h->rows = nullptr;
	h->stride = 0;
	const size_t stride = round_up(n_frames, 4);
	ZA_TRY(counted_malloc(&h->mem, (void**)&h->rows, sizeof(float) * 3 * (size_t)h->C * stride, "zen_hip_malloc(staging rows)"));
	h->stride = stride;
	return ZEN_HIP_OK;
}

int offline_io(zen_hip_multi_offline* h, size_t bytes)
{
	if (bytes <= h->io_each)
		return ZEN_HIP_OK;
	ZA_HIP(hipStreamSynchronize(h->stream));
	ZA_ZEN(zen_hip_free(h->io));
	h->io = nullptr;
	h->io_each = 0;
	const size_t each = round_up(bytes, 16);
	ZA_TRY(counted_malloc(&h->mem, (void**)&h->io, 3 * each, "zen_hip_malloc(interleaved staging)"));
	h->io_each = each;
	return ZEN_HIP_OK;
}

int offline_check(const char* who, zen_hip_multi_offline_t h, int fmt, const void* in, size_t n_frames, const void* harm, const void* perc,
                  int mode)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	ZA_TRY(check_format(who, fmt, h->C));
	ZA_TRY(check_mode(who, mode));
	ZA_TRY(check_count(who, n_frames, h->C));
	if (n_frames == 0)
		return ZEN_HIP_OK;
	ZA_TRY(check_interleaved(who, fmt, in));
	if (harm)
		ZA_TRY(check_interleaved(who, fmt, harm));
	if (perc)
		ZA_TRY(check_interleaved(who, fmt, perc));
	const void* bufs[3] = {in, harm, perc};
	return check_apart(who, bufs, 3, n_frames * (size_t)h->C * sample_bytes(fmt));
}

// the arguments are checked and n_frames > 0
int offline_run(zen_hip_multi_offline* h, int fmt, const void* in, size_t n, void* harm, void* perc, int mode, float gain, float* peaks)
{
	ZA_TRY(offline_rows(h, n));
	const size_t st = h->stride, set = (size_t)h->C * st;
	float *x = h->rows, *yh = h->rows + set, *yp = h->rows + 2 * set;
	void* out[2] = {harm, perc};
	float* stem[2] = {yh, yp};
	const bool peak_mode = fmt == ZEN_HIP_MULTI_I16 && mode == ZEN_HIP_MULTI_PEAK;
	ZA_HIP(zen_multi::launch_split(fmt, in, h->C, n, x, st, h->stream));
	ZA_ZEN(zen_hip_hpri_process_device(h->eng, x, n, st, harm ? yh : nullptr, perc ? yp : nullptr, nullptr, st));
	unsigned active = 0;
	if (peak_mode) {
		ZA_HIP(zen_multi::launch_minmax_init(h->minmax, 2, h->stream));
		for (int o = 0; o < 2; ++o)
			if (out[o]) {
				ZA_HIP(zen_multi::launch_peak(stem[o], h->C, n, st, h->minmax + 2 * o, h->stream));
				active |= 1u << o;
			}
	}
	for (int o = 0; o < 2; ++o)
		if (out[o])
			ZA_HIP(zen_multi::launch_join(fmt, stem[o], h->C, n, st, mode, gain, h->minmax + 2 * o, out[o], h->stream));
	if (peaks)
		ZA_HIP(zen_multi::launch_peaks_of(h->minmax, 2, active, peaks, h->stream));
	h->calls += 1;
	return ZEN_HIP_OK;
}

// ---- realtime -----------------------------------------------------------------------------------------------------------

int realtime_check(const char* who, zen_hip_multi_realtime_t h, int fmt, const void* in, size_t n_hops, void* const* outs)
{
	static const unsigned flag[3] = {ZEN_HIP_OUTPUT_HARMONIC, ZEN_HIP_OUTPUT_PERCUSSIVE, ZEN_HIP_OUTPUT_RESIDUAL};
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	ZA_TRY(check_format(who, fmt, h->C));
	if (n_hops > SIZE_MAX / 16 / h->hop / (size_t)h->C)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu hops of %zu frames do not fit the address space", who, n_hops, h->hop);
	for (int o = 0; o < 3; ++o)
		if (outs[o] && !(h->flags & flag[o]))
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: output %d was not among the output_flags given to create", who, o);
	if (n_hops == 0)
		return ZEN_HIP_OK;
	ZA_TRY(check_interleaved(who, fmt, in));
	for (int o = 0; o < 3; ++o)
		if (outs[o])
			ZA_TRY(check_interleaved(who, fmt, outs[o]));
	const void* bufs[4] = {in, outs[0], outs[1], outs[2]};
	return check_apart(who, bufs, 4, n_hops * h->hop * (size_t)h->C * sample_bytes(fmt));
}

// one slice of cs <= max_hops hops on device pointers
int realtime_slice(zen_hip_multi_realtime* h, int fmt, const void* in, size_t cs, void* const* outs, float gain)
{
	const size_t n = cs * h->hop, st = h->stride, set = (size_t)h->C * st;
	float* y[3];
	for (int o = 0; o < 3; ++o)
		y[o] = outs[o] ? h->rows + (size_t)(1 + o) * set : nullptr;
	ZA_HIP(zen_multi::launch_split(fmt, in, h->C, n, h->rows, st, h->stream));
	ZA_ZEN(zen_hip_hpr_process(h->eng, h->rows, cs, st, y[0], y[1], y[2], st));
	for (int o = 0; o < 3; ++o)
		if (outs[o])
			ZA_HIP(zen_multi::launch_join(fmt, y[o], h->C, n, st, ZEN_HIP_MULTI_GAIN, gain, nullptr, outs[o], h->stream));
	return ZEN_HIP_OK;
}

} // namespace

extern "C" {

const char* zen_hip_multi_last_error(void) { return t_err; }
const char* zen_hip_multi_version(void) { return "zen_hip_multi 1 (gfx950)"; }

int zen_hip_multi_split(int fmt, const void* src_dev, int channels, size_t n_frames, float* dst_rows_dev, size_t row_stride, void* stream)
{
	ZA_TRY(check_format("multi_split", fmt, channels));
	ZA_TRY(check_count("multi_split", n_frames, channels));
	if (n_frames == 0)
		return ZEN_HIP_OK;
	ZA_TRY(check_interleaved("multi_split", fmt, src_dev));
	ZA_TRY(check_rows("multi_split", dst_rows_dev, n_frames, row_stride));
	ZA_HIP(zen_multi::launch_split(fmt, src_dev, channels, n_frames, dst_rows_dev, row_stride, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_multi_peak(const float* rows_dev, int channels, size_t n_frames, size_t row_stride, float* minmax_dev, void* stream)
{
	ZA_TRY(check_format("multi_peak", ZEN_HIP_MULTI_F32, channels));
	ZA_TRY(check_count("multi_peak", n_frames, channels));
	if (n_frames == 0)
		return ZEN_HIP_OK;
	ZA_TRY(check_rows("multi_peak", rows_dev, n_frames, row_stride));
	if (!minmax_dev || ((uintptr_t)minmax_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_peak: minmax_dev must be two floats in device memory");
	ZA_HIP(zen_multi::launch_peak(rows_dev, channels, n_frames, row_stride, minmax_dev, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

int zen_hip_multi_join(int fmt, const float* rows_dev, int channels, size_t n_frames, size_t row_stride, int mode, float gain,
                       const float* minmax_dev, void* dst_dev, void* stream)
{
	ZA_TRY(check_format("multi_join", fmt, channels));
	ZA_TRY(check_count("multi_join", n_frames, channels));
	if (fmt == ZEN_HIP_MULTI_I16)
		ZA_TRY(check_mode("multi_join", mode));
	if (n_frames == 0)
		return ZEN_HIP_OK;
	ZA_TRY(check_rows("multi_join", rows_dev, n_frames, row_stride));
	ZA_TRY(check_interleaved("multi_join", fmt, dst_dev));
	if (fmt == ZEN_HIP_MULTI_I16 && mode == ZEN_HIP_MULTI_PEAK && (!minmax_dev || ((uintptr_t)minmax_dev & 3)))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_join: ZEN_HIP_MULTI_PEAK needs minmax_dev, two floats in device memory");
	ZA_HIP(zen_multi::launch_join(fmt, rows_dev, channels, n_frames, row_stride, mode, gain, minmax_dev, dst_dev, (hipStream_t)stream));
	return ZEN_HIP_OK;
}

// ---- offline ------------------------------------------------------------------------------------------------------------

int zen_hip_multi_offline_create(float fs, size_t hop_h, size_t hop_p, float beta_h, float beta_p, int nocopybord, int channels,
                                 zen_hip_multi_offline_t* out)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_offline_create: null handle");
	ZA_TRY(check_format("multi_offline_create", ZEN_HIP_MULTI_F32, channels));
	zen_hip_multi_offline* h = new zen_hip_multi_offline;
	h->C = channels;
	auto build = [&]() -> int {
		ZA_ZEN(zen_hip_hpri_create(fs, hop_h, hop_p, beta_h, beta_p, nocopybord, (size_t)channels, &h->eng));
		ZA_TRY(counted_malloc(&h->mem, (void**)&h->minmax, sizeof(float) * 6, "zen_hip_malloc(minmax)"));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_multi_offline_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_multi_offline_destroy(zen_hip_multi_offline_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_hpri_destroy(h->eng);
	(void)zen_hip_free(h->rows);
	(void)zen_hip_free(h->minmax);
	(void)zen_hip_free(h->io);
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_multi_offline_use_sse_filter(zen_hip_multi_offline_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_offline_use_sse_filter: null handle");
	ZA_ZEN(zen_hip_hpri_use_sse_filter(h->eng));
	return ZEN_HIP_OK;
}

int zen_hip_multi_offline_use_soft_mask(zen_hip_multi_offline_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_offline_use_soft_mask: null handle");
	ZA_ZEN(zen_hip_hpri_use_soft_mask(h->eng));
	return ZEN_HIP_OK;
}

int zen_hip_multi_offline_set_stream(zen_hip_multi_offline_t h, void* stream)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_offline_set_stream: null handle");
	ZA_HIP(hipStreamSynchronize(h->stream));
	ZA_ZEN(zen_hip_hpri_set_stream(h->eng, stream));
	h->stream = (hipStream_t)stream;
	return ZEN_HIP_OK;
}

int zen_hip_multi_offline_device(zen_hip_multi_offline_t h, int fmt, const void* in_dev, size_t n_frames, void* harm_dev, void* perc_dev,
                                 int mode, float gain, float* peaks_dev)
{
	ZA_TRY(offline_check("multi_offline_device", h, fmt, in_dev, n_frames, harm_dev, perc_dev, mode));
	if ((uintptr_t)peaks_dev & 3)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_offline_device: float pointers need 4-byte alignment");
	if (n_frames == 0)
		return ZEN_HIP_OK;
	const void* bufs[3] = {in_dev, harm_dev, perc_dev};
	const size_t bytes = n_frames * (size_t)h->C * sample_bytes(fmt);
	for (const void* b : bufs) {
		const uintptr_t a = (uintptr_t)b, p = (uintptr_t)peaks_dev;
		if (a && p && a < p + 2 * sizeof(float) && p < a + bytes)
			ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_offline_device: peaks_dev overlaps a buffer of frames");
	}
	return offline_run(h, fmt, in_dev, n_frames, harm_dev, perc_dev, mode, gain, peaks_dev);
}

int zen_hip_multi_offline_host(zen_hip_multi_offline_t h, int fmt, const void* in_host, size_t n_frames, void* harm_host, void* perc_host,
                               int mode, float gain, float peaks[2])
{
	ZA_TRY(offline_check("multi_offline_host", h, fmt, in_host, n_frames, harm_host, perc_host, mode));
	if (peaks)
		peaks[0] = peaks[1] = 0.0f;
	if (n_frames == 0)
		return ZEN_HIP_OK;
	const size_t bytes = n_frames * (size_t)h->C * sample_bytes(fmt);
	ZA_TRY(offline_io(h, bytes));
	char *d_in = h->io, *d_h = harm_host ? h->io + h->io_each : nullptr, *d_p = perc_host ? h->io + 2 * h->io_each : nullptr;
	auto run = [&]() -> int {
		ZA_HIP(hipMemcpyAsync(d_in, in_host, bytes, hipMemcpyHostToDevice, h->stream));
		ZA_TRY(offline_run(h, fmt, d_in, n_frames, d_h, d_p, mode, gain, peaks ? h->minmax + 4 : nullptr));
		if (d_h)
			ZA_HIP(hipMemcpyAsync(harm_host, d_h, bytes, hipMemcpyDeviceToHost, h->stream));
		if (d_p)
			ZA_HIP(hipMemcpyAsync(perc_host, d_p, bytes, hipMemcpyDeviceToHost, h->stream));
		if (peaks)
			ZA_HIP(hipMemcpyAsync(peaks, h->minmax + 4, sizeof(float) * 2, hipMemcpyDeviceToHost, h->stream));
		return ZEN_HIP_OK;
	};
	const int rc = run();
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_multi_stats(zen_hip_multi_offline_t h, zen_hip_multi_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_stats: null argument");
	out->calls = h->calls;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	out->row_stride = h->stride;
	return ZEN_HIP_OK;
}

// ---- realtime -----------------------------------------------------------------------------------------------------------

int zen_hip_multi_realtime_create(float fs, size_t hop, float beta, unsigned output_flags, int channels, size_t max_hops,
                                  zen_hip_multi_realtime_t* out)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_realtime_create: null handle");
	ZA_TRY(check_format("multi_realtime_create", ZEN_HIP_MULTI_F32, channels));
	if (max_hops == 0)
		max_hops = 256;
	if (hop == 0 || hop > ((size_t)1 << 20) || max_hops > ((size_t)1 << 20))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_realtime_create: hop %zu or max_hops %zu outside 1..2^20", hop, max_hops);
	zen_hip_multi_realtime* h = new zen_hip_multi_realtime;
	h->C = channels;
	h->hop = hop;
	h->max_hops = max_hops;
	h->flags = output_flags;
	auto build = [&]() -> int {
		ZA_ZEN(zen_hip_hpr_create(fs, hop, beta, output_flags, ZEN_HIP_TIME_CAUSAL, 1, (size_t)channels, max_hops, &h->eng));
		h->stride = round_up(max_hops * hop, 4);
		h->io_each = round_up(h->stride * (size_t)channels * sizeof(float), 16);
		ZA_TRY(counted_malloc(&h->mem, (void**)&h->rows, sizeof(float) * 4 * (size_t)channels * h->stride, "zen_hip_malloc(staging rows)"));
		ZA_TRY(counted_malloc(&h->mem, (void**)&h->io, 4 * h->io_each, "zen_hip_malloc(interleaved staging)"));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_multi_realtime_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_multi_realtime_destroy(zen_hip_multi_realtime_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	zen_hip_hpr_destroy(h->eng);
	(void)zen_hip_free(h->rows);
	(void)zen_hip_free(h->io);
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_multi_realtime_use_sse_filter(zen_hip_multi_realtime_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_realtime_use_sse_filter: null handle");
	ZA_ZEN(zen_hip_hpr_use_sse_filter(h->eng));
	return ZEN_HIP_OK;
}

int zen_hip_multi_realtime_use_soft_mask(zen_hip_multi_realtime_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_realtime_use_soft_mask: null handle");
	ZA_ZEN(zen_hip_hpr_use_soft_mask(h->eng));
	return ZEN_HIP_OK;
}

int zen_hip_multi_realtime_reset(zen_hip_multi_realtime_t h)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_realtime_reset: null handle");
	ZA_ZEN(zen_hip_hpr_reset_buffers(h->eng));
	return ZEN_HIP_OK;
}

int zen_hip_multi_realtime_set_stream(zen_hip_multi_realtime_t h, void* stream)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "multi_realtime_set_stream: null handle");
	ZA_HIP(hipStreamSynchronize(h->stream));
	ZA_ZEN(zen_hip_hpr_set_stream(h->eng, stream));
	h->stream = (hipStream_t)stream;
	return ZEN_HIP_OK;
}

int zen_hip_multi_realtime_device(zen_hip_multi_realtime_t h, int fmt, const void* in_dev, size_t n_hops, void* harm_dev, void* perc_dev,
                                  void* resid_dev, float gain)
{
	void* const outs[3] = {harm_dev, perc_dev, resid_dev};
	ZA_TRY(realtime_check("multi_realtime_device", h, fmt, in_dev, n_hops, outs));
	const size_t hop_bytes = h->hop * (size_t)h->C * sample_bytes(fmt);
	for (size_t c0 = 0; c0 < n_hops; c0 += h->max_hops) {
		const size_t cs = n_hops - c0 < h->max_hops ? n_hops - c0 : h->max_hops;
		void* o[3];
		for (int k = 0; k < 3; ++k)
			o[k] = outs[k] ? (char*)outs[k] + c0 * hop_bytes : nullptr;
		ZA_TRY(realtime_slice(h, fmt, (const char*)in_dev + c0 * hop_bytes, cs, o, gain));
	}
	return ZEN_HIP_OK;
}

int zen_hip_multi_realtime_host(zen_hip_multi_realtime_t h, int fmt, const void* in_host, size_t n_hops, void* harm_host, void* perc_host,
                                void* resid_host, float gain)
{
	void* const outs[3] = {harm_host, perc_host, resid_host};
	ZA_TRY(realtime_check("multi_realtime_host", h, fmt, in_host, n_hops, outs));
	const size_t hop_bytes = h->hop * (size_t)h->C * sample_bytes(fmt);
	auto run = [&]() -> int {
		for (size_t c0 = 0; c0 < n_hops; c0 += h->max_hops) {
			const size_t cs = n_hops - c0 < h->max_hops ? n_hops - c0 : h->max_hops;
			// Up: the frames of the slice.  Down: its outputs.  The next slice overwrites the staging: stream order keeps
			// that behind these copies.
			void* d[3];
			for (int k = 0; k < 3; ++k)
				d[k] = outs[k] ? h->io + (size_t)(1 + k) * h->io_each : nullptr;
			ZA_HIP(hipMemcpyAsync(h->io, (const char*)in_host + c0 * hop_bytes, cs * hop_bytes, hipMemcpyHostToDevice, h->stream));
			ZA_TRY(realtime_slice(h, fmt, h->io, cs, d, gain));
			for (int k = 0; k < 3; ++k)
				if (outs[k])
					ZA_HIP(hipMemcpyAsync((char*)outs[k] + c0 * hop_bytes, d[k], cs * hop_bytes, hipMemcpyDeviceToHost, h->stream));
		}
		return ZEN_HIP_OK;
	};
	const int rc = run();
	const hipError_t es = hipStreamSynchronize(h->stream);
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

} // extern "C"
