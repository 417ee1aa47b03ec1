// resample.hip -- the C ABI of libzen_hip_resample.so (zen_hip_resample.h): band-limited rate conversion of rows in device
// memory.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as tsm.hip is: memory comes from zen_hip_malloc,
// and the two kernels of resample_kernels.hip do the rest.  The integer geometry and the table are host arithmetic, handed
// out without a device; create uploads the table and, on the polyphase route, expands the num coefficient rows once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "zen_hip_resample.h"

#include "../addon/addon_host.h"
#include "resample_kernels.h"

using namespace zen_addon;

namespace {

enum { K_EXPAND = 0, K_FIR, K_COUNT };
static_assert(K_COUNT == ZEN_HIP_RESAMPLE_KERNELS, "the header names the kernels");
static_assert(ZEN_HIP_RESAMPLE_TILE == zen_resample::TILE && ZEN_HIP_RESAMPLE_PHASES == zen_resample::PHASES &&
              ZEN_HIP_RESAMPLE_MAX_TAPS == zen_resample::MAX_TAPS, "the header states the kernels' constants");

typedef unsigned long long u64;
constexpr u64 MAX_TERM = 1ull << 20, MAX_TOTAL = 1ull << 40;

struct Quality {
	int Z;
	double roll, beta;
};
const Quality QUALITIES[] = {{8, 0.85, 7.0}, {16, 0.91, 10.0}, {32, 0.9476, 14.77}};

struct Geometry { // of a checked ratio
	u64 num, den; // reduced
	int Z, W, T, Tp;
	double roll, beta;
	bool poly_rule;
};

u64 gcd(u64 a, u64 b)
{
	while (b) {
		const u64 t = a % b;
		a = b;
		b = t;
	}
	return a;
}

int geometry_of(const char* who, u64 num, u64 den, int quality, Geometry* g)
{
	if (num == 0 || den == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a ratio of %llu / %llu", who, num, den);
	const u64 d = gcd(num, den);
	num /= d;
	den /= d;
	if (num > MAX_TERM || den > MAX_TERM)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the reduced ratio %llu / %llu has a term above 2^20", who, num, den);
	if (num > 4 * den || den > 4 * num)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the ratio %llu / %llu is outside 1/4..4", who, num, den);
	const Quality* q = nullptr;
	for (const Quality& c : QUALITIES)
		if (c.Z == quality)
			q = &c;
	if (!q)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: quality %d is none of 8, 16, 32", who, quality);
	g->num = num;
	g->den = den;
	g->Z = q->Z;
	g->roll = q->roll;
	g->beta = q->beta;
	g->W = num >= den ? q->Z : (int)(((u64)q->Z * den + num - 1) / num);
	g->T = 2 * g->W;
	g->Tp = (g->T + 7) / 8 * 8;
	g->poly_rule = num <= (u64)ZEN_HIP_RESAMPLE_MAX_POLY;
	return ZEN_HIP_OK;
}

u64 outputs_of(const Geometry& g, u64 n_total) { return (n_total * g.num + g.den - 1) / g.den; }

double bessel_i0(double x)
{
	const double hx = x / 2.0;
	double term = 1.0, sum = 1.0;
	for (int k = 1; k <= 48; ++k) {
		const double q = hx / (double)k;
		term = term * (q * q);
		sum = sum + term;
	}
	return sum;
}

// h[p][j], the contract's operations in the contract's order
float table_at(const Geometry& g, double c, double i0_beta, int p, int j)
{
	const double d = (double)(j - g.W + 1) - (double)p / (double)ZEN_HIP_RESAMPLE_PHASES;
	const double v = c * d;
	double s = 1.0;
	if (v != 0.0) {
		const double pv = M_PI * v;
		s = sin(pv) / pv;
	}
	const double u = d / (double)g.W;
	double r = 1.0 - u * u;
	if (!(r > 0.0))
		r = 0.0;
	const double w = bessel_i0(g.beta * sqrt(r)) / i0_beta;
	return (float)((c * s) * w);
}

// rows of `stride` floats, the floats behind tap T - 1 zero
void fill_table(const Geometry& g, float* out, int stride)
{
	const double ratio = (double)g.num / (double)g.den;
	const double c = (ratio < 1.0 ? ratio : 1.0) * g.roll;
	const double i0_beta = bessel_i0(g.beta);
	for (int p = 0; p <= ZEN_HIP_RESAMPLE_PHASES; ++p)
		for (int j = 0; j < stride; ++j)
			out[(size_t)p * stride + j] = j < g.T ? table_at(g, c, i0_beta, p, j) : 0.0f;
}

void span_of(const Geometry& g, u64 n_total, u64 out_first, u64 out_count, u64* in_first, u64* in_count)
{
	const u64 i_first = out_first * g.den / g.num, i_last = (out_first + out_count - 1) * g.den / g.num;
	const u64 lo = i_first + 1 > (u64)g.W ? i_first + 1 - (u64)g.W : 0;
	const u64 hi = i_last + (u64)g.W < n_total - 1 ? i_last + (u64)g.W : n_total - 1;
	*in_first = lo;
	*in_count = hi - lo + 1;
}

bool poly_switched_off()
{
	const char* e = getenv("ZEN_HIP_RESAMPLE");
	return e && strstr(e, "poly=0");
}

} // namespace

struct zen_hip_resample : Handle<K_COUNT> {
	Geometry g = {};
	bool poly = false;
	float* table = nullptr; // (L + 1) rows of Tp floats
	float* rows = nullptr;  // poly: num rows of Tp floats
	u64 calls = 0, n_rows = 0, outputs = 0, poly_calls = 0, interp_calls = 0;
};

namespace {

// the arguments of a device call, checked against the contract; nothing is touched
int check_run(const char* who, zen_hip_resample_t h, const float* in, size_t in_stride, u64 in_first, size_t in_count, u64 n_total, u64 out_first,
              size_t out_count, const float* out, size_t out_stride, size_t n_rows)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (!in || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null pointer", who);
	if (((uintptr_t)in & 3) || ((uintptr_t)out & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment", who);
	if (n_total == 0 || n_total > MAX_TOTAL)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a row of %llu samples, outside 1..2^40", who, n_total);
	if (n_rows == 0 || n_rows > (size_t)ZEN_HIP_RESAMPLE_MAX_ROWS)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu rows, outside 1..%d", who, n_rows, (int)ZEN_HIP_RESAMPLE_MAX_ROWS);
	const u64 n_out = outputs_of(h->g, n_total);
	if (out_count == 0 || out_first >= n_out || (u64)out_count > n_out - out_first)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: outputs %llu + %zu of a row that has %llu", who, out_first, out_count, n_out);
	if (in_count == 0 || in_first >= n_total || (u64)in_count > n_total - in_first)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a window %llu + %zu of a row of %llu samples", who, in_first, in_count, n_total);
	u64 need_first, need_count;
	span_of(h->g, n_total, out_first, out_count, &need_first, &need_count);
	if (in_first > need_first || in_first + in_count < need_first + need_count)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the window %llu + %zu is short of the span %llu + %llu of the outputs", who, in_first, in_count, need_first,
		        need_count);
	if (in_stride < in_count)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: in_stride %zu below the %zu samples of a window", who, in_stride, in_count);
	if (out_stride < out_count)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: out_stride %zu below the %zu outputs of a row", who, out_stride, out_count);
	if (((u64)out_count + ZEN_HIP_RESAMPLE_TILE - 1) / ZEN_HIP_RESAMPLE_TILE > 0x7FFFFFFFull)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %zu outputs per row are more than 2^31 - 1 tiles", who, out_count);
	const uintptr_t a0 = (uintptr_t)in, a1 = a0 + sizeof(float) * ((n_rows - 1) * in_stride + in_count);
	const uintptr_t b0 = (uintptr_t)out, b1 = b0 + sizeof(float) * ((n_rows - 1) * out_stride + out_count);
	if (a0 < b1 && b0 < a1)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: the input and the output rows overlap", who);
	return ZEN_HIP_OK;
}

// the arguments are checked
int run(zen_hip_resample* h, const float* in, size_t in_stride, u64 in_first, size_t in_count, u64 n_total, u64 out_first, size_t out_count,
        float* out, size_t out_stride, size_t n_rows)
{
	const Geometry& g = h->g;
	zen_resample::FirArgs a = {};
	a.in = in;
	a.out = out;
	a.coef = h->poly ? h->rows : h->table;
	a.in_stride = in_stride;
	a.out_stride = out_stride;
	a.in_first = in_first;
	a.in_count = in_count;
	a.n_total = n_total;
	a.out_first = out_first;
	a.out_count = out_count;
	a.num = (uint32_t)g.num;
	a.den = (uint32_t)g.den;
	a.tiles = (uint32_t)(((u64)out_count + zen_resample::TILE - 1) / zen_resample::TILE);
	a.n_rows = (uint32_t)n_rows;
	a.W = g.W;
	a.Tp = g.Tp;
	a.poly = h->poly;
	auto kt = h->prof.on_stream(h->stream);
	ZA_TRY(kt.begin(K_FIR, sizeof(float) * n_rows * ((u64)in_count + out_count)));
	ZA_HIP(zen_resample::launch_fir(a, h->stream));
	ZA_TRY(kt.end());
	h->calls += 1;
	h->n_rows += n_rows;
	h->outputs += (u64)n_rows * out_count;
	(h->poly ? h->poly_calls : h->interp_calls) += 1;
	return ZEN_HIP_OK;
}

} // namespace

extern "C" {

const char* zen_hip_resample_last_error(void) { return t_err; }
const char* zen_hip_resample_version(void) { return "zen_hip_resample 1 (gfx950)"; }

int zen_hip_resample_create(unsigned long long num, unsigned long long den, int quality, zen_hip_resample_t* out)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "resample_create: null handle");
	Geometry g;
	ZA_TRY(geometry_of("resample_create", num, den, quality, &g));
	zen_hip_resample* h = new zen_hip_resample;
	h->g = g;
	h->poly = g.poly_rule && !poly_switched_off();
	auto build = [&]() -> int {
		std::vector<float> tab((size_t)(ZEN_HIP_RESAMPLE_PHASES + 1) * g.Tp);
		fill_table(g, tab.data(), g.Tp);
		ZA_TRY(counted_malloc(&h->mem, (void**)&h->table, sizeof(float) * tab.size(), "zen_hip_malloc(table)"));
		if (h->poly)
			ZA_TRY(counted_malloc(&h->mem, (void**)&h->rows, sizeof(float) * g.num * g.Tp, "zen_hip_malloc(polyphase rows)"));
		ZA_ZEN(zen_hip_memcpy_h2d(h->table, tab.data(), sizeof(float) * tab.size()));
		if (h->poly) {
			// timed whatever the profile's switch says: there is no handle to switch it on before create
			zen_resample::ExpandArgs a = {h->table, h->rows, (uint32_t)g.num, g.Tp};
			h->prof.on = true;
			auto kt = h->prof.on_stream(h->stream);
			int rc = kt.begin(K_EXPAND, sizeof(float) * g.num * g.Tp * 3);
			if (rc == ZEN_HIP_OK) {
				const hipError_t e = zen_resample::launch_expand(a, h->stream);
				if (e != hipSuccess) {
					set_err("resample_create: launch_expand failed: %s", hipGetErrorString(e));
					rc = ZEN_HIP_E_HIP;
				}
			}
			if (rc == ZEN_HIP_OK)
				rc = kt.end();
			h->prof.on = false;
			ZA_TRY(rc);
		}
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_resample_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_resample_destroy(zen_hip_resample_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	(void)hipStreamSynchronize(h->stream);
	h->release({h->table, h->rows});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_resample_set_stream(zen_hip_resample_t h, void* stream) { return set_stream(h, stream, "resample"); }

int zen_hip_resample_run_device(zen_hip_resample_t h, const float* in_dev, size_t in_stride, unsigned long long in_first, size_t in_count,
                                unsigned long long n_total, unsigned long long out_first, size_t out_count, float* out_dev, size_t out_stride,
                                size_t n_rows)
{
	ZA_TRY(check_run("resample_run_device", h, in_dev, in_stride, in_first, in_count, n_total, out_first, out_count, out_dev, out_stride, n_rows));
	return run(h, in_dev, in_stride, in_first, in_count, n_total, out_first, out_count, out_dev, out_stride, n_rows);
}

int zen_hip_resample_run_host(zen_hip_resample_t h, const float* in_host, size_t in_stride, size_t n, float* out_host, size_t out_stride,
                              size_t n_rows)
{
	const char* who = "resample_run_host";
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (n == 0 || (u64)n > MAX_TOTAL)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a row of %zu samples, outside 1..2^40", who, n);
	const size_t n_out = (size_t)outputs_of(h->g, n);
	ZA_TRY(check_run(who, h, in_host, in_stride, 0, n, n, 0, n_out, out_host, out_stride, n_rows));
	// the device rows lie tight and live as long as the call
	float *d_in = nullptr, *d_out = nullptr;
	int rc = ZEN_HIP_OK;
	if (zen_hip_malloc((void**)&d_in, sizeof(float) * n * n_rows) != ZEN_HIP_OK || zen_hip_malloc((void**)&d_out, sizeof(float) * n_out * n_rows) != ZEN_HIP_OK) {
		set_err("%s: zen_hip_malloc: %s", who, zen_hip_last_error());
		rc = ZEN_HIP_E_HIP;
	}
	if (rc == ZEN_HIP_OK)
		rc = h->copy_rows_1d(d_in, n, in_host, in_stride, n, n_rows, hipMemcpyHostToDevice);
	if (rc == ZEN_HIP_OK)
		rc = run(h, d_in, n, 0, n, n, 0, n_out, d_out, n_out, n_rows);
	if (rc == ZEN_HIP_OK)
		rc = h->copy_rows_1d(out_host, out_stride, d_out, n_out, n_out, n_rows, hipMemcpyDeviceToHost);
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	(void)zen_hip_free(d_in);
	(void)zen_hip_free(d_out);
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_resample_stats(zen_hip_resample_t h, zen_hip_resample_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "resample_stats: null argument");
	out->calls = h->calls;
	out->rows = h->n_rows;
	out->outputs = h->outputs;
	out->poly_calls = h->poly_calls;
	out->interp_calls = h->interp_calls;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_resample_profile(zen_hip_resample_t h, int enable) { return profile(h, enable); }

int zen_hip_resample_profile_get(zen_hip_resample_t h, double ms[ZEN_HIP_RESAMPLE_KERNELS], unsigned long long bytes[ZEN_HIP_RESAMPLE_KERNELS],
                                 unsigned long long launches[ZEN_HIP_RESAMPLE_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "resample");
}

int zen_hip_resample_n_out(unsigned long long num, unsigned long long den, unsigned long long n_total, unsigned long long* n_out)
{
	const char* who = "resample_n_out";
	if (!n_out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	Geometry g;
	ZA_TRY(geometry_of(who, num, den, 16, &g));
	if (n_total == 0 || n_total > MAX_TOTAL)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a row of %llu samples, outside 1..2^40", who, n_total);
	*n_out = outputs_of(g, n_total);
	return ZEN_HIP_OK;
}

int zen_hip_resample_span(unsigned long long num, unsigned long long den, int quality, unsigned long long n_total, unsigned long long out_first,
                          unsigned long long out_count, unsigned long long* in_first, unsigned long long* in_count)
{
	const char* who = "resample_span";
	if (!in_first || !in_count)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	Geometry g;
	ZA_TRY(geometry_of(who, num, den, quality, &g));
	if (n_total == 0 || n_total > MAX_TOTAL)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a row of %llu samples, outside 1..2^40", who, n_total);
	const u64 n_out = outputs_of(g, n_total);
	if (out_count == 0 || out_first >= n_out || out_count > n_out - out_first)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: outputs %llu + %llu of a row that has %llu", who, out_first, out_count, n_out);
	span_of(g, n_total, out_first, out_count, in_first, in_count);
	return ZEN_HIP_OK;
}

int zen_hip_resample_geometry(unsigned long long num, unsigned long long den, int quality, size_t* W, size_t* T, int* route)
{
	const char* who = "resample_geometry";
	if (!W || !T || !route)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	Geometry g;
	ZA_TRY(geometry_of(who, num, den, quality, &g));
	*W = (size_t)g.W;
	*T = (size_t)g.T;
	*route = g.poly_rule ? ZEN_HIP_RESAMPLE_ROUTE_POLY : ZEN_HIP_RESAMPLE_ROUTE_INTERP;
	return ZEN_HIP_OK;
}

int zen_hip_resample_table(unsigned long long num, unsigned long long den, int quality, float* out, size_t cap)
{
	const char* who = "resample_table";
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null output", who);
	Geometry g;
	ZA_TRY(geometry_of(who, num, den, quality, &g));
	const size_t len = (size_t)(ZEN_HIP_RESAMPLE_PHASES + 1) * g.T;
	if (cap < len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: room for %zu floats, the table has %zu", who, cap, len);
	fill_table(g, out, g.T);
	return ZEN_HIP_OK;
}

int zen_hip_resample_ratio_for_shift(double semitones, unsigned long long* num, unsigned long long* den)
{
	const char* who = "resample_ratio_for_shift";
	if (!num || !den)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null argument", who);
	if (!std::isfinite(semitones) || fabs(semitones) > 24.0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a shift of %g semitones, outside -24..24", who, semitones);
	const u64 n = (u64)llround(65536.0 / pow(2.0, semitones / 12.0)), d = 65536, g = gcd(n, d);
	*num = n / g;
	*den = d / g;
	return ZEN_HIP_OK;
}

} // extern "C"
