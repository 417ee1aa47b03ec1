// cqt.hip -- the C ABI of libzen_hip_cqt.so (zen_hip_cqt.h): a sliced constant-Q transform and the harmonic / percussive /
// residual separation in its domain, on clips in device memory.
//
// Written on top of the public C ABI of libzen_hip.so (include/zen_hip.h), as repet.hip is: the transforms are
// zen_hip_fft_exec_batched (one Ls-point handle for the slices, one M-point handle for the bands), the medians are
// zen_hip_mfilt_run, memory comes from zen_hip_malloc, and the kernels of cqt_kernels.hip stand between them.
//
// One separate call (n_clips clips of n samples, ns slices each):
//   slice, slice_fft, fold, band_ifft     every clip at once: the one copy of the coefficients
//   per clip: overlap -> V, median_time -> H, median_freq -> P;
//   per clip and stem asked for: runs of slices through mask -> band_fft -> gather (the per-stem scratch holds one run),
//   then slice_ifft over the clip's rows (the slice spectra of step 1 are spent by then) and overlap_add -> the caller's row
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "zen_hip_cqt.h"

#include "../addon/addon_host.h"
#include "cqt_kernels.h"

using namespace zen_addon;

namespace {

enum { K_SLICE = 0, K_SLICE_FFT, K_FOLD, K_BAND_IFFT, K_OVERLAP, K_MEDIAN_TIME, K_MEDIAN_FREQ, K_MASK, K_BAND_FFT, K_GATHER, K_SLICE_IFFT, K_OLA, K_COUNT };
static_assert(K_COUNT == ZEN_HIP_CQT_KERNELS, "the header names the kernels");

constexpr int WMIN = 4;
constexpr size_t RUN_BYTES = (size_t)32 << 20; // the per-stem scratch: as many slices as fit, one at the least


// The host side of the contract: the centres, M and the tables, all from doubles (libm cos and pow), rounded once.
struct Plan {
	double fs = 0;
	size_t Ls = 0, N = 0, nb = 0, M = 0;
	std::vector<int> p, kb;
	std::vector<float> gL, gU, gdL, gdU, h, s;
};

int plan_centres(const char* who, float fs, size_t Ls, int B, double fmin, Plan* pl)
{
	if (!is_pow2(Ls) || Ls < 64 || Ls > 32768)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: slice %zu is not a power of two in 64..32768", who, Ls);
	if (!(fs > 0.0f) || !std::isfinite(fs))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: sample rate %g", who, (double)fs);
	if (B < 1 || B > ZEN_HIP_CQT_MAX_BANDS_PER_OCTAVE)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %d bands per octave, outside 1..%d", who, B, (int)ZEN_HIP_CQT_MAX_BANDS_PER_OCTAVE);
	if (!(fmin > 0.0) || !std::isfinite(fmin))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: lowest band at %g Hz", who, fmin);
	pl->fs = (double)fs;
	pl->Ls = Ls;
	pl->N = Ls / 2;
	const double N = (double)pl->N, r = pow(2.0, 1.0 / (double)B);
	double first = floor(fmin * (double)Ls / (double)fs + 0.5);
	if (first < (double)WMIN)
		first = (double)WMIN;
	pl->p.assign(1, 0);
	if (first <= N - WMIN) {
		pl->p.push_back((int)first);
		for (;;) {
			const int last = pl->p.back();
			int nx = (int)floor((double)last * r + 0.5);
			if (nx < last + WMIN)
				nx = last + WMIN;
			if (nx > (int)pl->N - WMIN)
				break;
			pl->p.push_back(nx);
		}
	}
	pl->p.push_back((int)pl->N);
	pl->nb = pl->p.size();
	if (pl->nb < 3)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: a lowest band at %g Hz leaves %zu bands below %g Hz, fewer than 3", who, fmin, pl->nb, (double)fs / 2);
	int width = 0;
	for (size_t k = 0; k < pl->nb; ++k) {
		const int w = pl->p[k + 1 < pl->nb ? k + 1 : pl->nb - 1] - pl->p[k ? k - 1 : 0] - 1;
		width = w > width ? w : width;
	}
	pl->M = 32;
	while (pl->M < (size_t)width)
		pl->M *= 2;
	return ZEN_HIP_OK;
}

void plan_tables(Plan* pl)
{
	const size_t N = pl->N, Ls = pl->Ls, nb = pl->nb;
	pl->kb.assign(N + 1, 0);
	pl->gL.assign(N + 1, 0.f);
	pl->gU.assign(N + 1, 0.f);
	pl->gdL.assign(N + 1, 0.f);
	pl->gdU.assign(N + 1, 0.f);
	for (size_t k = 0; k + 1 < nb; ++k) {
		const int a = pl->p[k], c = pl->p[k + 1];
		for (int b = a; b < c; ++b) {
			const double w = cos(M_PI * (double)(b - a) / (double)(c - a));
			pl->kb[b] = (int)k;
			pl->gL[b] = (float)(0.5 + 0.5 * w); // band k falls
			pl->gU[b] = (float)(0.5 - 0.5 * w); // band k + 1 rises
		}
	}
	pl->kb[N] = (int)nb - 1;
	pl->gL[N] = 1.0f;
	for (size_t b = 0; b <= N; ++b) {
		const double l = (double)pl->gL[b], u = (double)pl->gU[b], den = (double)pl->M * (l * l + u * u);
		pl->gdL[b] = (float)(l / den);
		pl->gdU[b] = (float)(u / den);
	}
	std::vector<double> h(Ls);
	for (size_t i = 0; i < Ls; ++i)
		h[i] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)Ls);
	pl->h.resize(Ls);
	pl->s.resize(Ls);
	for (size_t i = 0; i < Ls; ++i) {
		const double o = h[(i + N) % Ls];
		pl->h[i] = (float)h[i];
		pl->s[i] = (float)((h[i] / (h[i] * h[i] + o * o)) / (double)Ls);
	}
}

} // namespace

struct zen_hip_cqt : Handle<K_COUNT> {
	Plan pl;
	size_t C = 0, n = 0, ns = 0, T = 0, run = 0;
	float beta = 2.0f;
	int soft = 0, lh = 0, lp = 0, B = 0;
	zen_hip_fft_t fft_slice = nullptr, fft_band = nullptr;
	zen_hip_mfilt_t med_time = nullptr, med_freq = nullptr;
	float* rows = nullptr;    // C * ns rows of Ls complex values: the slice spectra, later Y_q of the stem at hand
	float* coef = nullptr;    // C * ns * nb rows of M complex values: the one copy of the coefficients
	float* scratch = nullptr; // run * nb rows of M complex values: the masked coefficients of the stem at hand
	float *v = nullptr, *hm = nullptr, *pm = nullptr; // T rows of nb floats: the clip at hand
	float* ftab = nullptr;    // gL, gU, gdL, gdU (N + 1 each), h, s (Ls each)
	int* itab = nullptr;      // kb (N + 1), the centres (nb)
	float* stage_in = nullptr; // the host call's device rows: C rows of n samples
	float* stage_out[3] = {nullptr, nullptr, nullptr};
	zen_cqt::Tables tab = {};
	unsigned long long calls = 0, clips = 0;
};

namespace {

void default_lengths(const zen_hip_cqt* h, int* lh, int* lp)
{
	double l = floor(0.2 * h->pl.fs * (double)h->pl.M / (double)h->pl.Ls);
	if (l > (double)h->T)
		l = (double)h->T;
	int a = (int)l;
	a += 1 - a % 2;
	*lh = (size_t)a > h->T ? (int)h->T : a;
	const int b = h->B + (1 - h->B % 2);
	*lp = (size_t)b > h->pl.nb ? (int)h->pl.nb : b;
}

// the two median handles for (lh, lp); the handle keeps its former pair where this fails
int make_filters(zen_hip_cqt* h, int lh, int lp)
{
	zen_hip_mfilt_t mt = nullptr, mf = nullptr;
	ZA_ZEN(zen_hip_mfilt_create((int)h->T, (int)h->pl.nb, lh, ZEN_HIP_TIME_ANTICAUSAL, 1, &mt));
	const int rc = zen_hip_mfilt_create((int)h->T, (int)h->pl.nb, lp, ZEN_HIP_FREQUENCY, 1, &mf);
	if (rc != ZEN_HIP_OK) {
		set_err("zen_hip_mfilt_create: %s", zen_hip_last_error());
		zen_hip_mfilt_destroy(mt);
		return rc;
	}
	(void)zen_hip_mfilt_assume_nonneg(mt, 1); // V is a matrix of magnitudes
	(void)zen_hip_mfilt_assume_nonneg(mf, 1);
	zen_hip_mfilt_destroy(h->med_time);
	zen_hip_mfilt_destroy(h->med_freq);
	h->med_time = mt;
	h->med_freq = mf;
	h->lh = lh;
	h->lp = lp;
	return ZEN_HIP_OK;
}

size_t coef_floats(const zen_hip_cqt* h) { return h->ns * h->pl.nb * h->pl.M * 2; } // of one clip

// steps 1-2 for every clip
int analyse(zen_hip_cqt* h, const float* in, size_t in_stride)
{
	const size_t Ls = h->pl.Ls, M = h->pl.M, nb = h->pl.nb, rows = h->C * h->ns;
	{
		zen_cqt::SliceArgs a = {in, h->tab.h, h->rows, in_stride, h->n, h->ns, h->C, (int)Ls};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_SLICE, sizeof(float) * (h->C * h->n + rows * 2 * Ls)));
		ZA_HIP(zen_cqt::launch_slice(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_SLICE_FFT, sizeof(float) * rows * 4 * Ls));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft_slice, h->rows, rows, 0, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_cqt::FoldArgs a = {h->rows, h->coef, h->tab, rows, (int)Ls, (int)nb, (int)M};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_FOLD, sizeof(float) * rows * (2 * (Ls / 2 + 1) + 2 * nb * M)));
		ZA_HIP(zen_cqt::launch_fold(a, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_BAND_IFFT, sizeof(float) * rows * nb * 4 * M));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft_band, h->coef, rows * nb, 1, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

// step 3 for clip c
int magnitudes(zen_hip_cqt* h, size_t c, float* v, size_t v_stride)
{
	zen_cqt::OverlapArgs a = {h->coef + c * coef_floats(h), v, v_stride, h->ns, (int)h->pl.nb, (int)h->pl.M};
	auto kt = h->prof.on_stream(h->stream);
	ZA_TRY(kt.begin(K_OVERLAP, sizeof(float) * (coef_floats(h) + h->T * h->pl.nb)));
	ZA_HIP(zen_cqt::launch_overlap(a, h->stream));
	ZA_TRY(kt.end());
	return ZEN_HIP_OK;
}

// step 4 on the clip in h->v
int medians(zen_hip_cqt* h)
{
	const unsigned long long bytes = sizeof(float) * 2 * h->T * h->pl.nb;
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_MEDIAN_TIME, bytes));
		ZA_ZEN(zen_hip_mfilt_run(h->med_time, h->v, h->hm, h->stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_MEDIAN_FREQ, bytes));
		ZA_ZEN(zen_hip_mfilt_run(h->med_freq, h->v, h->pm, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

// steps 5-7 for clip c: stem >= 0 masks the coefficients at `coef` (8-byte aligned: the handle's own), stem < 0 takes them as
// they are (any 4-byte aligned address: they are copied)
int synthesise(zen_hip_cqt* h, size_t c, const float* coef, int stem, float* out)
{
	const size_t Ls = h->pl.Ls, M = h->pl.M, nb = h->pl.nb, ns = h->ns;
	float* rows = h->rows + c * ns * 2 * Ls;
	for (size_t q0 = 0; q0 < ns; q0 += h->run) {
		const size_t run = ns - q0 < h->run ? ns - q0 : h->run, run_floats = run * nb * M * 2;
		if (stem >= 0) {
			zen_cqt::MaskArgs a = {coef, h->hm, h->pm, h->scratch, q0, run, h->beta, (int)nb, (int)M, stem, h->soft};
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_MASK, sizeof(float) * (2 * run_floats + 2 * (run + 1) * (M / 2) * nb)));
			ZA_HIP(zen_cqt::launch_mask(a, h->stream));
			ZA_TRY(kt.end());
		} else {
			ZA_HIP(hipMemcpyAsync(h->scratch, coef + q0 * nb * M * 2, sizeof(float) * run_floats, hipMemcpyDeviceToDevice, h->stream));
		}
		{
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_BAND_FFT, sizeof(float) * 2 * run_floats));
			ZA_ZEN(zen_hip_fft_exec_batched(h->fft_band, h->scratch, run * nb, 0, h->stream));
			ZA_TRY(kt.end());
		}
		{
			zen_cqt::GatherArgs a = {h->scratch, rows, h->tab, q0, run, (int)Ls, (int)nb, (int)M};
			auto kt = h->prof.on_stream(h->stream);
			ZA_TRY(kt.begin(K_GATHER, sizeof(float) * run * (4 * (Ls / 2 + 1) + 2 * Ls)));
			ZA_HIP(zen_cqt::launch_gather(a, h->stream));
			ZA_TRY(kt.end());
		}
	}
	{
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_SLICE_IFFT, sizeof(float) * ns * 4 * Ls));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft_slice, rows, ns, 1, h->stream));
		ZA_TRY(kt.end());
	}
	{
		zen_cqt::OlaArgs a = {rows, h->tab.s, out, h->n, h->n, ns, 1, (int)Ls};
		auto kt = h->prof.on_stream(h->stream);
		ZA_TRY(kt.begin(K_OLA, sizeof(float) * h->n * 7)); // two complex values and two of s read, one sample written
		ZA_HIP(zen_cqt::launch_overlap_add(a, h->stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

int check_rows(const char* who, zen_hip_cqt_t h, const void* p, size_t stride, const char* what, bool required)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null handle", who);
	if (!p && required)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null %s", who, what);
	if ((uintptr_t)p & 3)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: float pointers need 4-byte alignment (%s)", who, what);
	if (p && stride < h->n)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: %s stride %zu below the %zu samples of a clip", who, what, stride, h->n);
	return ZEN_HIP_OK;
}

int check_separate(const char* who, zen_hip_cqt_t h, const void* in, size_t in_stride, void* const out[3], size_t out_stride)
{
	ZA_TRY(check_rows(who, h, in, in_stride, "input", true));
	for (int o = 0; o < 3; ++o)
		ZA_TRY(check_rows(who, h, out[o], out_stride, "output", false));
	return ZEN_HIP_OK;
}

// the arguments are checked; the outputs are device rows
int separate(zen_hip_cqt* h, const float* in, size_t in_stride, float* const out[3], size_t out_stride)
{
	ZA_TRY(analyse(h, in, in_stride));
	for (size_t c = 0; c < h->C && (out[0] || out[1] || out[2]); ++c) {
		ZA_TRY(magnitudes(h, c, h->v, h->pl.nb));
		ZA_TRY(medians(h));
		for (int stem = 0; stem < 3; ++stem) {
			if (!out[stem])
				continue;
			float* row = out[stem] + c * out_stride;
			if (h->soft && stem == zen_cqt::STEM_RESIDUAL)
				ZA_HIP(hipMemsetAsync(row, 0, sizeof(float) * h->n, h->stream)); // the soft masks leave nothing: +0
			else
				ZA_TRY(synthesise(h, c, h->coef + c * coef_floats(h), stem, row));
		}
	}
	h->calls += 1;
	h->clips += h->C;
	return ZEN_HIP_OK;
}

// rows of `cnt` floats between host and device memory
int copy_rows(zen_hip_cqt* h, void* dst, size_t dst_stride, const void* src, size_t src_stride, size_t cnt, hipMemcpyKind kind)
{
	return h->copy_rows(dst, dst_stride, src, src_stride, cnt, h->C, kind);
}

} // namespace

extern "C" {

const char* zen_hip_cqt_last_error(void) { return t_err; }
const char* zen_hip_cqt_version(void) { return "zen_hip_cqt 1 (gfx950)"; }

int zen_hip_cqt_plan(float fs, size_t slice, int bands_per_octave, double fmin, size_t* nb, size_t* m, int* centres, size_t cap)
{
	Plan pl;
	ZA_TRY(plan_centres("cqt_plan", fs, slice, bands_per_octave, fmin, &pl));
	if (centres && cap < pl.nb)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_plan: room for %zu centres, the plan has %zu", cap, pl.nb);
	if (nb)
		*nb = pl.nb;
	if (m)
		*m = pl.M;
	for (size_t k = 0; centres && k < pl.nb; ++k)
		centres[k] = pl.p[k];
	return ZEN_HIP_OK;
}

int zen_hip_cqt_table(float fs, size_t slice, int bands_per_octave, double fmin, int which, void* out, size_t cap)
{
	if (!out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_table: null output");
	if (which < ZEN_HIP_CQT_TABLE_KB || which > ZEN_HIP_CQT_TABLE_S)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_table: unknown table %d", which);
	Plan pl;
	ZA_TRY(plan_centres("cqt_table", fs, slice, bands_per_octave, fmin, &pl));
	const size_t len = which >= ZEN_HIP_CQT_TABLE_H ? pl.Ls : pl.N + 1;
	if (cap < len)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_table: room for %zu values, the table has %zu", cap, len);
	plan_tables(&pl);
	if (which == ZEN_HIP_CQT_TABLE_KB) {
		memcpy(out, pl.kb.data(), sizeof(int) * len);
		return ZEN_HIP_OK;
	}
	const std::vector<float>* t[] = {nullptr, &pl.gL, &pl.gU, &pl.gdL, &pl.gdU, &pl.h, &pl.s};
	memcpy(out, t[which]->data(), sizeof(float) * len);
	return ZEN_HIP_OK;
}

int zen_hip_cqt_create(float fs, size_t slice, int bands_per_octave, double fmin, size_t n_clips, size_t n_samples, zen_hip_cqt_t* out)
{
	if (!out || n_clips == 0 || n_samples == 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_create: null handle, zero clips or zero samples");
	Plan pl;
	ZA_TRY(plan_centres("cqt_create", fs, slice, bands_per_octave, fmin, &pl));
	const size_t N = pl.N, Ls = pl.Ls, nb = pl.nb, M = pl.M;
	if (n_samples > (size_t)(ZEN_HIP_CQT_MAX_SLICES - 1) * N)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_create: %zu samples are more than %d slices at a hop of %zu", n_samples, (int)ZEN_HIP_CQT_MAX_SLICES, N);
	if (n_clips > ((size_t)1 << 16))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_create: n_clips %zu above 2^16", n_clips);
	const size_t ns = (n_samples + N - 1) / N + 1, T = (ns + 1) * (M / 2);
	if (T > 0x7fffffffu || nb > 0x7fffffffu || T * nb > 0x7fffffffu)
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "cqt_create: a matrix of %zu columns by %zu bands is beyond the median filters", T, nb);
	if (n_clips * ns * nb > 0x7fffffffu || n_clips * ns * nb * M > ((size_t)1 << 36))
		ZA_FAIL(ZEN_HIP_E_UNSUPPORTED, "cqt_create: %zu clips of %zu slices of %zu bands of %zu coefficients are beyond one batched transform", n_clips,
		        ns, nb, M);
	zen_hip_cqt* h = new zen_hip_cqt;
	plan_tables(&pl);
	h->pl = pl;
	h->C = n_clips;
	h->n = n_samples;
	h->ns = ns;
	h->T = T;
	h->B = bands_per_octave;
	h->run = RUN_BYTES / (nb * M * 8);
	h->run = h->run < 1 ? 1 : h->run > ns ? ns : h->run;
	auto build = [&]() -> int {
		int lh, lp;
		default_lengths(h, &lh, &lp);
		ZA_TRY(make_filters(h, lh, lp));
		ZA_ZEN(zen_hip_fft_create(Ls, &h->fft_slice));
		ZA_ZEN(zen_hip_fft_create(M, &h->fft_band));
		const size_t rows = n_clips * ns;
		ZA_TRY(h->alloc(&h->rows, rows * 2 * Ls));
		ZA_TRY(h->alloc(&h->coef, rows * nb * M * 2));
		ZA_TRY(h->alloc(&h->scratch, h->run * nb * M * 2));
		ZA_TRY(h->alloc(&h->v, T * nb));
		ZA_TRY(h->alloc(&h->hm, T * nb));
		ZA_TRY(h->alloc(&h->pm, T * nb));
		ZA_TRY(h->alloc(&h->ftab, 4 * (N + 1) + 2 * Ls));
		ZA_TRY(h->alloc(&h->itab, N + 1 + nb));
		ZA_TRY(h->alloc(&h->stage_in, n_clips * n_samples));
		for (float*& p : h->stage_out)
			ZA_TRY(h->alloc(&p, n_clips * n_samples));
		std::vector<float> ft;
		for (const std::vector<float>* t : {&h->pl.gL, &h->pl.gU, &h->pl.gdL, &h->pl.gdU, &h->pl.h, &h->pl.s})
			ft.insert(ft.end(), t->begin(), t->end());
		std::vector<int> it(h->pl.kb);
		it.insert(it.end(), h->pl.p.begin(), h->pl.p.end());
		ZA_ZEN(zen_hip_memcpy_h2d(h->ftab, ft.data(), sizeof(float) * ft.size()));
		ZA_ZEN(zen_hip_memcpy_h2d(h->itab, it.data(), sizeof(int) * it.size()));
		const float* f = h->ftab;
		h->tab = {h->itab, h->itab + N + 1, f, f + (N + 1), f + 2 * (N + 1), f + 3 * (N + 1), f + 4 * (N + 1), f + 4 * (N + 1) + Ls};
		// whatever the transforms and the medians allocate for their largest batches, up front: one run each on zeros
		ZA_HIP(hipMemsetAsync(h->rows, 0, sizeof(float) * rows * 2 * Ls, h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft_slice, h->rows, rows, 0, h->stream));
		ZA_HIP(hipMemsetAsync(h->coef, 0, sizeof(float) * rows * nb * M * 2, h->stream));
		ZA_ZEN(zen_hip_fft_exec_batched(h->fft_band, h->coef, rows * nb, 0, h->stream));
		ZA_HIP(hipMemsetAsync(h->v, 0, sizeof(float) * T * nb, h->stream));
		ZA_ZEN(zen_hip_mfilt_run(h->med_time, h->v, h->hm, h->stream));
		ZA_ZEN(zen_hip_mfilt_run(h->med_freq, h->v, h->pm, h->stream));
		ZA_HIP(hipStreamSynchronize(h->stream));
		return ZEN_HIP_OK;
	};
	ZA_TRY(build_or_destroy(build, [&] { zen_hip_cqt_destroy(h); }));
	*out = h;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_destroy(zen_hip_cqt_t h)
{
	if (!h)
		return ZEN_HIP_OK;
	if (h->rows)
		(void)hipStreamSynchronize(h->stream);
	zen_hip_fft_destroy(h->fft_slice);
	zen_hip_fft_destroy(h->fft_band);
	zen_hip_mfilt_destroy(h->med_time);
	zen_hip_mfilt_destroy(h->med_freq);
	h->release({h->rows, h->coef, h->scratch, h->v, h->hm, h->pm, h->ftab, h->itab, h->stage_in, h->stage_out[0], h->stage_out[1], h->stage_out[2]});
	delete h;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_set_stream(zen_hip_cqt_t h, void* stream) { return set_stream(h, stream, "cqt"); }

int zen_hip_cqt_set_params(zen_hip_cqt_t h, float beta, int soft, int lh, int lp)
{
	if (!h)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_set_params: null handle");
	if (beta == 0.0f)
		beta = 2.0f;
	if (!(beta >= 1.0f) || !std::isfinite(beta))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_set_params: beta %g is not 0 (the default) or a finite value from 1 on", (double)beta);
	if (lh < 0 || lp < 0)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_set_params: median lengths %d and %d", lh, lp);
	int dh, dp;
	default_lengths(h, &dh, &dp);
	lh = lh ? lh : dh;
	lp = lp ? lp : dp;
	if ((size_t)lh > h->T)
		ZA_FAIL(ZEN_HIP_E_FILTER_TOO_BIG, "cqt_set_params: a median over %d columns, the clip has %zu", lh, h->T);
	if ((size_t)lp > h->pl.nb)
		ZA_FAIL(ZEN_HIP_E_FILTER_TOO_BIG, "cqt_set_params: a median over %d bands, the plan has %zu", lp, h->pl.nb);
	if (lh != h->lh || lp != h->lp) {
		ZA_HIP(hipStreamSynchronize(h->stream));
		ZA_TRY(make_filters(h, lh, lp));
	}
	h->beta = beta;
	h->soft = soft != 0;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_shape(zen_hip_cqt_t h, zen_hip_cqt_shape_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_shape: null argument");
	out->slices = h->ns;
	out->bands = h->pl.nb;
	out->m = h->pl.M;
	out->columns = h->T;
	out->run = h->run;
	out->lh = (size_t)h->lh;
	out->lp = (size_t)h->lp;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_forward_device(zen_hip_cqt_t h, const float* in_dev, size_t in_stride, float* coef_dev)
{
	const char* who = "cqt_forward_device";
	ZA_TRY(check_rows(who, h, in_dev, in_stride, "input", true));
	if (!coef_dev || ((uintptr_t)coef_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned output", who);
	ZA_TRY(analyse(h, in_dev, in_stride));
	ZA_HIP(hipMemcpyAsync(coef_dev, h->coef, sizeof(float) * h->C * coef_floats(h), hipMemcpyDeviceToDevice, h->stream));
	h->calls += 1;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_spectrogram_device(zen_hip_cqt_t h, const float* in_dev, size_t in_stride, float* v_dev, size_t v_stride)
{
	const char* who = "cqt_spectrogram_device";
	ZA_TRY(check_rows(who, h, in_dev, in_stride, "input", true));
	if (!v_dev || ((uintptr_t)v_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned output", who);
	if (v_stride < h->pl.nb)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: v_stride %zu below the %zu bands of a column", who, v_stride, h->pl.nb);
	ZA_TRY(analyse(h, in_dev, in_stride));
	for (size_t c = 0; c < h->C; ++c)
		ZA_TRY(magnitudes(h, c, v_dev + c * h->T * v_stride, v_stride));
	h->calls += 1;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_inverse_device(zen_hip_cqt_t h, const float* coef_dev, float* out_dev, size_t out_stride)
{
	const char* who = "cqt_inverse_device";
	ZA_TRY(check_rows(who, h, out_dev, out_stride, "output", true));
	if (!coef_dev || ((uintptr_t)coef_dev & 3))
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "%s: null or misaligned coefficients", who);
	for (size_t c = 0; c < h->C; ++c)
		ZA_TRY(synthesise(h, c, coef_dev + c * coef_floats(h), -1, out_dev + c * out_stride));
	h->calls += 1;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_separate_device(zen_hip_cqt_t h, const float* in_dev, size_t in_stride, float* harmonic_dev, float* percussive_dev,
                                float* residual_dev, size_t out_stride)
{
	float* const out[3] = {harmonic_dev, percussive_dev, residual_dev};
	ZA_TRY(check_separate("cqt_separate_device", h, in_dev, in_stride, (void* const*)out, out_stride));
	return separate(h, in_dev, in_stride, out, out_stride);
}

int zen_hip_cqt_separate_host(zen_hip_cqt_t h, const float* in_host, size_t in_stride, float* harmonic_host, float* percussive_host,
                              float* residual_host, size_t out_stride)
{
	float* const host[3] = {harmonic_host, percussive_host, residual_host};
	ZA_TRY(check_separate("cqt_separate_host", h, in_host, in_stride, (void* const*)host, out_stride));
	float* const dev[3] = {host[0] ? h->stage_out[0] : nullptr, host[1] ? h->stage_out[1] : nullptr, host[2] ? h->stage_out[2] : nullptr};
	int rc = copy_rows(h, h->stage_in, h->n, in_host, in_stride, h->n, hipMemcpyHostToDevice);
	if (rc == ZEN_HIP_OK)
		rc = separate(h, h->stage_in, h->n, dev, h->n);
	for (int o = 0; o < 3 && rc == ZEN_HIP_OK; ++o)
		if (host[o])
			rc = copy_rows(h, host[o], out_stride, dev[o], h->n, h->n, hipMemcpyDeviceToHost);
	const hipError_t es = hipStreamSynchronize(h->stream); // whatever happened, nothing of this call stays in flight
	ZA_TRY(rc);
	ZA_HIP(es);
	return ZEN_HIP_OK;
}

int zen_hip_cqt_stats(zen_hip_cqt_t h, zen_hip_cqt_stats_t* out)
{
	if (!h || !out)
		ZA_FAIL(ZEN_HIP_E_BAD_ARG, "cqt_stats: null argument");
	out->calls = h->calls;
	out->clips = h->clips;
	out->device_bytes = h->mem.device_bytes;
	out->allocations = h->mem.allocations;
	return ZEN_HIP_OK;
}

int zen_hip_cqt_profile(zen_hip_cqt_t h, int enable) { return profile(h, enable); }

int zen_hip_cqt_profile_get(zen_hip_cqt_t h, double ms[ZEN_HIP_CQT_KERNELS], unsigned long long bytes[ZEN_HIP_CQT_KERNELS],
                            unsigned long long launches[ZEN_HIP_CQT_KERNELS])
{
	return profile_get(h, ms, bytes, launches, "cqt");
}

} // extern "C"
