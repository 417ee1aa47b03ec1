// test_blockrun_edge_count_host.cpp -- zen_amd/blockrun/blockrun_edge_count.h run on the CPU (plain C++, no GPU) against the
// selection it replaces: for bin N/2 and the bins N - 23 .. N - 1 of a magnitude row the counted mask bit must equal
//   hard_mask_exact(median, mag + FLT_EPSILON, thr),   thr = hard_mask_threshold(beta),
// with the median of the 47 keys of the window taken by znet::medians<47, 1, 47> (median_net.h under ZNET_HOST_TEST).
//
//   test_blockrun_edge_count_host [rows_per_unit]      (default 1000: about 2 * 10^6 windows)
//
// A row is mag[0 .. N/2] as bit patterns.  The COUNT reads it from an image built by the kernel's rules (blockrun_kernel.hip:
// FwdOut's columns 0 .. N/2 and its mirrors of bins 1 .. 56 and 2009 .. 2047, the border loop's replicas; every other word
// of the image holds garbage), through a wave of arrays in place of the device's EdgeWave.  The REFERENCE reads the bordered
// Hermitian row built from mag directly: column c is mag[0] below 0, mag[c] up to N/2, mag[N - c] up to N - 1, mag[1] above.
// Row families: uniform and log-uniform magnitudes; rows quantised to 8 levels; rows whose elements sit at f* (the smallest
// float above the threshold product), at the float below and at the float above it; rows of zeros, subnormals, FLT_MIN and
// FLT_MAX; rows with +inf / NaN patterns at exactly 0, 1, 23, 24 and 47 positions of one of the 24 windows (each in turn).
// Betas: 0.5, 1, 1.5, 2, 3 (even significands: the inclusive threshold) and 2 + 2^-22 (odd: the strict one).
// For bin N/2 the direct count over all 47 columns is compared with the 23-key form the routine uses.
#include <hip/hip_runtime.h> // tests/cpp/host_shim

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define ZNET_HOST_TEST 1
using std::max;
using std::min;
static inline int __float_as_int(float f)
{
	int i;
	std::memcpy(&i, &f, 4);
	return i;
}
static inline float __int_as_float(int i)
{
	float f;
	std::memcpy(&f, &i, 4);
	return f;
}
struct int4 {
	int x, y, z, w;
};
[[maybe_unused]] static inline int4 make_int4(int x, int y, int z, int w) { return {x, y, z, w}; }

#include "../../zen_amd/csrc/masks.h"
#include "../../zen_amd/csrc/median_net.h"
#include "../../zen_amd/blockrun/blockrun_edge_count.h"

using namespace zen_blockrun;

static constexpr int N = 4096, NH = N / 2, TAPS = 47, MID = TAPS / 2;
static constexpr int MIR_LO = 56, MIR_HI = 39, IMG_END = 255 * 16 + 64; // blockrun_kernel.hip
static constexpr int IMG_WORDS = (IMG_END / 16) * EDGE_IMG_RSTR;
static constexpr int KEY_INF = 0x7f800000;

struct HostWave { // the 64 lanes of the device's EdgeWave
	int a[64], b[64], k[64];
	unsigned long long ge(bool from_b, int K) const
	{
		unsigned long long m = 0;
		for (int l = 0; l < 64; ++l)
			m |= (unsigned long long)((from_b ? b[l] : a[l]) >= K) << l;
		return m;
	}
	int threshold(int j) const { return k[j]; }
};

static std::mt19937 rng(20240611);
static unsigned garbage_state = 12345u;
static int garbage() { return (int)(garbage_state = garbage_state * 1664525u + 1013904223u); }

// the image as FwdOut and the border loop leave it; everything else garbage (NaN patterns and negative keys among it)
static void build_image(const std::vector<int>& mag, std::vector<int>& img)
{
	for (int& w : img)
		w = garbage();
	for (int k = 0; k <= NH; ++k)
		img[edge_img_addr(k)] = mag[k];
	for (int k = 1; k <= MIR_LO; ++k)
		img[edge_img_addr(N - k)] = mag[k];
	for (int k = NH - MIR_HI; k < NH; ++k)
		img[edge_img_addr(N - k)] = mag[k];
	const int v0 = img[edge_img_addr(0)], v1 = img[edge_img_addr(N - 1)];
	for (int g = 0; g < EDGE_IMG_COL0; ++g)
		img[edge_img_addr(g - EDGE_IMG_COL0)] = v0;
	for (int g = N + EDGE_IMG_COL0; g < IMG_END; ++g)
		img[edge_img_addr(g - EDGE_IMG_COL0)] = v1;
}

static int column(const std::vector<int>& mag, int c) // the bordered Hermitian row
{
	return c < 0 ? mag[0] : c <= NH ? mag[c] : c < N ? mag[N - c] : mag[1];
}

static long long g_windows = 0, g_bad = 0, g_set = 0, g_at_fstar = 0, g_below_fstar = 0, g_nan_median = 0, g_no_fstar = 0, g_succ = 0;
static long long g_flip[EDGE_OUTPUTS][2];

static void check_row(const std::vector<int>& mag, double thr, const char* family)
{
	static std::vector<int> img(IMG_WORDS);
	build_image(mag, img);
	HostWave w;
	for (int l = 0; l < 64; ++l) {
		w.a[l] = img[edge_img_addr(l)];
		w.b[l] = img[edge_img_addr(NH - l)];
		w.k[l] = edge_threshold_key(thr, l == 0 ? w.b[l] : w.a[l]);
	}
	const unsigned bits = edge_count_bits(w);
	for (int j = 0; j < EDGE_OUTPUTS; ++j) {
		const int bin = j == 0 ? NH : N - j;
		int e[TAPS], out[1];
		for (int i = 0; i < TAPS; ++i)
			e[i] = column(mag, bin - MID + i);
		znet::medians<TAPS, 1, TAPS>(e, out);
		const float d = __int_as_float(column(mag, bin)) + FLT_EPSILON;
		const float want = zen_hip_impl::hard_mask_exact(__int_as_float(out[0]), d, thr);
		const float got = (bits >> j) & 1u ? 1.0f : 0.0f;
		// f* found independently of the routine: step up from the rounded product
		const double t = thr * (double)d;
		bool has = t < (double)INFINITY;
		float fs = (float)t;
		if (has) {
			if ((double)fs > t)
				; // fl(t) is f*
			else {
				fs = std::nextafterf(fs, INFINITY);
				++g_succ;
			}
			if (w.k[j] != __float_as_int(fs)) {
				if (g_bad < 20)
					std::printf("FAIL %s: threshold key of output %d: %08x, want %08x\n", family, j, w.k[j], __float_as_int(fs));
				++g_bad;
			}
			g_at_fstar += out[0] == __float_as_int(fs);
			g_below_fstar += out[0] == __float_as_int(fs) - 1;
		}
		else {
			++g_no_fstar;
		}
		g_nan_median += out[0] > KEY_INF;
		if (j == 0 && has) { // 2c + b >= 24 <=> c >= 12: the full window's count against the 23-key form
			int full = 0;
			for (int i = 0; i < TAPS; ++i)
				full += e[i] >= w.k[0];
			if ((full >= 24) != edge_count_reaches(w.ge(true, w.k[0]), 0)) {
				if (g_bad < 20)
					std::printf("FAIL %s: bin N/2: %d of 47 keys reach the threshold, the 23-key form disagrees\n", family, full);
				++g_bad;
			}
		}
		++g_windows;
		g_set += want != 0.0f;
		++g_flip[j][want != 0.0f];
		if (want != got) {
			if (g_bad < 20)
				std::printf("FAIL %s: bin %d: counted %g, selected %g (median %08x, mag %08x, thr %a)\n", family, bin, got, want, out[0],
				            column(mag, bin), thr);
			++g_bad;
		}
	}
}

static float uni(float lo, float hi) { return lo + (hi - lo) * (float)((rng() >> 8) * (1.0 / 16777216.0)); }

// only mag[0 .. 63] and mag[N/2 - 63 .. N/2] reach the count or the reference: `gen` fills those, the rest is garbage
template <class G>
static void fill(std::vector<int>& mag, G gen)
{
	for (int k = 0; k <= NH; ++k)
		mag[k] = (k < 64 || k > NH - 64) ? __float_as_int(gen(k)) : (garbage() & 0x7fffffff);
}

static float fstar_of(float v, double thr)
{
	const double t = thr * (double)(v + FLT_EPSILON);
	float fs = (float)t;
	while (!((double)fs > t))
		fs = std::nextafterf(fs, INFINITY);
	return fs;
}

static void run_beta(float beta, int unit)
{
	int inc = 0;
	const double thr = zen_hip_impl::hard_mask_threshold(beta, &inc);
	if (!(thr > 0.0)) {
		std::printf("FAIL beta %g: no threshold\n", beta);
		++g_bad;
		return;
	}
	std::vector<int> mag(NH + 1);
	// ---- uniform and log-uniform magnitudes
	for (int r = 0; r < 4 * unit; ++r) {
		if (r & 1)
			fill(mag, [](int) { return uni(0.0f, 1.0f); });
		else
			fill(mag, [](int) { return std::exp2f(uni(-30.0f, 30.0f)); });
		check_row(mag, thr, "uniform");
	}
	// ---- heavily tied rows: 8 levels (a level and beta times it among them, so both mask values occur)
	for (int r = 0; r < 3 * unit; ++r) {
		const float base = uni(0.001f, 4.0f), step = (r & 1) ? base : base * beta * 0.5f;
		fill(mag, [&](int) { return base + step * (float)(rng() & 7); });
		check_row(mag, thr, "tied");
	}
	// ---- elements at f*, the float below and the float above, f* that of a centre value v which a share of the elements hold
	for (int r = 0; r < 3 * unit; ++r) {
		const float v = (r % 3 == 0) ? std::exp2f(uni(-20.0f, 20.0f)) : uni(0.01f, 1.0f);
		const float fs = fstar_of(v, thr);
		const float lo = std::nextafterf(fs, 0.0f), hi = std::nextafterf(fs, INFINITY);
		const unsigned share = 1 + rng() % 6; // of 8: elements that are v
		fill(mag, [&](int) {
			if (rng() % 8 < share)
				return v;
			const unsigned c = rng() % 3;
			return c == 0 ? lo : c == 1 ? fs : hi;
		});
		if (r & 1)
			mag[NH] = __float_as_int(v);
		check_row(mag, thr, "at f*");
	}
	// ---- zeros, subnormals, FLT_MIN, FLT_MAX
	for (int r = 0; r < 2 * unit; ++r) {
		static const float alphabet[] = {0.0f, 0x1p-149f, 0x1.8p-140f, 0x1.fffffcp-127f, FLT_MIN, 0x1p-23f, 1.0f, FLT_MAX, 0x1p127f};
		const unsigned span = 2 + rng() % 8, first = rng() % (9 - std::min(span, 8u));
		fill(mag, [&](int) { return alphabet[std::min(first + (unsigned)(rng() % span), 8u)]; });
		check_row(mag, thr, "extremes");
	}
	// ---- +inf and NaN patterns at exactly c positions of the window of one output
	static const int counts[] = {0, 1, 23, 24, 47};
	static const int nonfinite[] = {KEY_INF, 0x7fc00000, 0x7f800001, 0x7fffffff, (int)0xffc00000u};
	for (int rep = 0; rep < std::max(1, unit / 250); ++rep)
		for (int j = 0; j < EDGE_OUTPUTS; ++j)
			for (int c : counts)
				for (int kind = 0; kind < 4; ++kind) {
					if (rep & 1)
						fill(mag, [&](int) { return 0.25f * (float)(1 + (rng() & 7)); });
					else
						fill(mag, [](int) { return uni(0.0f, 1.0f); });
					auto value = [&]() {
						return kind == 0 ? KEY_INF : kind == 1 ? nonfinite[1 + rng() % 3] : kind == 2 ? nonfinite[rng() % 4] : nonfinite[rng() % 5];
					};
					std::vector<int> singles;
					int placed = 0;
					if (j == 0) { // mag[N/2 - 23 .. N/2 - 1] twice each, mag[N/2] once
						for (int k = NH - MID; k < NH; ++k)
							singles.push_back(k);
						std::shuffle(singles.begin(), singles.end(), rng);
						for (int i = 0; i < c / 2; ++i, placed += 2)
							mag[singles[i]] = value();
						if (c & 1) {
							mag[NH] = value();
							++placed;
						}
					}
					else { // mag[1] 25 - j times, mag[2 .. j + 23] once each
						const int m1 = 25 - j, ns = j + 22;
						for (int k = 2; k <= j + 23; ++k)
							singles.push_back(k);
						std::shuffle(singles.begin(), singles.end(), rng);
						int rest = c;
						if (c >= m1 && (c > ns || (rng() & 1))) {
							mag[1] = value();
							rest -= m1;
							placed += m1;
						}
						for (int i = 0; i < rest; ++i, ++placed)
							mag[singles[i]] = value();
					}
					if (placed != c) {
						std::printf("FAIL test construction: %d of %d positions\n", placed, c);
						++g_bad;
					}
					check_row(mag, thr, "non-finite");
				}
}

int main(int argc, char** argv)
{
	const int unit = argc > 1 ? std::atoi(argv[1]) : 1000;
	const float betas[] = {0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 2.0f + 0x1p-22f};
	for (float beta : betas) {
		const long long w0 = g_windows, b0 = g_bad;
		run_beta(beta, unit);
		std::printf("beta %.9g (%s threshold): %lld windows, %lld mismatches\n", beta, (__float_as_int(beta) & 1) ? "strict" : "inclusive",
		            g_windows - w0, g_bad - b0);
	}
	int both = 0;
	for (int j = 0; j < EDGE_OUTPUTS; ++j)
		both += g_flip[j][0] > 0 && g_flip[j][1] > 0;
	std::printf("masks set: %lld, median at f*: %lld, median one float below f*: %lld, f* the successor of the rounded product: %lld\n", g_set,
	            g_at_fstar, g_below_fstar, g_succ);
	std::printf("NaN medians: %lld, windows without f*: %lld, outputs that took both values: %d of %d\n", g_nan_median, g_no_fstar, both,
	            EDGE_OUTPUTS);
	if (both != EDGE_OUTPUTS || g_at_fstar == 0 || g_below_fstar == 0 || g_nan_median == 0 || g_no_fstar == 0 || g_succ == 0) {
		std::printf("FAIL: a case the test is about never occurred\n");
		++g_bad;
	}
	std::printf("edge count against the selected median: %lld windows, %lld mismatches, done\n", g_windows, g_bad);
	return g_bad ? 1 : 0;
}
