// zen_amd/addon/median_select.h compiled as plain C++ (behind tests/cpp/host_shim; tests/test_cpp_host.py builds this with
// -fsanitize=address,undefined): the bitonic network and the pick of the median for every P the kernels instantiate and
// every count 1..P, against std::sort and the (lo + hi) * 0.5f rule, and the register-median body the two libraries share on
// a small matrix, for rows a stride apart (zen_amd/repet) and rows an index list names (zen_amd/repsim).
#include <hip/hip_runtime.h> // tests/cpp/host_shim

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../zen_amd/addon/median_select.h"

using namespace zen_addon;

static int failures = 0;

static uint32_t bits(float x)
{
	uint32_t u;
	memcpy(&u, &x, 4);
	return u;
}

#define CHECK(cond, ...)                 \
	do {                                 \
		if (!(cond)) {                   \
			if (++failures <= 20) {      \
				printf("FAIL: ");        \
				printf(__VA_ARGS__);     \
				printf("\n");            \
			}                            \
		}                                \
	} while (0)

// the median of c values as the contracts state it: sorted, the middle one, or (s[c/2 - 1] + s[c/2]) * 0.5f for an even count
static float reference_median(std::vector<float> v)
{
	std::sort(v.begin(), v.end());
	const size_t c = v.size();
	return (c & 1) ? v[(c - 1) / 2] : (v[c / 2 - 1] + v[c / 2]) * 0.5f;
}

// Bit for bit, with the one freedom a selection has: -0 and +0 compare equal, so which of them stands at a rank is the
// order of equal values, which neither std::sort nor the network promises.  Where the reference is a zero, a zero it is.
static bool same_median(float got, float want) { return bits(got) == bits(want) || (got == 0.0f && want == 0.0f); }

enum Kind { RANDOM, EQUAL, ZEROS, DENORMAL, INF_AMONG, KINDS };
static const char* kind_name[KINDS] = {"random", "all equal", "+-0 mixed", "denormals", "+inf among the values"};

static float value_of(Kind kind, std::mt19937& rng)
{
	std::uniform_real_distribution<float> u(-1.0f, 1.0f);
	switch (kind) {
	case RANDOM: return std::ldexp(u(rng), (int)(rng() % 60) - 30);
	case EQUAL: return 0.37f;
	case ZEROS: {
		const unsigned r = rng() % 4;
		return r == 0 ? 0.0f : r == 1 ? -0.0f : r == 2 ? u(rng) : (rng() & 1 ? 0.0f : -0.0f);
	}
	case DENORMAL: return std::ldexp(u(rng), -140 + (int)(rng() % 12)); // around and below FLT_MIN = 2^-126
	default: return rng() % 3 == 0 ? INFINITY : u(rng) * 100.0f;
	}
}

template <int P>
static void test_network(std::mt19937& rng)
{
	for (int kind = 0; kind < KINDS; ++kind)
		for (int c = 1; c <= P; ++c)
			for (int rep = 0; rep < 50; ++rep) {
				float a[P];
				std::vector<float> vals(c);
				for (int i = 0; i < P; ++i)
					a[i] = i < c ? (vals[i] = value_of((Kind)kind, rng)) : INFINITY;
				std::vector<uint32_t> before(P), after(P);
				for (int i = 0; i < P; ++i)
					before[i] = bits(a[i]);
				sort_network<P>(a);
				for (int i = 0; i < P; ++i)
					after[i] = bits(a[i]);
				bool ascending = true;
				for (int i = 1; i < P; ++i)
					ascending = ascending && a[i - 1] <= a[i];
				std::sort(before.begin(), before.end());
				std::sort(after.begin(), after.end());
				CHECK(ascending && before == after, "P = %d, c = %d, %s: the network does not leave its input sorted", P, c, kind_name[kind]);
				const float got = pick_median<P>(a, c), want = reference_median(vals);
				const float own = (c & 1) ? a[(c - 1) / 2] : (a[c / 2 - 1] + a[c / 2]) * 0.5f; // the rule on the network's own order
				CHECK(bits(got) == bits(own), "P = %d, c = %d, %s: pick %a, the rule on the sorted values gives %a", P, c, kind_name[kind], got, own);
				CHECK(same_median(got, want), "P = %d, c = %d, %s: median %a (%08x), std::sort gives %a (%08x)", P, c, kind_name[kind], got, bits(got),
				      want, bits(want));
			}
}

// ---- the register-median body: a matrix of 3 rows x 9 bins, rows 12 floats apart (16-byte rows for VEC = 4), bin 8 a tail
constexpr int ROWS = 3, BINS = 9, STRIDE = 12;
constexpr float SENTINEL = 12345.0f;

struct Strided { // as zen_amd/repet has it: row q is frame l + q * period while the matrix has one
	const float* v;
	size_t l, period, m;
	bool present(int q) const { return l + (size_t)q * period < m; }
	const float* row(int q) const { return v + (l + (size_t)q * period) * STRIDE; }
};

struct Gathered { // as zen_amd/repsim has it: row q is the q-th frame of a list of c
	const float* v;
	const int* idx;
	int c;
	bool present(int q) const { return q < c; }
	const float* row(int q) const { return v + (size_t)(q < c ? idx[q] : 0) * STRIDE; }
};

template <int P, int VEC, class RowOf>
static void test_body(const RowOf& rows, const float* v, const std::vector<int>& frames, const char* what)
{
	alignas(16) float out[STRIDE];
	for (float& o : out)
		o = SENTINEL;
	for (size_t f = 0; f < BINS; f += VEC) // the lanes of a wave, one after the other
		median_in_registers<P, VEC>(rows, f, (size_t)BINS, out + f);
	for (int f = 0; f < BINS; ++f) {
		std::vector<float> col;
		for (int fr : frames)
			col.push_back(v[fr * STRIDE + f]);
		const float want = reference_median(col);
		CHECK(same_median(out[f], want), "%s, P = %d, VEC = %d, bin %d: %a, the column's median is %a", what, P, VEC, f, out[f], want);
	}
	for (int f = BINS; f < STRIDE; ++f)
		CHECK(out[f] == SENTINEL, "%s, P = %d, VEC = %d: written behind the bins, at %d", what, P, VEC, f);
}

template <int P>
static void test_bodies(const float* v)
{
	for (size_t period = 1; period <= 3; ++period)
		for (size_t l = 0; l < period; ++l) {
			std::vector<int> frames;
			for (size_t fr = l; fr < ROWS; fr += period)
				frames.push_back((int)fr);
			if ((int)frames.size() > P)
				continue;
			const Strided rows = {v, l, period, ROWS};
			test_body<P, 1>(rows, v, frames, "strided");
			test_body<P, 4>(rows, v, frames, "strided");
		}
	const std::vector<std::vector<int>> lists = {{2, 0, 1}, {1, 1}, {2}, {0, 2}, {2, 2, 0, 1}};
	for (const std::vector<int>& list : lists) {
		if ((int)list.size() > P)
			continue;
		const std::vector<int> exact(list); // a list of exactly c entries: nothing behind it may be read (the sanitizer's to see)
		const Gathered rows = {v, exact.data(), (int)exact.size()};
		test_body<P, 1>(rows, v, list, "gathered");
		test_body<P, 4>(rows, v, list, "gathered");
	}
}

int main()
{
	std::mt19937 rng(20240607);
	test_network<2>(rng);
	test_network<4>(rng);
	test_network<8>(rng);
	test_network<16>(rng);
	test_network<32>(rng);

	alignas(16) float v[ROWS * STRIDE];
	std::uniform_real_distribution<float> u(-1.0f, 1.0f);
	for (int r = 0; r < ROWS; ++r)
		for (int f = 0; f < STRIDE; ++f)
			v[r * STRIDE + f] = f < BINS ? u(rng) : NAN; // a NaN behind the bins: a read there would reach a median
	v[0 * STRIDE + 3] = v[2 * STRIDE + 3] = 0.25f; // equal values in a column
	v[1 * STRIDE + 8] = INFINITY;                   // a real +inf, in the tail bin
	test_bodies<2>(v);
	test_bodies<4>(v);
	test_bodies<8>(v);

	if (failures) {
		printf("%d failures\n", failures);
		return 1;
	}
	printf("median_select.h: networks of 2..32 at every count, and the register body on 3 x 9: passed\n");
	return 0;
}
