// test_blockrun_first_pass_host.cpp -- zen_amd/blockrun/blockrun_first_pass.h run on the CPU (plain C++, no GPU) against
// the generic butterfly<16, false, true, true, .> of zen_amd/csrc/fft_dev.h, with the twiddle table the engine builds
// (zen_hip_impl::make_twiddles of libzen_hip.so, which this program links against).
//
//   test_blockrun_first_pass_host [n_random]
//
// For n_random (default 2^20) random 8-sample inputs of several kinds and a list of special ones (zeros, single samples,
// +-FLT_MAX, denormals, an infinity / a NaN in every position, inputs from a small alphabet that cancel everywhere) the
// 16 outputs of first_pass16<false, SYM> are compared with the generic butterfly's on bits; +0 and -0 compare equal; where
// the generic value is not finite the routine's must not be finite either (NaN payloads and signs are free).  Both cases of
// the switch are run: SYM = true where the table has the symmetry (asserted for the engine's table: that is the shipped
// case), SYM = false on the engine's table and on a perturbed table without the symmetry.  Prints, for information, how
// many zeros differed in sign.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define ZBR_FIRST_PASS_HOST_TEST 1
#include "../../zen_amd/blockrun/blockrun_first_pass.h" // (fft_dev.h finds tests/cpp/host_shim/hip/hip_runtime.h)

namespace zen_hip_impl {
void make_twiddles(float* tw_interleaved, size_t n);
}

static constexpr int LOG2N = 12, N = 1 << LOG2N;

struct HostTw {
	static constexpr bool PLAIN = true;
	static constexpr bool PACKED = false;
	const float2* p;
	float2 get(int, int, int, int idx) const { return p[idx]; }
};

static uint32_t bits(float f)
{
	uint32_t u;
	std::memcpy(&u, &f, 4);
	return u;
}

static long long g_cases = 0, g_bad = 0, g_zero_sign = 0;

// finite values on bits (+0 == -0); where the generic value is not finite the routine's must not be finite either
static bool same(float want, float got)
{
	if (!std::isfinite(want))
		return !std::isfinite(got);
	if (want == 0.0f && got == 0.0f) {
		g_zero_sign += bits(want) != bits(got);
		return true;
	}
	return bits(want) == bits(got);
}

template <bool SYM>
static void check(const float (&p)[8], const float2* tw, const char* what)
{
	float2 a[16], Y[16];
	for (int m = 0; m < 16; ++m)
		a[m] = make_float2(m < 8 ? p[m] : 0.0f, 0.0f);
	const HostTw t{tw};
	zfft::butterfly<16, false, true, true, HostTw>(a, 0, 0, LOG2N, t, 0, 0);
	zen_blockrun::first_pass16<false, SYM>(p, tw[N / 16], tw[N / 8], tw[3 * N / 16], Y);
	++g_cases;
	for (int c = 0; c < 16; ++c) {
		const bool ok = same(a[c].x, Y[c].x) && same(a[c].y, Y[c].y);
		if (!ok) {
			if (g_bad < 20) {
				std::printf("FAIL %s SYM=%d k=%d: generic (%a, %a) routine (%a, %a)  input", what, (int)SYM, c, a[c].x, a[c].y, Y[c].x, Y[c].y);
				for (int m = 0; m < 8; ++m)
					std::printf(" %a", p[m]);
				std::printf("\n");
			}
			++g_bad;
		}
	}
}

template <bool SYM>
static void run_all(const float2* tw, long long n_random, const char* what)
{
	float p[8];
	auto fill = [&](float v) {
		for (float& x : p)
			x = v;
	};
	// ---- special inputs
	fill(0.0f);
	check<SYM>(p, tw, "zeros");
	fill(-0.0f);
	check<SYM>(p, tw, "negative zeros");
	const float singles[] = {1.0f, -1.0f, 0.37f, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, 1e-45f, -1e-45f, 3e-42f, INFINITY, -INFINITY, NAN};
	for (float v : singles) {
		for (int m = 0; m < 8; ++m) {
			fill(0.0f);
			p[m] = v;
			check<SYM>(p, tw, "single sample");
			for (int i = 0; i < 8; ++i)
				p[i] = i == m ? v : 0.25f * (float)(i + 1);
			check<SYM>(p, tw, "single sample among finite ones");
		}
		fill(v);
		check<SYM>(p, tw, "constant");
		for (int m = 0; m < 8; ++m)
			p[m] = (m & 1) ? -v : v;
		check<SYM>(p, tw, "alternating");
	}
	std::mt19937_64 rng(12345);
	// ---- a small alphabet: sums and differences cancel in every stage
	{
		const float alpha[] = {0.0f, 1.0f, -1.0f, 0.5f, -0.5f, 0.70710677f, 2.0f, 0.0f};
		for (long long i = 0; i < (n_random >> 2) + 1; ++i) {
			uint64_t r = rng();
			for (int m = 0; m < 8; ++m, r >>= 3)
				p[m] = alpha[r & 7];
			check<SYM>(p, tw, "alphabet");
		}
	}
	// ---- random inputs: uniform(-1, 1) (windowed audio), any finite bit pattern, denormals, values near FLT_MAX
	std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
	for (long long i = 0; i < n_random; ++i) {
		for (int m = 0; m < 8; ++m)
			p[m] = uni(rng);
		check<SYM>(p, tw, "uniform");
	}
	for (long long i = 0; i < (n_random >> 1); ++i) {
		for (int m = 0; m < 8; ++m) {
			uint32_t u;
			do
				u = (uint32_t)rng();
			while ((u & 0x7f800000u) == 0x7f800000u);
			std::memcpy(&p[m], &u, 4);
		}
		check<SYM>(p, tw, "any finite bits");
	}
	for (long long i = 0; i < (n_random >> 2); ++i) {
		for (int m = 0; m < 8; ++m) {
			const uint32_t u = ((uint32_t)rng() & 0x807fffffu) | ((rng() & 3) == 0 ? 0x00800000u : 0u);
			std::memcpy(&p[m], &u, 4);
		}
		check<SYM>(p, tw, "denormals");
		for (int m = 0; m < 8; ++m) {
			const uint32_t u = ((uint32_t)rng() & 0x807fffffu) | (0xfcu + (uint32_t)(rng() % 3)) << 23;
			std::memcpy(&p[m], &u, 4);
		}
		check<SYM>(p, tw, "near FLT_MAX");
	}
	(void)what;
}

int main(int argc, char** argv)
{
	const long long n_random = argc > 1 ? std::atoll(argv[1]) : (1ll << 20);
	std::vector<float> tw(N);
	zen_hip_impl::make_twiddles(tw.data(), N);
	const float2* t = reinterpret_cast<const float2*>(tw.data());
	// the shipped case: the engine's table has the symmetry
	const bool sym = zen_blockrun::table_is_symmetric(tw.data(), N);
	std::printf("table symmetry of the engine's %d-point table: %s\n", N, sym ? "holds (shipped case: SYM)" : "DOES NOT HOLD (fallback)");
	if (!sym) {
		std::printf("FAIL: the shipped table is documented as symmetric (DESIGN section 14)\n");
		return 1;
	}
	run_all<true>(t, n_random, "engine table");
	const long long sym_cases = g_cases, sym_zero = g_zero_sign;
	run_all<false>(t, n_random >> 2, "engine table");
	// a table without the symmetry: the check must say so, and the fallback must still be the generic butterfly's
	std::vector<float> tw2(tw);
	tw2[2 * (N / 8) + 1] = std::nextafterf(tw2[2 * (N / 8) + 1], 0.0f);
	tw2[2 * (3 * N / 16)] = std::nextafterf(tw2[2 * (3 * N / 16)], 0.0f);
	if (zen_blockrun::table_is_symmetric(tw2.data(), N)) {
		std::printf("FAIL: a perturbed table passes table_is_symmetric\n");
		return 1;
	}
	run_all<false>(reinterpret_cast<const float2*>(tw2.data()), n_random >> 2, "perturbed table");
	std::printf("%lld inputs (%lld with SYM), %lld mismatches, zeros of the other sign: %lld (%lld with SYM)\n", g_cases, sym_cases, g_bad,
	            g_zero_sign, sym_zero);
	return g_bad ? 1 : 0;
}
