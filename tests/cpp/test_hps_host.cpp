// test_hps_host.cpp -- HPRIOffline<GPU>::process (zen_amd/libzen/hps.cpp) and its helper threads (host_threads.h) against the
// test double of the C-ABI (fake_zen_hip.cpp): no device.  Built plain, under -fsanitize=thread and under
// -fsanitize=address,undefined by tests/test_host_threads.py.  Prints "passed" and returns 0 only if every case holds.
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <dirent.h>
#include <unistd.h>

#include <libzen/hps.h>

extern "C" {
extern std::size_t fake_zen_hip_range_samples;
extern int fake_zen_hip_misbehave;
}

#if defined(__SANITIZE_THREAD__) || defined(__SANITIZE_ADDRESS__)
#define UNDER_SANITIZER 1
#endif

using zen::Backend;
typedef zen::hps::HPRIOffline<Backend::GPU> Offline;

static int g_checks = 0, g_fail = 0;
#define CHECK(c)                                                        \
	do {                                                                \
		++g_checks;                                                     \
		if (!(c)) {                                                     \
			++g_fail;                                                   \
			std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
		}                                                               \
	} while (0)

#ifndef UNDER_SANITIZER
// every helper thread has been joined by the time static destructors have run: this handler is registered first, so it runs last
static void count_threads_at_exit()
{
	int tasks = 0;
	if (DIR* d = opendir("/proc/self/task")) {
		while (dirent* e = readdir(d))
			tasks += e->d_name[0] != '.';
		closedir(d);
	}
	if (tasks != 1) {
		std::printf("FAILED: %d threads alive at exit\n", tasks);
		std::fflush(stdout);
		_exit(1);
	}
}
#endif

static std::vector<float> clip(std::size_t n, unsigned seed)
{
	std::vector<float> x(n);
	unsigned lcg = seed;
	for (std::size_t i = 0; i < n; ++i) {
		lcg = lcg * 1664525u + 1013904223u;
		x[i] = (float)(lcg >> 8) / 8388608.0f - 1.0f; // [-1, 1)
	}
	return x;
}

static std::uint32_t bits(float f)
{
	std::uint32_t u;
	std::memcpy(&u, &f, 4);
	return u;
}

// three vectors of size n; harmonic and percussive bit-equal to the fake's function of x, every residual sample +0.0f
static bool correct(const std::array<std::vector<float>, 3>& out, const std::vector<float>& x)
{
	const std::size_t n = x.size();
	if (out[0].size() != n || out[1].size() != n || out[2].size() != n)
		return false;
	bool same = true;
	for (std::size_t i = 0; i < n; ++i) {
		const float harm = 0.5f * x[i];
		same = same && bits(out[0][i]) == bits(harm) && bits(out[1][i]) == bits(x[i] - harm) && bits(out[2][i]) == 0u;
	}
	return same;
}

static void test_sizes_and_ranges()
{
	const std::size_t m = (std::size_t)1 << 21;
	const std::size_t sizes[] = {0, 1, m - 1, m, m + 12345, 2 * m + 4099 /* prefaulter engaged */, 4 * m + 1 /* deferred free */};
	const std::size_t ranges[] = {(std::size_t)4 << 20, (std::size_t)1 << 20, 1000003 /* divides no n */};
	Offline hpss(44100.0F, 4096, 256, 2.0, 2.0);
	for (std::size_t len : ranges) {
		fake_zen_hip_range_samples = len;
		for (std::size_t n : sizes) {
			const auto x = clip(n, 12345u + (unsigned)n);
			CHECK(correct(hpss.process(x), x)); // by value
			auto copy = x;
			CHECK(correct(hpss.process(std::move(copy)), x)); // moved in
		}
	}
	fake_zen_hip_range_samples = (std::size_t)4 << 20;
}

static void test_three_calls_in_a_row()
{
	Offline hpss(44100.0F);
	for (unsigned r = 0; r < 3; ++r) {
		const auto x = clip(((std::size_t)1 << 23) + 1, 77u + r);
		CHECK(correct(hpss.process(x), x));
	}
}

// the deferred free is shared by every object of the process
static void test_two_objects_on_two_threads()
{
	bool ok[2] = {false, false};
	std::thread th[2];
	for (unsigned t = 0; t < 2; ++t)
		th[t] = std::thread([t, &ok] {
			Offline hpss(44100.0F, 4096, 256);
			const auto x = clip(((std::size_t)1 << 23) + 1, 1000u + t);
			bool all = true;
			for (int r = 0; r < 2; ++r)
				all = all && correct(hpss.process(x), x);
			ok[t] = all;
		});
	for (auto& t : th)
		t.join();
	CHECK(ok[0] && ok[1]);
}

static void test_misbehaving_engine()
{
	Offline hpss(44100.0F);
	const auto x = clip(((std::size_t)1 << 23) + 1, 5u);
	for (int how = 1; how <= 2; ++how) { // 1: a range out of order, 2: the last range left out
		fake_zen_hip_misbehave = how;
		bool thrown = false;
		try {
			hpss.process(x);
		}
		catch (const zen::ZgException& e) {
			thrown = std::string(e.what()).find("did not arrive in order") != std::string::npos;
		}
		fake_zen_hip_misbehave = 0;
		CHECK(thrown);
		CHECK(correct(hpss.process(x), x)); // the object is still good
	}
}

static void test_other_entry_points()
{
	bool thrown = false;
	try {
		Offline bad(44100.0F, 4096, 300);
	}
	catch (const zen::ZgException&) {
		thrown = true;
	}
	CHECK(thrown);
	Offline hpss(44100.0F);
	hpss.use_sse_filter();
	hpss.use_soft_mask();
	zen::hps::HPRRealtime<Backend::GPU> rt(44100.0F, 256, 2.0F, zen::hps::OUTPUT_PERCUSSIVE);
	rt.use_soft_mask();
}

int main()
{
#ifndef UNDER_SANITIZER
	std::atexit(count_threads_at_exit);
#endif
	test_sizes_and_ranges();
	test_three_calls_in_a_row();
	test_two_objects_on_two_threads();
	test_misbehaving_engine();
	test_other_entry_points();
	std::printf("%d checks, %d failures\n", g_checks, g_fail);
	if (g_fail)
		return 1;
	std::printf("passed\n");
	return 0;
}
