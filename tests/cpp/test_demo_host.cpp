// test_demo_host.cpp -- zen_amd/cli/demo.h on the host alone, behind stubs of the zen_hip_* functions it names (run from
// tests/test_cpp_host.py with the address and undefined-behaviour sanitizers): the option parsers against what strtoull,
// strtol, strtod and strtof with a `*end` test take, load_mono against wav.h called directly, peak_normalise, and the three
// exits of the runner with what they write to stderr.
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "demo.h"

static unsigned long long g_corrupt = 0;
static int g_memcheck_rc = ZEN_HIP_OK, g_memchecks = 0;

extern "C" const char* zen_hip_last_error(void) { return "the stub's message"; }
extern "C" int zen_hip_memcheck(zen_hip_memcheck_report* out)
{
	memset(out, 0, sizeof(*out));
	out->corrupt_words = g_corrupt;
	snprintf(out->first_message, sizeof(out->first_message), "3 words behind allocation 7");
	++g_memchecks;
	return g_memcheck_rc;
}

static int failures = 0;
#define EXPECT(cond)                                                   \
	do {                                                               \
		if (!(cond)) {                                                 \
			printf("line %d: %s does not hold\n", __LINE__, #cond);    \
			++failures;                                                \
		}                                                              \
	} while (0)

// what `f` writes to stderr
template <class F>
static std::string stderr_of(F f)
{
	fflush(stderr);
	const int saved = dup(2);
	FILE* t = tmpfile();
	dup2(fileno(t), 2);
	f();
	fflush(stderr);
	dup2(saved, 2);
	close(saved);
	std::string s;
	rewind(t);
	for (int c; (c = fgetc(t)) != EOF;)
		s.push_back((char)c);
	fclose(t);
	return s;
}

static void put16(FILE* f, unsigned v) { fputc(v & 255, f), fputc((v >> 8) & 255, f); }
static void put32(FILE* f, unsigned v) { put16(f, v & 65535), put16(f, v >> 16); }

static void write_pcm16(const std::string& path, int channels, int rate, const std::vector<short>& s)
{
	FILE* f = fopen(path.c_str(), "wb");
	const unsigned bytes = (unsigned)s.size() * 2;
	fwrite("RIFF", 1, 4, f), put32(f, 36 + bytes), fwrite("WAVEfmt ", 1, 8, f), put32(f, 16), put16(f, 1), put16(f, channels);
	put32(f, rate), put32(f, rate * channels * 2), put16(f, channels * 2), put16(f, 16), fwrite("data", 1, 4, f), put32(f, bytes);
	for (short v : s)
		put16(f, (unsigned short)v);
	fclose(f);
}

int main(int argc, char** argv)
{
	using namespace zen::demo;
	const std::string dir = argc > 1 ? argv[1] : ".";

	// the parsers: the whole string is the number; the empty string is zero; a sign in front of an unsigned value wraps
	size_t z = 7;
	unsigned long long u = 7;
	long l = 7;
	double d = 7;
	float f = 7;
	EXPECT(option("12", &z) && z == 12 && option("12", &u) && u == 12 && option("12", &l) && l == 12);
	EXPECT(option("12", &d) && d == 12.0 && option("12", &f) && f == 12.0f);
	EXPECT(!option("12x", &z) && !option("12x", &u) && !option("12x", &l) && !option("12x", &d) && !option("12x", &f));
	EXPECT(option("", &z) && z == 0 && option("", &u) && u == 0 && option("", &l) && l == 0 && option("", &d) && d == 0.0 && option("", &f) && f == 0.0f);
	EXPECT(option("-1", &z) && z == (size_t)-1 && option("-1", &u) && u == ~0ull && option("-1", &l) && l == -1);
	EXPECT(option("-1", &d) && d == -1.0 && option("-1", &f) && f == -1.0f);
	EXPECT(!option("1e3", &z) && !option("1e3", &u) && !option("1e3", &l) && option("1e3", &d) && d == 1000.0 && option("1e3", &f) && f == 1000.0f);
	for (const char* s : {"12", "12x", "", "-1", "1e3", " 5", "0x10", "nan"}) { // and against the library calls themselves
		char* end = nullptr;
		const unsigned long long wu = strtoull(s, &end, 10);
		EXPECT(option(s, &u) == !*end && u == wu && option(s, &z) == !*end && z == (size_t)wu);
		const long wl = strtol(s, &end, 10);
		EXPECT(option(s, &l) == !*end && l == wl);
		const double wd = strtod(s, &end);
		EXPECT(option(s, &d) == !*end && !memcmp(&d, &wd, sizeof(d)));
		const float wf = strtof(s, &end);
		EXPECT(option(s, &f) == !*end && !memcmp(&f, &wf, sizeof(f)));
	}

	// load_mono: a mono file as it is, a stereo one as wav.h mixes it
	const std::vector<short> samples = {0, 1000, -32768, 32767, -5, 6, 12345, -12346};
	for (int channels = 1; channels <= 2; ++channels) {
		const std::string path = dir + "/demo" + std::to_string(channels) + ".wav";
		write_pcm16(path, channels, 8000 * channels, samples);
		zen::wav::AudioData fd;
		zen::wav::load(fd, path);
		std::vector<float> want = fd.samples;
		if (channels == 2) {
			want.assign(samples.size() / 2, 0.0f);
			zen::wav::stereo_to_mono(fd.samples.data(), want.data(), fd.samples.size());
		}
		int rate = 0;
		const std::vector<float> got = load_mono(path, &rate);
		EXPECT(fd.channelCount == channels && rate == 8000 * channels && got.size() == samples.size() / channels);
		EXPECT(got.size() == want.size() && !memcmp(got.data(), want.data(), sizeof(float) * got.size()));
		if (channels == 2)
			EXPECT(got[1] == (-32768 / 32767.f + 32767 / 32767.f) / 2.0f);
	}
	std::string what;
	try {
		int rate = 0;
		load_mono(dir + "/absent.wav", &rate);
	} catch (const std::exception& e) {
		what = e.what();
	}
	EXPECT(what == "cannot open " + dir + "/absent.wav");

	// peak_normalise: zeros stay, the largest magnitude becomes 1 whatever its sign
	std::vector<float> zeros(5, 0.0f), neg = {0.25f, -0.5f, 0.125f};
	peak_normalise(zeros);
	peak_normalise(neg);
	EXPECT(zeros == std::vector<float>(5, 0.0f) && neg == (std::vector<float>{0.5f, -1.0f, 0.25f}));

	// check and its macro
	what.clear();
	try {
		ZEN(ZEN_HIP_E_BAD_ARG);
	} catch (const std::exception& e) {
		what = e.what();
	}
	EXPECT(what == "ZEN_HIP_E_BAD_ARG: the stub's message");
	ZEN(ZEN_HIP_OK);

	// the runner: 0, 1 and 86; the release step runs every time, the memory check only behind a body that went well
	int released = 0, status = -1;
	std::string err = stderr_of([&] { status = run("prog", [] {}, [&] { ++released; }); });
	EXPECT(status == 0 && err.empty() && released == 1 && g_memchecks == 1);
	err = stderr_of([&] { status = run("prog", [] { throw std::runtime_error("cannot open x.wav"); }, [&] { ++released; }); });
	EXPECT(status == 1 && err == "prog: cannot open x.wav\n" && released == 2 && g_memchecks == 1);
	g_corrupt = 3;
	err = stderr_of([&] { status = run("prog", [] {}, [&] { ++released; }); });
	EXPECT(status == 86 && err == "prog: memory check: 3 words behind allocation 7\n" && released == 3 && g_memchecks == 2);
	err = stderr_of([&] { status = run("prog", [] { throw std::runtime_error("first"); }, [&] { ++released; }); });
	EXPECT(status == 1 && err == "prog: first\n" && released == 4 && g_memchecks == 2);
	g_memcheck_rc = ZEN_HIP_E_BAD_ARG; // a check that could not be made is no finding
	err = stderr_of([&] { status = run("prog", [] {}, [&] { ++released; }); });
	EXPECT(status == 0 && err.empty() && released == 5);

	printf(failures ? "%d failures\n" : "passed\n", failures);
	return failures ? 1 : 0;
}
