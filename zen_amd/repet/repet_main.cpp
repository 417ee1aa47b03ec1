// repet_main.cpp -- zen_amd/bin/zen-repet: the repeating background of a recording and what stands in front of it.
//
//   zen-repet in.wav -o prefix [--nfft 2048] [--period seconds] [--highpass 100]
//
// The file is mixed to mono as `zen offline` does, uploaded once and separated by one zen_hip_repet_separate_device call;
// prefix_background.wav and prefix_foreground.wav are written as 16-bit PCM (cli/wav.h's rounding) and the period is printed.
// Without --period it is found from the beat spectrum.  A recording of more than 16384 frames or 256 repetitions is refused:
// the library has no windowed form of the method.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "demo.h"
#include "wav.h"
#include "zen_hip.h"
#include "zen_hip_repet.h"

using zen::demo::option;

namespace {

#define REPET(call) ZEN_LIB(zen_hip_repet_last_error, call)

int usage()
{
	fprintf(stderr, "usage: zen-repet in.wav -o prefix [--nfft N] [--period s] [--highpass Hz]\n  N: the frame, a power of two in 64..8192 (default "
	                "2048); s: the period of the accompaniment in seconds (default: found); Hz: bins below go to the background (default 100, 0 = off)\n"
	                "  writes prefix_background.wav and prefix_foreground.wav; at most 16384 frames of N / 2 samples and 256 repetitions\n");
	return 2;
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile, prefix;
	size_t nfft = 2048;
	double period_s = 0.0, highpass = 100.0;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			prefix = argv[++i];
		} else if (!strcmp(argv[i], "--nfft") && i + 1 < argc) {
			if (!option(argv[++i], &nfft))
				return usage();
		} else if (!strcmp(argv[i], "--period") && i + 1 < argc) {
			if (!option(argv[++i], &period_s) || !(period_s > 0.0))
				return usage();
		} else if (!strcmp(argv[i], "--highpass") && i + 1 < argc) {
			if (!option(argv[++i], &highpass) || !(highpass >= 0.0))
				return usage();
		} else if (argv[i][0] == '-' || !infile.empty()) {
			return usage();
		} else {
			infile = argv[i];
		}
	}
	if (infile.empty() || prefix.empty() || nfft < 2)
		return usage();
	zen_hip_repet_t rp = nullptr;
	float* dev = nullptr;
	const auto body = [&] {
		int rate = 0;
		const std::vector<float> mono = zen::demo::load_mono(infile, &rate);
		const size_t n = mono.size(), hop = nfft / 2;
		if (n == 0)
			throw std::runtime_error("no samples in " + infile);
		const float fs = (float)rate;
		ZEN(zen_hip_init(0));
		REPET(zen_hip_repet_create(fs, nfft, 1, n, &rp));
		REPET(zen_hip_repet_set_params(rp, 0.8, 8.0, highpass));
		size_t given = 0, used = 0;
		if (period_s > 0.0) {
			given = (size_t)floor(period_s * (double)fs / (double)hop + 0.5);
			if (given == 0)
				given = 1;
		}
		std::vector<float> bg(n), fg(n);
		ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * 3 * n));
		ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * n));
		REPET(zen_hip_repet_separate_device(rp, dev, n, n, &given, dev + n, dev + 2 * n, n, &used, nullptr, 0));
		ZEN(zen_hip_memcpy_d2h(bg.data(), dev + n, sizeof(float) * n));
		ZEN(zen_hip_memcpy_d2h(fg.data(), dev + 2 * n, sizeof(float) * n));
		zen::wav::encode_pcm16_mono(bg, rate, prefix + "_background.wav");
		zen::wav::encode_pcm16_mono(fg, rate, prefix + "_foreground.wav");
		if (used)
			printf("period: %zu frames, %.4f s\n", used, (double)(used * hop) / (double)fs);
		else
			printf("period: none found\n");
	};
	return zen::demo::run("zen-repet", body, [&] {
		zen_hip_repet_destroy(rp);
		zen_hip_free(dev);
	});
}
