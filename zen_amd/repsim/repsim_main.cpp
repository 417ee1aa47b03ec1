// repsim_main.cpp -- zen_amd/bin/zen-repsim: the repeating background of a recording and what stands in front of it, where
// the repetition has no single period.
//
//   zen-repsim in.wav -o prefix [--nfft 2048] [--distance 1] [--number 100] [--threshold 0] [--highpass 100]
//
// The file is mixed to mono as `zen offline` does, uploaded once and separated by one zen_hip_repsim_separate_device call;
// prefix_background.wav and prefix_foreground.wav are written as 16-bit PCM (cli/wav.h's rounding) and the mean number of
// frames a frame's median was taken over is printed.  A recording of more than 16384 frames is refused: the library has no
// windowed form of the method.
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
#include "zen_hip_repsim.h"

using zen::demo::option;

namespace {

#define REPSIM(call) ZEN_LIB(zen_hip_repsim_last_error, call)

int usage()
{
	fprintf(stderr, "usage: zen-repsim in.wav -o prefix [--nfft N] [--distance s] [--number k] [--threshold t] [--highpass Hz]\n  N: the frame, a power "
	                "of two in 64..8192 (default 2048); s: the least distance between two frames of one median in seconds (default 1); k: the "
	                "frames of a median, 1..256 (default 100); t: the least similarity of such a frame, in [0, 1) (default 0); Hz: bins below go "
	                "to the background (default 100, 0 = off)\n  writes prefix_background.wav and prefix_foreground.wav; at most 16384 frames "
	                "of N / 2 samples\n");
	return 2;
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile, prefix;
	size_t nfft = 2048, number = 100;
	double distance = 1.0, threshold = 0.0, highpass = 100.0;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			prefix = argv[++i];
		} else if (!strcmp(argv[i], "--nfft") && i + 1 < argc) {
			if (!option(argv[++i], &nfft))
				return usage();
		} else if (!strcmp(argv[i], "--number") && i + 1 < argc) {
			if (!option(argv[++i], &number))
				return usage();
		} else if (!strcmp(argv[i], "--distance") && i + 1 < argc) {
			if (!option(argv[++i], &distance) || !(distance >= 0.0))
				return usage();
		} else if (!strcmp(argv[i], "--threshold") && i + 1 < argc) {
			if (!option(argv[++i], &threshold) || !(threshold >= 0.0))
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
	zen_hip_repsim_t rs = nullptr;
	float* dev = nullptr;
	int* counts_dev = nullptr;
	const auto body = [&] {
		int rate = 0;
		std::vector<float> mono = zen::demo::load_mono(infile, &rate);
		const size_t n = mono.size(), hop = nfft / 2;
		if (n == 0)
			throw std::runtime_error("no samples in " + infile);
		const float fs = (float)rate;
		ZEN(zen_hip_init(0));
		REPSIM(zen_hip_repsim_create(fs, nfft, 1, n, &rs));
		REPSIM(zen_hip_repsim_set_params(rs, threshold, distance, number, highpass));
		const size_t m = (n + hop - 1) / hop + 1;
		std::vector<float> bg(n), fg(n);
		std::vector<int> counts(m);
		ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * 3 * n));
		ZEN(zen_hip_malloc((void**)&counts_dev, sizeof(int) * m));
		ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * n));
		REPSIM(zen_hip_repsim_separate_device(rs, dev, n, n, dev + n, dev + 2 * n, n, counts_dev, nullptr));
		ZEN(zen_hip_memcpy_d2h(bg.data(), dev + n, sizeof(float) * n));
		ZEN(zen_hip_memcpy_d2h(fg.data(), dev + 2 * n, sizeof(float) * n));
		ZEN(zen_hip_memcpy_d2h(counts.data(), counts_dev, sizeof(int) * m));
		zen::wav::encode_pcm16_mono(bg, rate, prefix + "_background.wav");
		zen::wav::encode_pcm16_mono(fg, rate, prefix + "_foreground.wav");
		unsigned long long total = 0;
		for (int c : counts)
			total += (unsigned long long)c;
		printf("frames: %zu, a median over %.2f frames in the mean\n", m, (double)total / (double)m);
	};
	return zen::demo::run("zen-repsim", body, [&] {
		zen_hip_repsim_destroy(rs);
		zen_hip_free(dev);
		zen_hip_free(counts_dev);
	});
}
