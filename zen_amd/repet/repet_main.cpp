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

#include "wav.h"
#include "zen_hip.h"
#include "zen_hip_repet.h"

namespace {

void check(int rc, const char* what, const char* msg)
{
	if (rc != ZEN_HIP_OK)
		throw std::runtime_error(std::string(what) + ": " + msg);
}
#define ZEN(call) check((call), #call, zen_hip_last_error())
#define REPET(call) check((call), #call, zen_hip_repet_last_error())

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
		char* end = nullptr;
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			prefix = argv[++i];
		} else if (!strcmp(argv[i], "--nfft") && i + 1 < argc) {
			nfft = (size_t)strtoull(argv[++i], &end, 10);
			if (*end)
				return usage();
		} else if (!strcmp(argv[i], "--period") && i + 1 < argc) {
			period_s = strtod(argv[++i], &end);
			if (*end || !(period_s > 0.0))
				return usage();
		} else if (!strcmp(argv[i], "--highpass") && i + 1 < argc) {
			highpass = strtod(argv[++i], &end);
			if (*end || !(highpass >= 0.0))
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
	int status = 0;
	try {
		zen::wav::AudioData fd;
		zen::wav::load(fd, infile);
		std::vector<float> mono;
		if (fd.channelCount == 2) {
			mono.resize(fd.samples.size() / 2);
			zen::wav::stereo_to_mono(fd.samples.data(), mono.data(), fd.samples.size());
		} else {
			mono = fd.samples;
		}
		const size_t n = mono.size(), hop = nfft / 2;
		if (n == 0)
			throw std::runtime_error("no samples in " + infile);
		const float fs = (float)fd.sampleRate;
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
		zen::wav::encode_pcm16_mono(bg, fd.sampleRate, prefix + "_background.wav");
		zen::wav::encode_pcm16_mono(fg, fd.sampleRate, prefix + "_foreground.wav");
		if (used)
			printf("period: %zu frames, %.4f s\n", used, (double)(used * hop) / (double)fs);
		else
			printf("period: none found\n");
	} catch (const std::exception& e) {
		fprintf(stderr, "zen-repet: %s\n", e.what());
		status = 1;
	}
	zen_hip_repet_destroy(rp);
	zen_hip_free(dev);
	if (status == 0) { // as `zen`: a red zone found overwritten is an error of its own
		zen_hip_memcheck_report rep;
		if (zen_hip_memcheck(&rep) == ZEN_HIP_OK && rep.corrupt_words) {
			fprintf(stderr, "zen-repet: memory check: %s\n", rep.first_message);
			status = 86;
		}
	}
	return status;
}
