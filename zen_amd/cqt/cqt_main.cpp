// cqt_main.cpp -- zen_amd/bin/zen-cqt: harmonic, percussive and residual stems of a recording by median filtering in a
// constant-Q domain.
//
//   zen-cqt in.wav -o prefix [--slice 16384] [--bpo 12] [--fmin 60] [--beta 2] [--soft-mask]
//
// The file is mixed to mono as `zen offline` does, uploaded once and separated by one zen_hip_cqt_separate_device call;
// prefix_harm.wav, prefix_perc.wav and prefix_residual.wav are written as `zen offline` writes its stems: divided by the
// stem's peak (a silent stem stays silent), 16-bit PCM with cli/wav.h's rounding.  The plan is printed first.  A recording of
// more than 4096 slices is refused: the library has no streaming form of the transform.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "wav.h"
#include "zen_hip.h"
#include "zen_hip_cqt.h"

namespace {

void check(int rc, const char* what, const char* msg)
{
	if (rc != ZEN_HIP_OK)
		throw std::runtime_error(std::string(what) + ": " + msg);
}
#define ZEN(call) check((call), #call, zen_hip_last_error())
#define CQT(call) check((call), #call, zen_hip_cqt_last_error())

int usage()
{
	fprintf(stderr, "usage: zen-cqt in.wav -o prefix [--slice N] [--bpo B] [--fmin Hz] [--beta b] [--soft-mask]\n  N: the slice, a power of two in "
	                "64..32768 (default 16384); B: bands per octave, 1..96 (default 12); Hz: the lowest band (default 60); b: the separation "
	                "factor of the hard masks, from 1 on (default 2)\n  writes prefix_harm.wav, prefix_perc.wav and prefix_residual.wav; at most "
	                "4096 slices of N / 2 samples\n");
	return 2;
}

void peak_normalise(std::vector<float>& x) // as `zen offline`; a stem of zeros is left as it is
{
	auto limits = std::minmax_element(x.begin(), x.end());
	const float real_max = std::max(-1 * (*limits.first), *limits.second);
	if (!(real_max > 0.0f))
		return;
	for (float& v : x)
		v /= real_max;
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile, prefix;
	size_t slice = 16384;
	long bpo = 12;
	double fmin = 60.0, beta = 2.0;
	int soft = 0;
	for (int i = 1; i < argc; ++i) {
		char* end = nullptr;
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			prefix = argv[++i];
		} else if (!strcmp(argv[i], "--slice") && i + 1 < argc) {
			slice = (size_t)strtoull(argv[++i], &end, 10);
			if (*end)
				return usage();
		} else if (!strcmp(argv[i], "--bpo") && i + 1 < argc) {
			bpo = strtol(argv[++i], &end, 10);
			if (*end || bpo < 1 || bpo > 96)
				return usage();
		} else if (!strcmp(argv[i], "--fmin") && i + 1 < argc) {
			fmin = strtod(argv[++i], &end);
			if (*end || !(fmin > 0.0))
				return usage();
		} else if (!strcmp(argv[i], "--beta") && i + 1 < argc) {
			beta = strtod(argv[++i], &end);
			if (*end || !(beta >= 1.0))
				return usage();
		} else if (!strcmp(argv[i], "--soft-mask")) {
			soft = 1;
		} else if (argv[i][0] == '-' || !infile.empty()) {
			return usage();
		} else {
			infile = argv[i];
		}
	}
	if (infile.empty() || prefix.empty())
		return usage();
	zen_hip_cqt_t cq = nullptr;
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
		const size_t n = mono.size();
		if (n == 0)
			throw std::runtime_error("no samples in " + infile);
		const float fs = (float)fd.sampleRate;
		size_t nb = 0, m = 0;
		CQT(zen_hip_cqt_plan(fs, slice, (int)bpo, fmin, &nb, &m, nullptr, 0));
		printf("plan: %zu bands, %zu coefficients per band and slice, %.2f columns per second\n", nb, m, (double)fs * (double)m / (double)slice);
		ZEN(zen_hip_init(0));
		CQT(zen_hip_cqt_create(fs, slice, (int)bpo, fmin, 1, n, &cq));
		CQT(zen_hip_cqt_set_params(cq, (float)beta, soft, 0, 0));
		ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * 4 * n));
		ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * n));
		CQT(zen_hip_cqt_separate_device(cq, dev, n, dev + n, dev + 2 * n, dev + 3 * n, n));
		static const char* suffix[3] = {"_harm.wav", "_perc.wav", "_residual.wav"};
		std::vector<float> stem(n);
		for (int o = 0; o < 3; ++o) {
			ZEN(zen_hip_memcpy_d2h(stem.data(), dev + (size_t)(o + 1) * n, sizeof(float) * n));
			peak_normalise(stem);
			zen::wav::encode_pcm16_mono(stem, fd.sampleRate, prefix + suffix[o]);
		}
	} catch (const std::exception& e) {
		fprintf(stderr, "zen-cqt: %s\n", e.what());
		status = 1;
	}
	zen_hip_cqt_destroy(cq);
	zen_hip_free(dev);
	if (status == 0) { // as `zen`: a red zone found overwritten is an error of its own
		zen_hip_memcheck_report rep;
		if (zen_hip_memcheck(&rep) == ZEN_HIP_OK && rep.corrupt_words) {
			fprintf(stderr, "zen-cqt: memory check: %s\n", rep.first_message);
			status = 86;
		}
	}
	return status;
}
