// cqt_main.cpp -- zen_amd/bin/zen-cqt: harmonic, percussive and residual stems of a recording by median filtering in a
// constant-Q domain.
//
//   zen-cqt in.wav -o prefix [--slice 16384] [--bpo 12] [--fmin 60] [--beta 2] [--soft-mask]
//
// The file is mixed to mono as `zen offline` does, uploaded once and separated by one zen_hip_cqt_separate_device call;
// prefix_harm.wav, prefix_perc.wav and prefix_residual.wav are written as `zen offline` writes its stems: divided by the
// stem's peak (a silent stem stays silent), 16-bit PCM with cli/wav.h's rounding.  The plan is printed first.  A recording of
// more than 4096 slices is refused: the library has no streaming form of the transform.
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
#include "zen_hip_cqt.h"

using zen::demo::option;

namespace {

#define CQT(call) ZEN_LIB(zen_hip_cqt_last_error, call)

int usage()
{
	fprintf(stderr, "usage: zen-cqt in.wav -o prefix [--slice N] [--bpo B] [--fmin Hz] [--beta b] [--soft-mask]\n  N: the slice, a power of two in "
	                "64..32768 (default 16384); B: bands per octave, 1..96 (default 12); Hz: the lowest band (default 60); b: the separation "
	                "factor of the hard masks, from 1 on (default 2)\n  writes prefix_harm.wav, prefix_perc.wav and prefix_residual.wav; at most "
	                "4096 slices of N / 2 samples\n");
	return 2;
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
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			prefix = argv[++i];
		} else if (!strcmp(argv[i], "--slice") && i + 1 < argc) {
			if (!option(argv[++i], &slice))
				return usage();
		} else if (!strcmp(argv[i], "--bpo") && i + 1 < argc) {
			if (!option(argv[++i], &bpo) || bpo < 1 || bpo > 96)
				return usage();
		} else if (!strcmp(argv[i], "--fmin") && i + 1 < argc) {
			if (!option(argv[++i], &fmin) || !(fmin > 0.0))
				return usage();
		} else if (!strcmp(argv[i], "--beta") && i + 1 < argc) {
			if (!option(argv[++i], &beta) || !(beta >= 1.0))
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
	const auto body = [&] {
		int rate = 0;
		std::vector<float> mono = zen::demo::load_mono(infile, &rate);
		const size_t n = mono.size();
		if (n == 0)
			throw std::runtime_error("no samples in " + infile);
		const float fs = (float)rate;
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
			zen::demo::peak_normalise(stem);
			zen::wav::encode_pcm16_mono(stem, rate, prefix + suffix[o]);
		}
	};
	return zen::demo::run("zen-cqt", body, [&] {
		zen_hip_cqt_destroy(cq);
		zen_hip_free(dev);
	});
}
