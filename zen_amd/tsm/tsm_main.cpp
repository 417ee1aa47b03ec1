// tsm_main.cpp -- zen_amd/bin/zen-stretch: a recording played slower or faster at its own pitch.
//
//   zen-stretch in.wav -a 1.5 -o out.wav [--plain] [--nfft 4096] [--nfft-ola 256] [--hpr-hop 1024] [--beta 2.5]
//
// The file is mixed to mono as `zen offline` does, padded with zeros to a multiple of the separation's hop, uploaded once, and
// stays on the device: one zen_hip_hpr_process call (causal, all three outputs) writes the harmonic, the percussive and the
// residual stream behind the input, one zen_hip_tsm_stretch_hp_device call stretches them -- the harmonic one through the
// phase-locked vocoder, the other two through overlap-add on short frames.  --plain: the mixture through the vocoder alone,
// without the separation, to hear the difference.  out.wav is 16-bit PCM (cli/wav.h's rounding), divided by its largest
// magnitude first where that is above 1; the lengths are printed.
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
#include "zen_hip_tsm.h"

using zen::demo::option;

namespace {

#define TSM(call) ZEN_LIB(zen_hip_tsm_last_error, call)

int usage()
{
	fprintf(stderr, "usage: zen-stretch in.wav -a ratio -o out.wav [--plain] [--nfft N] [--nfft-ola P] [--hpr-hop M] [--beta B]\n  ratio: the length of "
	                "the output over the input's, 0.25..4; N: the vocoder's frame, a power of two in 64..8192 (default 4096); P: the overlap-add "
	                "frame, a power of two in 16..4096 (default 256); M: the separation's hop (default 1024); B: separation factor (default 2.5)\n"
	                "  --plain: the vocoder alone on the mixture; at most 16384 frames of N / 4 and of P / 2 output samples: with the defaults 47 s of "
	                "output at 44.1 kHz -- a longer recording takes a longer overlap-add frame (--nfft-ola 2048: 6 minutes)\n");
	return 2;
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile, outfile;
	size_t nfft = 4096, nfft_ola = 256, hpr_hop = 1024;
	double alpha = 0.0;
	float beta = 2.5f;
	bool plain = false;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			outfile = argv[++i];
		} else if (!strcmp(argv[i], "-a") && i + 1 < argc) {
			if (!option(argv[++i], &alpha))
				return usage();
		} else if (!strcmp(argv[i], "--plain")) {
			plain = true;
		} else if (!strcmp(argv[i], "--nfft") && i + 1 < argc) {
			if (!option(argv[++i], &nfft))
				return usage();
		} else if (!strcmp(argv[i], "--nfft-ola") && i + 1 < argc) {
			if (!option(argv[++i], &nfft_ola))
				return usage();
		} else if (!strcmp(argv[i], "--hpr-hop") && i + 1 < argc) {
			if (!option(argv[++i], &hpr_hop))
				return usage();
		} else if (!strcmp(argv[i], "--beta") && i + 1 < argc) {
			if (!option(argv[++i], &beta))
				return usage();
		} else if (argv[i][0] == '-' || !infile.empty()) {
			return usage();
		} else {
			infile = argv[i];
		}
	}
	if (infile.empty() || outfile.empty() || !(alpha >= 0.25 && alpha <= 4.0) || hpr_hop == 0)
		return usage();
	zen_hip_hpr_t hpr = nullptr;
	zen_hip_tsm_t ts = nullptr;
	float *dev = nullptr, *out = nullptr;
	const auto body = [&] {
		int rate = 0;
		std::vector<float> mono = zen::demo::load_mono(infile, &rate);
		if (mono.empty())
			throw std::runtime_error("no samples in " + infile);
		const size_t n = (mono.size() + hpr_hop - 1) / hpr_hop * hpr_hop;
		mono.resize(n, 0.0f);
		const size_t n_out = (size_t)floor((double)n * alpha);
		const float fs = (float)rate;
		if (n_out > 16383 * (nfft_ola / 2) && nfft_ola >= 16 && nfft_ola < 4096)
			throw std::runtime_error("the output of " + std::to_string(n_out) + " samples is more than 16384 overlap-add frames of " +
			                         std::to_string(nfft_ola / 2) + ": pick a longer overlap-add frame with --nfft-ola (up to 4096)");
		ZEN(zen_hip_init(0));
		TSM(zen_hip_tsm_create(fs, nfft, nfft_ola, 1, n, alpha, &ts));
		std::vector<float> y(n_out);
		ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * 4 * n));
		ZEN(zen_hip_malloc((void**)&out, sizeof(float) * n_out));
		ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * n));
		if (plain) {
			TSM(zen_hip_tsm_stretch_pv_device(ts, dev, n, n, alpha, out, n_out));
		} else {
			const unsigned flags = ZEN_HIP_OUTPUT_HARMONIC | ZEN_HIP_OUTPUT_PERCUSSIVE | ZEN_HIP_OUTPUT_RESIDUAL;
			ZEN(zen_hip_hpr_create(fs, hpr_hop, beta, flags, ZEN_HIP_TIME_CAUSAL, 1, 1, 0, &hpr));
			ZEN(zen_hip_hpr_process(hpr, dev, n / hpr_hop, n, dev + n, dev + 2 * n, dev + 3 * n, n));
			TSM(zen_hip_tsm_stretch_hp_device(ts, dev + n, dev + 2 * n, dev + 3 * n, n, n, alpha, out, n_out));
		}
		ZEN(zen_hip_memcpy_d2h(y.data(), out, sizeof(float) * n_out));
		// the causal engine hands out its harmonic and residual rows at the scale of its transform: as `zen offline` does for
		// its stems, the output is divided by its largest magnitude -- here only where that would not fit 16 bits
		float peak = 0.0f;
		for (float v : y)
			peak = fabsf(v) > peak ? fabsf(v) : peak;
		if (peak > 1.0f)
			for (float& v : y)
				v = v / peak;
		zen::wav::encode_pcm16_mono(y, rate, outfile);
		printf("%zu samples in, %zu out, ratio %g%s\n", n, n_out, alpha, plain ? ", vocoder alone" : "");
	};
	return zen::demo::run("zen-stretch", body, [&] {
		zen_hip_tsm_destroy(ts);
		zen_hip_hpr_destroy(hpr);
		zen_hip_free(dev);
		zen_hip_free(out);
	});
}
