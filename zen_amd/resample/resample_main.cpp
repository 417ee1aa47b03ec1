// resample_main.cpp -- zen_amd/bin/zen-shift: a recording at another pitch and its own tempo, or at another sample rate.
//
//   zen-shift in.wav -s semitones -o out.wav [--plain] [--quality 8|16|32] [--nfft 4096] [--nfft-ola 256] [--hpr-hop 1024] [--beta 2.5]
//   zen-shift in.wav --rate 44100 -o out.wav [--quality 8|16|32]
//
// The file is mixed to mono as `zen offline` does and uploaded once.  -s: padded with zeros to a multiple of the separation's
// hop, one zen_hip_hpr_process call (causal, all three outputs) writes the stems behind the input, one
// zen_hip_tsm_stretch_hp_device call stretches them by alpha = den / num, one zen_hip_resample_run_device call brings the
// result back by num / den, (num, den) from zen_hip_resample_ratio_for_shift; the n - 3 .. n samples that gives are padded
// with zeros to n.  --plain: the mixture through the vocoder alone in front of the resampler, without the separation.
// --rate: the samples through the resampler alone, by new rate / old rate.  out.wav is 16-bit PCM (cli/wav.h's rounding),
// divided by its largest magnitude first where that is above 1; the lengths are printed.
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
#include "zen_hip_resample.h"
#include "zen_hip_tsm.h"

using zen::demo::option;

namespace {

#define TSM(call) ZEN_LIB(zen_hip_tsm_last_error, call)
#define RES(call) ZEN_LIB(zen_hip_resample_last_error, call)

int usage()
{
	fprintf(stderr, "usage: zen-shift in.wav -s semitones -o out.wav [--plain] [--quality 8|16|32] [--nfft N] [--nfft-ola P] [--hpr-hop M] [--beta B]\n"
	                "       zen-shift in.wav --rate hertz -o out.wav [--quality 8|16|32]\n  semitones: -24..24, the output keeps the length of the "
	                "input; hertz: the new sample rate, a quarter to four times the file's; quality: zero crossings of the filter per side "
	                "(default 16)\n  N, P, M, B: the time stretch's frames, the separation's hop and factor, as zen-stretch has them; --plain: the "
	                "vocoder alone on the mixture in front of the resampler\n");
	return 2;
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile, outfile;
	size_t nfft = 4096, nfft_ola = 256, hpr_hop = 1024;
	double semitones = 0.0;
	unsigned long long rate = 0;
	int quality = 16;
	float beta = 2.5f;
	bool plain = false, have_shift = false;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			outfile = argv[++i];
		} else if (!strcmp(argv[i], "-s") && i + 1 < argc) {
			have_shift = true;
			if (!option(argv[++i], &semitones))
				return usage();
		} else if (!strcmp(argv[i], "--rate") && i + 1 < argc) {
			if (!option(argv[++i], &rate) || rate == 0)
				return usage();
		} else if (!strcmp(argv[i], "--quality") && i + 1 < argc) {
			long q = 0;
			if (!option(argv[++i], &q))
				return usage();
			quality = (int)q;
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
	if (infile.empty() || outfile.empty() || have_shift == (rate != 0) || !(fabs(semitones) <= 24.0) || hpr_hop == 0 ||
	    (quality != 8 && quality != 16 && quality != 32))
		return usage();
	zen_hip_hpr_t hpr = nullptr;
	zen_hip_tsm_t ts = nullptr;
	zen_hip_resample_t rs = nullptr;
	float *dev = nullptr, *mid = nullptr, *out = nullptr;
	const auto body = [&] {
		int file_rate = 0;
		std::vector<float> mono = zen::demo::load_mono(infile, &file_rate);
		if (mono.empty())
			throw std::runtime_error("no samples in " + infile);
		std::vector<float> y;
		unsigned long long num = 0, den = 0, k = 0;
		int out_rate = file_rate;
		if (rate) {
			// the resampler alone: refused here, before a device is touched, where the ratio is outside its range
			const size_t n = mono.size();
			num = rate;
			den = (unsigned long long)file_rate;
			RES(zen_hip_resample_n_out(num, den, n, &k));
			ZEN(zen_hip_init(0));
			RES(zen_hip_resample_create(num, den, quality, &rs));
			ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * n));
			ZEN(zen_hip_malloc((void**)&out, sizeof(float) * k));
			ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * n));
			RES(zen_hip_resample_run_device(rs, dev, n, 0, n, n, 0, (size_t)k, out, (size_t)k, 1));
			y.resize((size_t)k);
			ZEN(zen_hip_memcpy_d2h(y.data(), out, sizeof(float) * k));
			out_rate = (int)rate;
			printf("%zu samples at %d Hz in, %llu at %llu Hz out, quality %d\n", n, file_rate, k, rate, quality);
		} else {
			const size_t n = (mono.size() + hpr_hop - 1) / hpr_hop * hpr_hop;
			mono.resize(n, 0.0f);
			RES(zen_hip_resample_ratio_for_shift(semitones, &num, &den));
			const double alpha = (double)den / (double)num;
			const size_t m = (size_t)floor((double)n * alpha);
			if (m == 0)
				throw std::runtime_error("nothing left of " + std::to_string(n) + " samples");
			RES(zen_hip_resample_n_out(num, den, m, &k));
			if (k > n)
				throw std::runtime_error("the length rule of the shift does not hold");
			const float fs = (float)file_rate;
			if (m > 16383 * (nfft_ola / 2) && nfft_ola >= 16 && nfft_ola < 4096)
				throw std::runtime_error("the stretched " + std::to_string(m) + " samples are more than 16384 overlap-add frames of " +
				                         std::to_string(nfft_ola / 2) + ": pick a longer overlap-add frame with --nfft-ola (up to 4096)");
			ZEN(zen_hip_init(0));
			TSM(zen_hip_tsm_create(fs, nfft, nfft_ola, 1, n, alpha, &ts));
			RES(zen_hip_resample_create(num, den, quality, &rs));
			ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * 4 * n));
			ZEN(zen_hip_malloc((void**)&mid, sizeof(float) * m));
			ZEN(zen_hip_malloc((void**)&out, sizeof(float) * n));
			ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * n));
			if (plain) {
				TSM(zen_hip_tsm_stretch_pv_device(ts, dev, n, n, alpha, mid, m));
			} else {
				const unsigned flags = ZEN_HIP_OUTPUT_HARMONIC | ZEN_HIP_OUTPUT_PERCUSSIVE | ZEN_HIP_OUTPUT_RESIDUAL;
				ZEN(zen_hip_hpr_create(fs, hpr_hop, beta, flags, ZEN_HIP_TIME_CAUSAL, 1, 1, 0, &hpr));
				ZEN(zen_hip_hpr_process(hpr, dev, n / hpr_hop, n, dev + n, dev + 2 * n, dev + 3 * n, n));
				TSM(zen_hip_tsm_stretch_hp_device(ts, dev + n, dev + 2 * n, dev + 3 * n, n, n, alpha, mid, m));
			}
			RES(zen_hip_resample_run_device(rs, mid, m, 0, m, m, 0, (size_t)k, out, n, 1));
			y.assign(n, 0.0f);
			ZEN(zen_hip_memcpy_d2h(y.data(), out, sizeof(float) * k));
			printf("%zu samples in, %zu stretched, %llu resampled, %zu out, %g semitones by %llu / %llu%s\n", n, m, k, n, semitones, num, den,
			       plain ? ", vocoder alone" : "");
		}
		// as zen-stretch: the engine's rows are at the scale of its transform, so the output is divided by its largest
		// magnitude where that would not fit 16 bits
		float peak = 0.0f;
		for (float v : y)
			peak = fabsf(v) > peak ? fabsf(v) : peak;
		if (peak > 1.0f)
			for (float& v : y)
				v = v / peak;
		zen::wav::encode_pcm16_mono(y, out_rate, outfile);
	};
	return zen::demo::run("zen-shift", body, [&] {
		zen_hip_resample_destroy(rs);
		zen_hip_tsm_destroy(ts);
		zen_hip_hpr_destroy(hpr);
		zen_hip_free(dev);
		zen_hip_free(mid);
		zen_hip_free(out);
	});
}
