// multi_stems.cpp -- zen_amd/bin/zen-stems: the harmonic and the percussive stem of a recording, with its channels kept.
//
//   zen-stems in.wav [-o prefix] [--hps hop_h beta_h hop_p beta_p] [--soft-mask] [--sse]
//
// What `zen offline` does to the mono mix, done to every channel: the file's frames go up as 16-bit samples, one
// zen_hip_multi_offline_host call separates all channels (PCM16 out, PEAK mode: one peak per stem over all its channels, so
// a stem keeps the balance between them), and prefix_harm.wav and prefix_perc.wav come out with the input's channel
// count.  A mono file gives the samples `zen offline` writes.  Files of other encodings than PCM16 are rounded to 16 bits
// on the way in.
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
#include "zen_hip_multi.h"

namespace {

#define MULTI(call) ZEN_LIB(zen_hip_multi_last_error, call)

int usage()
{
	fprintf(stderr, "usage: zen-stems in.wav [-o prefix] [--hps hop_h beta_h hop_p beta_p] [--soft-mask] [--sse]\n"
	                "  writes prefix_harm.wav and prefix_perc.wav (default prefix: the input without .wav) with the input's channels (1..%d),\n"
	                "  PCM16, each stem normalised by one peak over all its channels; default --hps 4096 2.0 256 2.0\n",
	        (int)ZEN_HIP_MULTI_MAX_CHANNELS);
	return 2;
}

bool number(const char* s, double* v)
{
	char* end = nullptr;
	*v = strtod(s, &end);
	return end != s && *end == '\0';
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile, prefix;
	double hop_h = 4096, beta_h = 2.0, hop_p = 256, beta_p = 2.0;
	bool soft = false, sse = false;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			prefix = argv[++i];
		} else if (!strcmp(argv[i], "--hps") && i + 4 < argc) {
			if (!number(argv[i + 1], &hop_h) || !number(argv[i + 2], &beta_h) || !number(argv[i + 3], &hop_p) || !number(argv[i + 4], &beta_p))
				return usage();
			i += 4;
		} else if (!strcmp(argv[i], "--soft-mask")) {
			soft = true;
		} else if (!strcmp(argv[i], "--sse")) {
			sse = true;
		} else if (argv[i][0] == '-' || !infile.empty()) {
			return usage();
		} else {
			infile = argv[i];
		}
	}
	const double max_hop = 1 << 20; // far above what the engines accept; the casts below stay defined
	if (infile.empty() || !(hop_h >= 1 && hop_h <= max_hop) || !(hop_p >= 1 && hop_p <= max_hop))
		return usage();
	if (prefix.empty()) {
		prefix = infile;
		if (prefix.size() > 4 && prefix.compare(prefix.size() - 4, 4, ".wav") == 0)
			prefix.resize(prefix.size() - 4);
	}
	zen_hip_multi_offline_t h = nullptr;
	const auto body = [&] {
		zen::wav::AudioData fd;
		zen::wav::load(fd, infile);
		if (fd.channelCount > ZEN_HIP_MULTI_MAX_CHANNELS)
			throw std::runtime_error(infile + ": " + std::to_string(fd.channelCount) + " channels; zen-stems separates at most " +
			                         std::to_string((int)ZEN_HIP_MULTI_MAX_CHANNELS));
		if (fd.channelCount < 1)
			throw std::runtime_error(infile + ": no channels");
		const int C = fd.channelCount;
		const size_t n_frames = fd.samples.size() / (size_t)C;
		std::vector<int16_t> in(n_frames * C), harm(n_frames * C), perc(n_frames * C);
		for (size_t i = 0; i < in.size(); ++i) { // exact for a PCM16 file: wav.h read s / 32767.f
			const float v = fd.samples[i] * 32767.f;
			in[i] = (int16_t)(v >= 32767.f ? 32767 : v <= -32768.f ? -32768 : lroundf(v));
		}
		float peaks[2] = {0.f, 0.f};
		ZEN(zen_hip_init(0));
		MULTI(zen_hip_multi_offline_create((float)fd.sampleRate, (size_t)hop_h, (size_t)hop_p, (float)beta_h, (float)beta_p, 0, C, &h));
		if (sse)
			MULTI(zen_hip_multi_offline_use_sse_filter(h));
		if (soft)
			MULTI(zen_hip_multi_offline_use_soft_mask(h));
		MULTI(zen_hip_multi_offline_host(h, ZEN_HIP_MULTI_I16, in.data(), n_frames, harm.data(), perc.data(), ZEN_HIP_MULTI_PEAK, 0.f, peaks));
		zen::wav::encode_pcm16_interleaved(harm, C, fd.sampleRate, prefix + "_harm.wav");
		zen::wav::encode_pcm16_interleaved(perc, C, fd.sampleRate, prefix + "_perc.wav");
		printf("%zu frames of %d channels at %d Hz -> %s_harm.wav (peak %g), %s_perc.wav (peak %g)\n", n_frames, C, fd.sampleRate, prefix.c_str(),
		       (double)peaks[0], prefix.c_str(), (double)peaks[1]);
	};
	return zen::demo::run("zen-stems", body, [&] {
		zen_hip_multi_offline_destroy(h);
	});
}
