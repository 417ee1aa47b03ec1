// beat_track.cpp -- zen_amd/bin/beat-track: the beats of a recording, with and without percussive separation in front of the
// tracker (the counterpart of the reference's demos/beat-tracking).
//
//   beat-track in.wav [--hop 512] [--hpr-hop 1024] [--beta 2.5]
//
// The file is mixed to mono as `zen` does, cut to a multiple of both hops, uploaded once, and stays on the device: one
// zen_hip_hpr_process call (causal, percussive output) writes the percussive stream behind the input, one
// zen_hip_beat_run_device call tracks both rows.  Only the two beat rows come back.  Two lines: the seconds (hop index *
// hop / fs) of the hops with a beat, with and without the separation.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "demo.h"
#include "wav.h"
#include "zen_hip.h"
#include "zen_hip_beat.h"

using zen::demo::option;

namespace {

#define BEAT(call) ZEN_LIB(zen_hip_beat_last_error, call)

int usage()
{
	fprintf(stderr, "usage: beat-track in.wav [--hop N] [--hpr-hop M] [--beta B]\n  N: the tracker's hop, a power of two in 64..2048 (default 512); "
	                "M: the separation's hop (default 1024); B: separation factor (default 2.5)\n");
	return 2;
}

void print_beats(const char* title, const float* beat, size_t n_hops, size_t hop, double fs)
{
	printf("%s beat timestamps: ", title);
	for (size_t t = 0; t < n_hops; ++t)
		if (beat[t] > 0.0f)
			printf("%.4f ", (double)(t * hop) / fs);
	printf("\n");
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile;
	size_t hop = 512, hpr_hop = 1024;
	float beta = 2.5f;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "--hop") && i + 1 < argc) {
			if (!option(argv[++i], &hop))
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
	if (infile.empty() || hop == 0 || hpr_hop == 0)
		return usage();
	zen_hip_hpr_t hpr = nullptr;
	zen_hip_beat_t bt = nullptr;
	float *dev = nullptr, *out = nullptr;
	const auto body = [&] {
		int rate = 0;
		std::vector<float> mono = zen::demo::load_mono(infile, &rate);
		const size_t unit = hop > hpr_hop ? hop : hpr_hop;
		if (unit % hop || unit % hpr_hop)
			throw std::runtime_error("one hop must be a multiple of the other");
		const size_t len = mono.size() / unit * unit, n_hops = len / hop;
		const float fs = (float)rate;
		ZEN(zen_hip_init(0));
		BEAT(zen_hip_beat_create(fs, hop, 2, 0, &bt)); // stream 0: the recording, stream 1: its percussive part
		ZEN(zen_hip_hpr_create(fs, hpr_hop, beta, ZEN_HIP_OUTPUT_PERCUSSIVE, ZEN_HIP_TIME_CAUSAL, 1, 1, 0, &hpr));
		std::vector<float> beat(2 * n_hops);
		if (n_hops) {
			ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * 2 * len));
			ZEN(zen_hip_malloc((void**)&out, sizeof(float) * 2 * n_hops));
			ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * len));
			ZEN(zen_hip_hpr_process(hpr, dev, len / hpr_hop, len, nullptr, dev + len, nullptr, len));
			BEAT(zen_hip_beat_run_device(bt, dev, len, n_hops, nullptr, nullptr, out, nullptr, n_hops));
			ZEN(zen_hip_memcpy_d2h(beat.data(), out, sizeof(float) * 2 * n_hops));
		}
		print_beats("+HPR", beat.data() + n_hops, n_hops, hop, (double)fs);
		print_beats("-HPR", beat.data(), n_hops, hop, (double)fs);
	};
	return zen::demo::run("beat-track", body, [&] {
		zen_hip_beat_destroy(bt);
		zen_hip_hpr_destroy(hpr);
		zen_hip_free(dev);
		zen_hip_free(out);
	});
}
