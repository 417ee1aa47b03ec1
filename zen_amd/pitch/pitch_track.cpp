// pitch_track.cpp -- zen_amd/bin/pitch-track: the pitch of a recording chunk by chunk, with and without harmonic separation
// in front of the tracker (the counterpart of the reference's demos/pitch-tracking).
//
//   pitch-track in.wav [--chunk 4096] [--beta 2.5]
//
// The file is mixed to mono as `zen` does, uploaded once, and stays on the device: one zen_hip_hpr_process call (causal,
// hop = chunk, harmonic output) writes the harmonic stream behind the input, one zen_hip_pitch_run_device call tracks both
// rows.  Only the two pitch rows come back.  One line per whole chunk: t (seconds, the start of the chunk) and both pitches
// in Hz, -1 where the tracker found none.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "demo.h"
#include "wav.h"
#include "zen_hip.h"
#include "zen_hip_pitch.h"

using zen::demo::option;

namespace {

#define PITCH(call) ZEN_LIB(zen_hip_pitch_last_error, call)

int usage()
{
	fprintf(stderr, "usage: pitch-track in.wav [--chunk N] [--beta B]\n  N: a power of two, 32..8192 (default 4096); B: separation factor (default 2.5)\n");
	return 2;
}

} // namespace

int main(int argc, char** argv)
{
	std::string infile;
	size_t chunk = 4096;
	float beta = 2.5f;
	for (int i = 1; i < argc; ++i) {
		if (!strcmp(argv[i], "--chunk") && i + 1 < argc) {
			if (!option(argv[++i], &chunk))
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
	if (infile.empty())
		return usage();
	zen_hip_hpr_t hpr = nullptr;
	zen_hip_pitch_t pt = nullptr;
	float *dev = nullptr, *out = nullptr;
	const auto body = [&] {
		int rate = 0;
		const std::vector<float> mono = zen::demo::load_mono(infile, &rate);
		const size_t n_chunks = mono.size() / chunk, len = n_chunks * chunk;
		const float fs = (float)rate;
		ZEN(zen_hip_init(0));
		PITCH(zen_hip_pitch_create(fs, chunk, 2, 0, &pt)); // stream 0: the recording, stream 1: its harmonic part
		ZEN(zen_hip_hpr_create(fs, chunk, beta, ZEN_HIP_OUTPUT_HARMONIC, ZEN_HIP_TIME_CAUSAL, 1, 1, 0, &hpr));
		if (n_chunks) {
			ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * 2 * len));
			ZEN(zen_hip_malloc((void**)&out, sizeof(float) * 2 * n_chunks));
			ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * len));
			ZEN(zen_hip_hpr_process(hpr, dev, n_chunks, len, dev + len, nullptr, nullptr, len));
			PITCH(zen_hip_pitch_run_device(pt, dev, len, n_chunks, chunk, out, nullptr, nullptr, nullptr, n_chunks));
			std::vector<float> pitch(2 * n_chunks);
			ZEN(zen_hip_memcpy_d2h(pitch.data(), out, sizeof(float) * 2 * n_chunks));
			for (size_t c = 0; c < n_chunks; ++c)
				printf("t: %.3f,\tpitch (+HPR): %.2f,\tpitch (-HPR): %.2f\n", (double)(c * chunk) / (double)fs, (double)pitch[n_chunks + c],
				       (double)pitch[c]);
		}
	};
	return zen::demo::run("pitch-track", body, [&] {
		zen_hip_pitch_destroy(pt);
		zen_hip_hpr_destroy(hpr);
		zen_hip_free(dev);
		zen_hip_free(out);
	});
}
