// nmf_main.cpp -- zen_amd/bin/zen-nmf: learn a dictionary of spectra from a recording of one source, and separate a mixture
// with the dictionaries of its sources held fixed.
//
//   zen-nmf train in.wav -o dict.znmf [--nfft 2048] [--components 32] [--iterations 100] [--seed 0]
//   zen-nmf separate mix.wav -d a.znmf -d b.znmf ... -o prefix [--free K] [--iterations 100] [--seed 0]
//
// A file is mixed to mono as `zen offline` does, uploaded once and factorised by one zen_hip_nmf_process_device call; W
// starts from zen_hip_nmf_init(seed), H from seed + 1.  separate writes prefix_0.wav, prefix_1.wav, ... (one stem per
// dictionary, and one more for the --free components, which are learned on the mixture), each divided by its peak (a silent
// stem stays silent), as 16-bit PCM with cli/wav.h's rounding.  A recording of more than 16384 frames is refused.
//
// A .znmf file is little-endian: the four bytes "ZNMF", uint32 version (1), uint32 nfft, uint32 K, float32 fs, then K rows of
// nfft / 2 + 1 float32: the spectra.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "demo.h"
#include "wav.h"
#include "zen_hip.h"
#include "zen_hip_nmf.h"

using zen::demo::option;

namespace {

#define NMF(call) ZEN_LIB(zen_hip_nmf_last_error, call)

int usage()
{
	fprintf(stderr, "usage: zen-nmf train in.wav -o dict.znmf [--nfft N] [--components K] [--iterations I] [--seed S]\n"
	                "       zen-nmf separate mix.wav -d a.znmf [-d b.znmf ...] -o prefix [--free K] [--iterations I] [--seed S]\n"
	                "  N: the frame, a power of two in 64..8192 (default 2048); K: components, 1..256 in all (default 32; --free: 0); I: "
	                "iterations (default 100); S: the seed of the initial values (default 0)\n  train writes the dictionary learned from in.wav; "
	                "separate holds the dictionaries, learns the --free components on the mixture and writes prefix_0.wav ... one stem per "
	                "dictionary and one for the free components; at most 16384 frames of N / 2 samples\n");
	return 2;
}

struct Dictionary {
	uint32_t nfft = 0, K = 0;
	float fs = 0.f;
	std::vector<float> w; // K rows of nfft / 2 + 1
};

void write_le32(FILE* f, uint32_t v)
{
	const unsigned char b[4] = {(unsigned char)v, (unsigned char)(v >> 8), (unsigned char)(v >> 16), (unsigned char)(v >> 24)};
	if (fwrite(b, 1, 4, f) != 4)
		throw std::runtime_error("short write");
}

uint32_t read_le32(FILE* f, const std::string& path)
{
	unsigned char b[4];
	if (fread(b, 1, 4, f) != 4)
		throw std::runtime_error(path + " ends early");
	return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24;
}

uint32_t bits_of(float v)
{
	uint32_t u;
	memcpy(&u, &v, 4);
	return u;
}

float float_of(uint32_t u)
{
	float v;
	memcpy(&v, &u, 4);
	return v;
}

void save(const Dictionary& d, const std::string& path)
{
	FILE* f = fopen(path.c_str(), "wb");
	if (!f)
		throw std::runtime_error("cannot write " + path);
	try {
		if (fwrite("ZNMF", 1, 4, f) != 4)
			throw std::runtime_error("short write");
		write_le32(f, 1);
		write_le32(f, d.nfft);
		write_le32(f, d.K);
		write_le32(f, bits_of(d.fs));
		for (float v : d.w)
			write_le32(f, bits_of(v));
	} catch (...) {
		fclose(f);
		throw;
	}
	if (fclose(f) != 0)
		throw std::runtime_error("cannot write " + path);
}

Dictionary load(const std::string& path)
{
	FILE* f = fopen(path.c_str(), "rb");
	if (!f)
		throw std::runtime_error("cannot read " + path);
	Dictionary d;
	try {
		char magic[4];
		if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "ZNMF", 4) != 0 || read_le32(f, path) != 1)
			throw std::runtime_error(path + " is no .znmf file of version 1");
		d.nfft = read_le32(f, path);
		d.K = read_le32(f, path);
		d.fs = float_of(read_le32(f, path));
		const bool pow2 = d.nfft && !(d.nfft & (d.nfft - 1));
		if (!pow2 || d.nfft < 64 || d.nfft > 8192 || d.K < 1 || d.K > (uint32_t)ZEN_HIP_NMF_MAX_COMPONENTS)
			throw std::runtime_error(path + ": frame or components out of range");
		d.w.resize((size_t)d.K * (d.nfft / 2 + 1));
		for (float& v : d.w) {
			v = float_of(read_le32(f, path));
			if (!(v >= 0.0f) || !std::isfinite(v))
				throw std::runtime_error(path + ": a spectrum that is negative or not finite");
		}
	} catch (...) {
		fclose(f);
		throw;
	}
	fclose(f);
	return d;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc < 2 || (strcmp(argv[1], "train") && strcmp(argv[1], "separate")))
		return usage();
	const bool train = !strcmp(argv[1], "train");
	std::string infile, outname;
	std::vector<std::string> dict_files;
	size_t nfft = 2048, components = train ? 32 : 0;
	unsigned long long seed = 0;
	long iterations = 100;
	for (int i = 2; i < argc; ++i) {
		if (!strcmp(argv[i], "-o") && i + 1 < argc) {
			outname = argv[++i];
		} else if (!strcmp(argv[i], "-d") && i + 1 < argc && !train) {
			dict_files.push_back(argv[++i]);
		} else if (!strcmp(argv[i], "--nfft") && i + 1 < argc && train) {
			if (!option(argv[++i], &nfft))
				return usage();
		} else if (!strcmp(argv[i], train ? "--components" : "--free") && i + 1 < argc) {
			if (!option(argv[++i], &components))
				return usage();
		} else if (!strcmp(argv[i], "--iterations") && i + 1 < argc) {
			if (!option(argv[++i], &iterations) || iterations < 0 || iterations > 1000000)
				return usage();
		} else if (!strcmp(argv[i], "--seed") && i + 1 < argc) {
			if (!option(argv[++i], &seed))
				return usage();
		} else if (argv[i][0] == '-' || !infile.empty()) {
			return usage();
		} else {
			infile = argv[i];
		}
	}
	if (infile.empty() || outname.empty() || (!train && dict_files.empty()))
		return usage();
	zen_hip_nmf_t nm = nullptr;
	float* dev = nullptr;
	const auto body = [&] {
		int rate = 0;
		const std::vector<float> mono = zen::demo::load_mono(infile, &rate);
		if (mono.empty())
			throw std::runtime_error("no samples in " + infile);
		const size_t n = mono.size();
		std::vector<Dictionary> dicts;
		size_t fixed = 0;
		for (const std::string& p : dict_files) {
			dicts.push_back(load(p));
			if (dicts.back().nfft != dicts[0].nfft)
				throw std::runtime_error(p + ": the dictionaries differ in their frame");
			fixed += dicts.back().K;
		}
		if (!train)
			nfft = dicts[0].nfft;
		const size_t K = fixed + components, F = nfft / 2 + 1, hop = nfft / 2;
		ZEN(zen_hip_init(0));
		NMF(zen_hip_nmf_create((float)rate, nfft, K, 1, n, &nm));
		const size_t m = (n + hop - 1) / hop + 1;
		std::vector<float> w(K * F), hm(K * m);
		std::vector<int> groups(K);
		NMF(zen_hip_nmf_init(seed, components * F, w.data() + fixed * F)); // the learned spectra, behind the held ones
		NMF(zen_hip_nmf_init(seed + 1, hm.size(), hm.data()));
		size_t k0 = 0;
		for (size_t d = 0; d < dicts.size(); ++d) {
			std::copy(dicts[d].w.begin(), dicts[d].w.end(), w.begin() + k0 * F);
			for (size_t k = 0; k < dicts[d].K; ++k)
				groups[k0 + k] = (int)d;
			k0 += dicts[d].K;
		}
		for (size_t k = k0; k < K; ++k)
			groups[k] = (int)dicts.size();
		const size_t G = train ? 0 : dicts.size() + (components ? 1 : 0);
		// the clip, W, H and the stems in one allocation, every part on a 16-byte boundary
		auto up4 = [](size_t v) { return (v + 3) & ~(size_t)3; };
		const size_t o_w = up4(n), o_h = o_w + up4(K * F), o_s = o_h + up4(K * m), total = o_s + G * up4(n);
		ZEN(zen_hip_malloc((void**)&dev, sizeof(float) * total));
		ZEN(zen_hip_memcpy_h2d(dev, mono.data(), sizeof(float) * n));
		ZEN(zen_hip_memcpy_h2d(dev + o_w, w.data(), sizeof(float) * w.size()));
		ZEN(zen_hip_memcpy_h2d(dev + o_h, hm.data(), sizeof(float) * hm.size()));
		NMF(zen_hip_nmf_process_device(nm, dev, n, n, dev + o_w, F, K * F, dev + o_h, m, K * m, fixed, (int)iterations, train ? nullptr : groups.data(),
		                               G, dev + o_s, up4(n)));
		if (train) {
			Dictionary d;
			d.nfft = (uint32_t)nfft;
			d.K = (uint32_t)K;
			d.fs = (float)rate;
			d.w.resize(K * F);
			ZEN(zen_hip_memcpy_d2h(d.w.data(), dev + o_w, sizeof(float) * d.w.size()));
			save(d, outname);
			printf("frames: %zu, %zu spectra of %zu bins after %ld iterations\n", m, K, F, iterations);
		} else {
			for (size_t g = 0; g < G; ++g) {
				std::vector<float> stem(n);
				ZEN(zen_hip_memcpy_d2h(stem.data(), dev + o_s + g * up4(n), sizeof(float) * n));
				zen::demo::peak_normalise(stem);
				zen::wav::encode_pcm16_mono(stem, rate, outname + "_" + std::to_string(g) + ".wav");
			}
			printf("frames: %zu, %zu spectra held and %zu learned, %zu stems after %ld iterations\n", m, fixed, components, G, iterations);
		}
	};
	return zen::demo::run("zen-nmf", body, [&] {
		zen_hip_nmf_destroy(nm);
		zen_hip_free(dev);
	});
}
