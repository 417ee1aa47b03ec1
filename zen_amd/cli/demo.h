// demo.h -- the frame the demo programs of the add-on libraries share (zen_amd/bin/pitch-track ... zen-shift; not the `zen`
// tool): the return-code check, the option parsers, the recording as a mono row, the stems' normalisation and the tail of
// main -- the body's exception, the release of the handles, the memory check.  Header-only, plain C++17 beside wav.h; each
// program keeps its usage text, its option loop and its body.
#ifndef ZG_CLI_DEMO_H
#define ZG_CLI_DEMO_H

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "wav.h"
#include "zen_hip.h"

namespace zen {
namespace demo {

	inline void check(int rc, const char* what, const char* msg)
	{
		if (rc != ZEN_HIP_OK)
			throw std::runtime_error(std::string(what) + ": " + msg);
	}
// a call into libzen_hip.so, and one into an add-on library whose message `last_error` hands out
#define ZEN(call) zen::demo::check((call), #call, zen_hip_last_error())
#define ZEN_LIB(last_error, call) zen::demo::check((call), #call, last_error())

	// An option's value: the whole string has to be the number.  What strtoull, strtol, strtod and strtof take is taken,
	// the empty string (zero) and a sign in front of an unsigned value included; the programs check the range.
	inline bool option(const char* s, unsigned long long* v)
	{
		char* end = nullptr;
		*v = strtoull(s, &end, 10);
		return !*end;
	}
	inline bool option(const char* s, size_t* v)
	{
		unsigned long long u = 0;
		const bool ok = option(s, &u);
		*v = (size_t)u;
		return ok;
	}
	inline bool option(const char* s, long* v)
	{
		char* end = nullptr;
		*v = strtol(s, &end, 10);
		return !*end;
	}
	inline bool option(const char* s, double* v)
	{
		char* end = nullptr;
		*v = strtod(s, &end);
		return !*end;
	}
	inline bool option(const char* s, float* v)
	{
		char* end = nullptr;
		*v = strtof(s, &end);
		return !*end;
	}

	// the file mixed to mono as `zen offline` does
	inline std::vector<float> load_mono(const std::string& path, int* sample_rate)
	{
		wav::AudioData fd;
		wav::load(fd, path);
		*sample_rate = fd.sampleRate;
		if (fd.channelCount != 2)
			return fd.samples;
		std::vector<float> mono(fd.samples.size() / 2);
		wav::stereo_to_mono(fd.samples.data(), mono.data(), fd.samples.size());
		return mono;
	}

	inline void peak_normalise(std::vector<float>& x) // as `zen offline`; a stem of zeros is left as it is
	{
		auto limits = std::minmax_element(x.begin(), x.end());
		const float real_max = std::max(-1 * (*limits.first), *limits.second);
		if (!(real_max > 0.0f))
			return;
		for (float& v : x)
			v /= real_max;
	}

	// The tail of main: `body` throws what goes wrong (status 1, "<prog>: <what>"), `release` destroys the handles and
	// frees the device memory either way, and after a body that went well a red zone found overwritten is, as in `zen`, an
	// error of its own (status 86).
	template <class Body, class Release>
	int run(const char* prog, Body body, Release release)
	{
		int status = 0;
		try {
			body();
		} catch (const std::exception& e) {
			fprintf(stderr, "%s: %s\n", prog, e.what());
			status = 1;
		}
		release();
		if (status == 0) {
			zen_hip_memcheck_report rep;
			if (zen_hip_memcheck(&rep) == ZEN_HIP_OK && rep.corrupt_words) {
				fprintf(stderr, "%s: memory check: %s\n", prog, rep.first_message);
				status = 86;
			}
		}
		return status;
	}

} // namespace demo
} // namespace zen

#endif
