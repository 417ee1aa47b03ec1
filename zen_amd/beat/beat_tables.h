// beat_tables.h -- the host tables of libzen_hip_beat.so (zen_hip_beat.h): everything transcendental
// of the method, computed once per (fs, hop) in double with libm and rounded once to float32.  tests/beat_model.py computes
// the same values with Python's math module -- the same libm calls, operation for operation (the file is compiled with
// contraction off, as all of the library).  Host code only.
#pragma once

#include <cmath>
#include <cstddef>
#include <vector>

namespace zen_beat {

constexpr int TEMPI = 41, HISTORY = 512, MAX_PERIOD = 128;
constexpr int W1_ROW = 2 * MAX_PERIOD, W2_ROW = MAX_PERIOD; // floats per period in the device tables

inline int r2_of(int b) { return 2 * b; }
inline int rh_of(int b) { return (b + 1) / 2; } // floor(b / 2 + 0.5)

// offsets (in floats) of the device copy: transition | rayleigh | tempo | period | past [129][256] | future [129][128] | window [N]
constexpr size_t OFF_TRANS = 0, OFF_RAYLEIGH = OFF_TRANS + TEMPI * TEMPI, OFF_TEMPO = OFF_RAYLEIGH + 128, OFF_PERIOD = OFF_TEMPO + TEMPI,
                 OFF_PAST = OFF_PERIOD + TEMPI, OFF_FUTURE = OFF_PAST + (size_t)(MAX_PERIOD + 1) * W1_ROW,
                 OFF_WINDOW = OFF_FUTURE + (size_t)(MAX_PERIOD + 1) * W2_ROW;

inline bool is_pow2(size_t x) { return x && (x & (x - 1)) == 0; }

// bp_j; false where create refuses (fs, hop)
inline bool periods(float fs, size_t hop, int bp[TEMPI])
{
	if (!is_pow2(hop) || hop < 64 || hop > 2048 || !(fs > 0.f) || !std::isfinite(fs))
		return false;
	for (int j = 0; j < TEMPI; ++j) {
		const double v = std::floor(60.0 * (double)fs / ((double)((80 + 2 * j) * (long)hop)) + 0.5);
		if (!(v >= 0.0 && v <= 1e6))
			return false;
		bp[j] = (int)v;
	}
	return bp[0] <= MAX_PERIOD && bp[TEMPI - 1] >= 4;
}

inline float window_at(size_t i, size_t n) { return (float)(0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)(n - 1))); }

inline float past_at(int b, int k)
{
	const double t = 5.0 * std::log((double)(2 * b - k) / (double)b);
	return (float)std::exp(-(t * t) / 2.0);
}

inline float future_at(int b, int n)
{
	const double h = (double)b / 2.0, d = (double)(n + 1) - h;
	return (float)std::exp(-(d * d) / (2.0 * (h * h)));
}

inline float rayleigh_at(int i)
{
	const double s2 = 43.0 * 43.0;
	return (float)(((double)i / s2) * std::exp(-(double)(i * i) / (2.0 * s2)));
}

inline float transition_at(int i, int j)
{
	const double sg = 41 / 8.0, d = (double)((i - j) * (i - j));
	return (float)(std::exp(-d / (2.0 * (sg * sg))) / (sg * std::sqrt(2.0 * M_PI)));
}

inline float tempo_at(float fs, size_t hop, int b) { return (float)(60.0 * (double)fs / ((double)((long)hop * b))); }

// the device copy; rows of the two weightings exist for the periods among bp only, the rest stays zero
inline std::vector<float> device_tables(float fs, size_t hop, const int bp[TEMPI])
{
	const size_t n = 2 * hop;
	std::vector<float> t(OFF_WINDOW + n, 0.0f);
	for (int i = 0; i < TEMPI; ++i)
		for (int j = 0; j < TEMPI; ++j)
			t[OFF_TRANS + i * TEMPI + j] = transition_at(i, j);
	for (int i = 0; i < 128; ++i)
		t[OFF_RAYLEIGH + i] = rayleigh_at(i);
	for (int j = 0; j < TEMPI; ++j) {
		const int b = bp[j];
		t[OFF_TEMPO + j] = tempo_at(fs, hop, b);
		t[OFF_PERIOD + j] = (float)b;
		for (int k = 0; k <= r2_of(b) - rh_of(b); ++k)
			t[OFF_PAST + (size_t)b * W1_ROW + k] = past_at(b, k);
		for (int m = 0; m < b; ++m)
			t[OFF_FUTURE + (size_t)b * W2_ROW + m] = future_at(b, m);
	}
	for (size_t i = 0; i < n; ++i)
		t[OFF_WINDOW + i] = window_at(i, n);
	return t;
}

} // namespace zen_beat
