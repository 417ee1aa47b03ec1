/* pcm_convert.h -- the sample-format arithmetic of libzen_hip_pcm.so, as inline functions that compile for the host (C99 or
 * C++) and for the device, so that the CPU tier tests the very code the kernels of pcm_kernels.hip run.
 *
 * The formulas are the ones zen_amd/cli/wav.h applies on the host, one sample at a time:
 *   PCM16 -> float : (float)s / 32767.f, an IEEE division            (wav.h:77-78)
 *   stereo -> mono : (L + R) / 2.0f on the widened samples            (wav.h:101-105)
 *   float -> PCM16 : lroundf(x * 32767.f), halves away from zero      (wav.h:130-132)
 * with ONE difference on the way out: wav.h casts the rounded long to int16_t, which wraps modulo 2^16 when
 * |x * 32767| >= 32767.5; float_to_pcm16 SATURATES to [-32768, 32767] instead, and turns NaN into 0.  For every sample with
 * |x * 32767| < 32767.5 the two agree bit for bit.
 *
 * Every product and quotient below is rounded to binary32 on its own.  Files that include this header are compiled with
 * -ffp-contract=off and without any fast-math flag (zen_amd/addon_build.py); the pragma below says the same to clang.
 */
#ifndef ZEN_PCM_CONVERT_H
#define ZEN_PCM_CONVERT_H

#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define ZEN_PCM_FN __host__ __device__ static inline
#else
#define ZEN_PCM_FN static inline
#endif

enum { ZEN_PCM_MODE_PEAK = 0, ZEN_PCM_MODE_GAIN = 1 };

ZEN_PCM_FN float pcm16_to_float(int16_t s)
{
	return (float)s / 32767.f;
}

ZEN_PCM_FN float stereo_to_mono(int16_t l, int16_t r)
{
	return (pcm16_to_float(l) + pcm16_to_float(r)) / 2.0f;
}

/* v rounded to the nearest integer, halves away from zero, saturated to int16; NaN -> 0.  Not floorf(v + 0.5f): in
 * binary32 0.49999997f + 0.5f is 1.0f.  trunc and the remainder v - trunc(v) are both exact. */
ZEN_PCM_FN int16_t pcm16_round_sat(float v)
{
	float t, d;
	if (!(v == v))
		return 0;
	v = fminf(fmaxf(v, -32769.f), 32768.f); /* infinities and everything that clips anyway: trunc stays finite */
	t = truncf(v);
	d = v - t;
	if (d >= 0.5f)
		t += 1.0f;
	else if (d <= -0.5f)
		t -= 1.0f;
	if (t > 32767.f)
		t = 32767.f;
	if (t < -32768.f)
		t = -32768.f;
	return (int16_t)(int)t;
}

ZEN_PCM_FN int16_t float_to_pcm16(float x)
{
	const float v = x * 32767.f;
	return pcm16_round_sat(v);
}

/* max(-min, max) of the whole output: what peak_normalise (zen_amd/cli/main.cpp:86-92) divides by */
ZEN_PCM_FN float pcm16_peak_of(float mn, float mx)
{
	const float a = -1 * mn;
	return a < mx ? mx : a; /* std::max(a, mx), the sign of a zero included */
}

/* PEAK: peak_normalise followed by the encoder -- two roundings, the division first.  peak == 0 (an all-silent output, where
 * the command line tool divides 0 by 0 and encodes the NaN) gives zeros. */
ZEN_PCM_FN int16_t float_to_pcm16_peak(float y, float peak)
{
	float x;
	if (peak == 0.f)
		return 0;
	x = y / peak;
	return float_to_pcm16(x);
}

/* GAIN: one rounding, y * gain in place of x * 32767; saturation is what protects a stream that cannot know its peak */
ZEN_PCM_FN int16_t float_to_pcm16_gain(float y, float gain)
{
	const float v = y * gain;
	return pcm16_round_sat(v);
}

#endif /* ZEN_PCM_CONVERT_H */
