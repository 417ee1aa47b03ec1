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
 * Packed 24-bit samples (three little-endian bytes, as a WAV file holds them) go through the same steps on the scale 2^23:
 *   PCM24 -> float : (float)v / 8388608.f, exact for every code       (wav.h:80-86)
 *   float -> PCM24 : x * 8388608.f rounded as above, saturated to [-8388608, 8388607], NaN -> 0.  The multiplier is the
 *                    reader's divisor (as 32767 is for 16 bits), so every code k survives k / 2^23 and back.
 * pcm24_load / pcm24_store move the three bytes one at a time: a packed sample has no alignment.
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
enum { ZEN_PCM_FMT_I16 = 0, ZEN_PCM_FMT_I24 = 1 }; /* 2 and 3 bytes per sample, little-endian, packed */

/* bytes of one sample; 0 for a format that does not exist */
ZEN_PCM_FN int pcm_sample_bytes(int fmt)
{
	return fmt == ZEN_PCM_FMT_I16 ? 2 : fmt == ZEN_PCM_FMT_I24 ? 3 : 0;
}

ZEN_PCM_FN float pcm16_to_float(int16_t s)
{
	return (float)s / 32767.f;
}

ZEN_PCM_FN float stereo_to_mono(int16_t l, int16_t r)
{
	return (pcm16_to_float(l) + pcm16_to_float(r)) / 2.0f;
}

/* v rounded to the nearest integer, halves away from zero, saturated to [lo, hi] (both integers whose neighbours lo - 1 and
 * hi + 1 are binary32 values too); NaN -> 0.  Not floorf(v + 0.5f): in binary32 0.49999997f + 0.5f is 1.0f.  trunc and the
 * remainder v - trunc(v) are both exact.  The clamp in front keeps trunc finite and the cast in range. */
ZEN_PCM_FN int32_t pcm_round_sat(float v, float lo, float hi)
{
	float t, d;
	if (!(v == v))
		return 0;
	v = fminf(fmaxf(v, lo - 1.0f), hi + 1.0f); /* infinities and everything that clips anyway */
	t = truncf(v);
	d = v - t;
	if (d >= 0.5f)
		t += 1.0f;
	else if (d <= -0.5f)
		t -= 1.0f;
	if (t > hi)
		t = hi;
	if (t < lo)
		t = lo;
	return (int32_t)t;
}

ZEN_PCM_FN int16_t pcm16_round_sat(float v)
{
	return (int16_t)pcm_round_sat(v, -32768.f, 32767.f);
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

/* ---- packed 24-bit samples ---------------------------------------------------------------------------------------- */
ZEN_PCM_FN int32_t pcm24_load(const uint8_t* p)
{
	const int32_t u = (int32_t)p[0] | ((int32_t)p[1] << 8) | ((int32_t)p[2] << 16); /* 0 .. 2^24 - 1 */
	return (u ^ 0x800000) - 0x800000;                                                /* the sign bit, without a shift */
}

ZEN_PCM_FN void pcm24_store(uint8_t* p, int32_t v)
{
	const uint32_t u = (uint32_t)v; /* modulo 2^32: the low three bytes are the code */
	p[0] = (uint8_t)(u & 255u);
	p[1] = (uint8_t)((u >> 8) & 255u);
	p[2] = (uint8_t)((u >> 16) & 255u);
}

ZEN_PCM_FN float pcm24_to_float(int32_t v)
{
	return (float)v / 8388608.f;
}

ZEN_PCM_FN float pcm24_stereo_to_mono(int32_t l, int32_t r)
{
	return (pcm24_to_float(l) + pcm24_to_float(r)) / 2.0f;
}

ZEN_PCM_FN int32_t pcm24_round_sat(float v)
{
	return pcm_round_sat(v, -8388608.f, 8388607.f);
}

ZEN_PCM_FN int32_t float_to_pcm24(float x)
{
	const float v = x * 8388608.f;
	return pcm24_round_sat(v);
}

ZEN_PCM_FN int32_t float_to_pcm24_peak(float y, float peak)
{
	float x;
	if (peak == 0.f)
		return 0;
	x = y / peak;
	return float_to_pcm24(x);
}

ZEN_PCM_FN int32_t float_to_pcm24_gain(float y, float gain)
{
	const float v = y * gain;
	return pcm24_round_sat(v);
}

#endif /* ZEN_PCM_CONVERT_H */
