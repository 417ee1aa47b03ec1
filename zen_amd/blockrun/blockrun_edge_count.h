// blockrun_edge_count.h -- the 24 percussive mask bits of the run kernel that lie outside blocks 0 .. 127 of the median
// stage (bin N/2 and the bins N - 23 .. N - 1), by counting instead of selecting.
//
// The consumer of the median P[k] of these bins is the hard mask alone: hard_mask_exact(P[k], d, thr) with
// d = mag[k] + FLT_EPSILON, that is [(double)P[k] > t] for t = thr * (double)d.  P[k] is the 24th smallest of the 47 keys of
// its window, keys being the magnitudes' bit patterns ordered as signed integers (median47_core.h).
//   - Let f* be the smallest float whose double value exceeds t (t >= 0: thr >= 0, d > 0 or NaN).  For a key M that is not a
//     NaN pattern above key(+inf): (double)M > t  <=>  M >= f*  <=>  key(M) >= key(f*): non-negative floats order like
//     their bits, and a key with the sign bit (a -0 or a NaN with it: a negative integer) is below every key(f*) >= 1 and
//     fails (double)M > t >= 0 as well.  f* = fl(t) if that exceeds t, else the next float up; +inf is a valid f*
//     (t above FLT_MAX).  t = +inf or NaN has no f*: the mask is 0 whatever the median is.
//   - The 24th smallest of 47 keys is >= K exactly when at least 24 of them are (at most 23 are below K).
//   - The median is a NaN pattern above key(+inf) exactly when at least 24 keys are; (double)NaN > t is false.
// So the bit is [#{keys >= key(f*)} >= 24] and not [#{keys > key(+inf)} >= 24]; the second count is only taken when some key
// of the windows is above key(+inf) at all (wave-uniform).  "No f*" is the key 0x7fffffff: the keys that reach it are NaN
// patterns, which the second count removes.
//
// The windows, from the image as FwdOut and the border loop leave it (column c of the bordered Hermitian row):
//   - bin N - j, j = 1 .. 23: columns N - j - 23 .. N - 1 are the mirrors of mag[1 .. j + 23], columns N .. N - j + 23 are
//     24 - j border replicas of column N - 1 = mag[1]: the keys mag[1 .. j + 23] once each and 24 - j more copies of mag[1].
//     d comes from mag[j].
//   - bin N/2: columns N/2 - 23 .. N/2 + 23 = mag[N/2 - 23 .. N/2 - 1], mag[N/2], and the mirrors of the former: with
//     c = #{mag[N/2 - 23 .. N/2 - 1] >= K} and b = [mag[N/2] >= K] the count is 2c + b, and 2c + b >= 24 <=> c >= 12
//     (c = 12 gives 24 or 25, c = 11 gives 22 or 23).
//
// Layout: one lane per KEY, not per output.  Lane l of the wave holds a = mag[l] and b = mag[N/2 - l]; the threshold key of
// output j (j = 0: bin N/2, else bin N - j) is computed in lane j from mag[j] resp. mag[N/2], broadcast with a
// v_readlane, compared in all lanes at once, and the compare mask is cut to the window's lanes and counted on the scalar
// unit.  Per output that is two vector instructions; the lane-per-output layout needs two per KEY and output
// (DESIGN 14 has both counts).
//
// The decision logic (edge_threshold_key, edge_count_reaches, edge_count_bits) is plain C++ and is what
// tests/cpp/test_blockrun_edge_count_host.cpp runs on the CPU against znet::medians and hard_mask_exact, with a wave of
// arrays in place of EdgeWave.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>

#pragma clang fp contract(off)

namespace zen_blockrun {

constexpr int EDGE_OUTPUTS = 24;             // output 0: bin N/2; output j: bin N - j
constexpr int EDGE_KEY_INF = 0x7f800000;     // keys above it are NaN patterns
constexpr int EDGE_KEY_NONE = 0x7fffffff;    // "no f*"
constexpr int EDGE_IMG_COL0 = 24, EDGE_IMG_RSTR = 20; // the image of median47_core.h: column k at word k + 24, 16-word chunks 20 apart
constexpr unsigned long long EDGE_LANES_A = (2ull << 46) - 2; // lanes 1 .. 46: mag[1 .. 46], every key of the 23 tail windows
constexpr unsigned long long EDGE_LANES_B = (2ull << 23) - 2; // lanes 1 .. 23: mag[N/2 - 1 .. N/2 - 23]

__device__ __forceinline__ int edge_img_addr(int col)
{
	const int g = col + EDGE_IMG_COL0;
	return (g >> 4) * EDGE_IMG_RSTR + (g & 15);
}

__device__ __forceinline__ int edge_bits_of(float f)
{
	int i;
	memcpy(&i, &f, sizeof(i));
	return i;
}
__device__ __forceinline__ float edge_float_of(int i)
{
	float f;
	memcpy(&f, &i, sizeof(f));
	return f;
}

// key(f*) for the bin whose magnitude has the bits mag_key: the smallest float above t = thr * (double)(mag + FLT_EPSILON),
// the product hard_mask_exact forms (thr >= 0)
__device__ __forceinline__ int edge_threshold_key(double thr, int mag_key)
{
	const float d = edge_float_of(mag_key) + FLT_EPSILON;
	const double t = thr * (double)d;
	const float r = (float)t; // round to nearest: r or its successor is f* (r = +inf for t above FLT_MAX's rounding boundary)
	const int kr = edge_bits_of(r);
	const int k = (double)r > t ? kr : (int)((unsigned)kr + 1u); // (a NaN's bits may wrap: replaced below)
	return t < (double)INFINITY ? k : EDGE_KEY_NONE; // (false for NaN too)
}

// does the count of window keys in the compare mask m (one bit per lane: key >= K) reach the middle of the window of output j?
__device__ __forceinline__ bool edge_count_reaches(unsigned long long m, int j)
{
	if (j == 0) // 2c + b >= 24 <=> c >= 12 (above)
		return __builtin_popcountll(m & EDGE_LANES_B) >= 12;
	const unsigned long long lanes = (2ull << (j + 23)) - 2; // mag[1 .. j + 23]
	return __builtin_popcountll(m & lanes) + (24 - j) * (int)((m >> 1) & 1) >= 24;
}

// Wave: ge(from_b, K) = the mask of lanes whose key (b if from_b, else a) is >= K as signed integers;
//       threshold(j)  = lane j's threshold key.
// Returns bit j = the mask of output j.
template <class Wave>
__device__ __forceinline__ unsigned edge_count_bits(const Wave& w)
{
	unsigned bits = 0;
#pragma unroll
	for (int j = 0; j < EDGE_OUTPUTS; ++j)
		bits |= (unsigned)edge_count_reaches(w.ge(j == 0, w.threshold(j)), j) << j;
	const unsigned long long na = w.ge(false, EDGE_KEY_INF + 1), nb = w.ge(true, EDGE_KEY_INF + 1);
	if (((na & EDGE_LANES_A) | (nb & EDGE_LANES_B)) != 0) { // some key is a NaN pattern: the medians that are NaN give 0
#pragma unroll
		for (int j = 0; j < EDGE_OUTPUTS; ++j)
			bits &= ~((unsigned)edge_count_reaches(j == 0 ? nb : na, j) << j);
	}
	return bits;
}

#if defined(__HIPCC__) // (not where the header is compiled as plain C++)
// one wave of the kernel: a, b the lane's two keys, k its threshold key
struct EdgeWave {
	int a, b, k;
	__device__ __forceinline__ unsigned long long ge(bool from_b, int K) const { return __builtin_amdgcn_ballot_w64((from_b ? b : a) >= K); }
	__device__ __forceinline__ int threshold(int j) const { return __builtin_amdgcn_readlane(k, j); }
};

// Called by all 64 lanes of one wave once the image's lower half is complete.  Returns the 24 bits (uniform).
__device__ __forceinline__ unsigned edge_count_wave(const int* img, int lane, double thr, int n_half)
{
	EdgeWave w;
	w.a = img[edge_img_addr(lane)];
	w.b = img[edge_img_addr(n_half - lane)];
	w.k = edge_threshold_key(thr, lane == 0 ? w.b : w.a);
	return edge_count_bits(w);
}
#endif

} // namespace zen_blockrun
