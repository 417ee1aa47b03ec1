// blockrun_first_pass.h -- the first pass of the run kernel's analysis transform as the real transform it is.
//
// Pass 0 of Plan<12> runs stages 1..4 of the radix-2 DIT DAG (fft_dev.h) on a thread's 16 values x[j + n * 256]: n >= 8 is
// the zero padding, n < 8 are real numbers (the windowed samples), so every thread computes a 16-point DFT of 8 real
// samples.  butterfly<16, false, true, true, TW> already skips stage 1 and the products with 1 and -i; this routine is the
// same DAG -- every product and every sum the same single IEEE operation on the same operands -- without
//   - the imaginary parts that are exact zeros: stage 2 and the groups 0 and 4 of stages 3 and 4 work on reals;
//   - (SYM) the outputs k = 9 .. 15 of a real input's transform, the conjugates of k = 7 .. 1: the groups 3, 6 and 7 of
//     stages 3 and 4 do the products of the groups 1, 2 and 5 with conjugated operands, and round-to-nearest is symmetric
//     in the sign -- PROVIDED the table has tw[N/8] == (c, -c) and tw[3N/16] == (-tw[N/16].y, -tw[N/16].x) bit for bit
//     (table_is_symmetric; the engine's table is built that way, csrc/api.hip make_twiddles).  Without it (!SYM) the
//     groups 3, 6 and 7 are computed as butterfly<> computes them.
// Every nonzero output has the bits of butterfly<>'s.  An exact zero may carry the other sign (as fft_dev.h allows for its
// own shortcuts); where butterfly<> forms 0 - x the routine does too (not -x), so that a zero that comes from zero or
// cancelling operands has butterfly<>'s sign in every case tests/cpp/test_blockrun_first_pass_host.cpp could construct
// from inputs that are not -0.
//
// Group numbering below: after stage q the 16 values are 2^q frequency groups c of 16 / 2^q sub-sequences m.
// Host test: tests/cpp/test_blockrun_first_pass_host.cpp (ZBR_FIRST_PASS_HOST_TEST) compiles this header and fft_dev.h as
// plain C++ behind tests/cpp/host_shim/hip/hip_runtime.h; PK = false is the scalar form of the same operations.
#pragma once
#include "../csrc/fft_dev.h"

#pragma clang fp contract(off)

namespace zen_blockrun {

// the two identities of the table the conjugate shortcut relies on; tw = the N/2 entries of an N-point transform's table
inline bool table_is_symmetric(const float* tw, int n)
{
	const float *e1 = tw + 2 * (n / 16), *e2 = tw + 2 * (n / 8), *e3 = tw + 2 * (3 * n / 16);
	return e2[0] == -e2[1] && e2[0] > 0.0f && e3[0] == -e1[1] && e3[1] == -e1[0];
}

// w * b for w = tw[N/8] = (c, -c) of a symmetric table: cmul<> rounds c * b.x, c * b.y, (-c) * b.y, (-c) * b.x and then
// r = (c*b.x - (-c)*b.y, c*b.y + (-c)*b.x); (-c) * v == -(c * v) and a - (-b) == a + b in every bit (zeros included), so two
// products and r = (q.x + q.y, q.y - q.x) are the same four roundings
template <bool PK>
__device__ __forceinline__ float2 cmul_eighth(float c, float2 b)
{
	if constexpr (PK) {
		const zfft::v2f q = (zfft::v2f){c, c} * (zfft::v2f){b.x, b.y};
		zfft::v2f r; // (q.x + q.y, q.y - q.x): the second operand's lanes swapped, one negated (as butterfly<>'s -i form)
		asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,0] neg_hi:[0,1]" : "=v"(r) : "v"(q));
		return make_float2(r.x, r.y);
	}
	else {
		const float qx = c * b.x, qy = c * b.y;
		return make_float2(qx + qy, qy - qx);
	}
}

// in : p[m] = x[j + m * 256] * w[...] (the thread's eight windowed samples), w1 = tw[N/16], w2 = tw[N/8], w3 = tw[3N/16]
//      (w3 is only read where !SYM)
// out: Y[c] = Y_4[j][c], what butterfly<16, false, true, true, TW>(a, 0, 0, log2N, tw, 0, 0) leaves in a[c]
template <bool PK, bool SYM>
__device__ __forceinline__ void first_pass16(const float (&p)[8], float2 w1, float2 w2, float2 w3, float2 (&Y)[16])
{
	using zfft::cadd;
	using zfft::cmul;
	using zfft::csub;
	// ---- stage 2: group 0 = (s, 0), group 2 = (d, 0), group 1 = (x[m] + 0, 0 - x[m+4]), group 3 = its conjugate
	float s[4], d[4];
	float2 c1[4];
#pragma unroll
	for (int m = 0; m < 4; ++m) {
		s[m] = p[m] + p[m + 4];
		d[m] = p[m] - p[m + 4];
		c1[m] = make_float2(p[m], 0.0f - p[m + 4]);
	}
	// ---- stage 3: groups 0 and 4 real, 1 and 5 the one complex product with tw[N/8], 2 = (d[m] + 0, 0 - d[m+2])
	float S[2], D[2];
	float2 U[2], V[2], G[2];
#pragma unroll
	for (int m = 0; m < 2; ++m) {
		S[m] = s[m] + s[m + 2];
		D[m] = s[m] - s[m + 2];
		const float2 t = SYM ? cmul_eighth<PK>(w2.x, c1[m + 2]) : cmul<PK>(w2, c1[m + 2]);
		U[m] = cadd<PK>(c1[m], t);
		V[m] = csub<PK>(c1[m], t);
		G[m] = make_float2(d[m], 0.0f - d[m + 2]);
	}
	// ---- stage 4
	Y[0] = make_float2(S[0] + S[1], 0.0f);
	Y[8] = make_float2(S[0] - S[1], 0.0f);
	Y[4] = make_float2(D[0], 0.0f - D[1]); // w = -i
	Y[12] = make_float2(D[0], D[1]);
	{
		const float2 t = cmul<PK>(w1, U[1]);
		Y[1] = cadd<PK>(U[0], t);
		Y[9] = csub<PK>(U[0], t);
	}
	{
		const float2 t = SYM ? cmul_eighth<PK>(w2.x, G[1]) : cmul<PK>(w2, G[1]);
		Y[2] = cadd<PK>(G[0], t);
		Y[10] = csub<PK>(G[0], t);
	}
	{
		const float2 t = cmul<PK>(make_float2(w1.y, -w1.x), V[1]); // tw[N/16 + N/4]
		Y[5] = cadd<PK>(V[0], t);
		Y[13] = csub<PK>(V[0], t);
	}
	if constexpr (SYM) {
		// group c + 2 of stage 2, c + 4 .. of stage 3: operands conjugated, twiddles -conj(w) -> Y[16 - k] = conj(Y[k])
#pragma unroll
		for (int k = 1; k < 16; ++k)
			if (k == 1 || k == 2 || k == 5 || k == 9 || k == 10 || k == 13)
				Y[16 - k] = make_float2(Y[k].x, 0.0f - Y[k].y);
	}
	else {
		float2 c3[4], g3[2], g7[2], g6[2];
#pragma unroll
		for (int m = 0; m < 4; ++m)
			c3[m] = make_float2(p[m], 0.0f + p[m + 4]);
		const float2 w2i = make_float2(w2.y, -w2.x), w3i = make_float2(w3.y, -w3.x);
#pragma unroll
		for (int m = 0; m < 2; ++m) {
			const float2 t = cmul<PK>(w2i, c3[m + 2]);
			g3[m] = cadd<PK>(c3[m], t);
			g7[m] = csub<PK>(c3[m], t);
			g6[m] = make_float2(d[m], 0.0f + d[m + 2]);
		}
		{
			const float2 t = cmul<PK>(w3, g3[1]);
			Y[3] = cadd<PK>(g3[0], t);
			Y[11] = csub<PK>(g3[0], t);
		}
		{
			const float2 t = cmul<PK>(w2i, g6[1]);
			Y[6] = cadd<PK>(g6[0], t);
			Y[14] = csub<PK>(g6[0], t);
		}
		{
			const float2 t = cmul<PK>(w3i, g7[1]);
			Y[7] = cadd<PK>(g7[0], t);
			Y[15] = csub<PK>(g7[0], t);
		}
	}
}

} // namespace zen_blockrun
