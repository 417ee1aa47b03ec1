// hpri_pair.h -- the two anticausal engines of the two-pass separation, as ragged.hip and live.hip hold them: created as
// zen_hip_hpri_create creates its pair (csrc/hpri.hip:85-90), with the calls that go to both.  Internal linkage throughout
// (see addon_host.h).
#pragma once

#include <cmath>

#include "addon_host.h"

namespace zen_addon {
namespace {

// hps.cu:109-126 hpss_chunk_padder: float ceil of a float quotient, plus `lag` chunks
size_t chunk_padder(size_t audio_size, size_t hop, size_t lag)
{
	const int n = (int)(ceilf((float)audio_size / (float)hop)) + (int)lag;
	return n > 0 ? (size_t)n * hop : 0;
}

struct HpriPair {
	zen_hip_hpr_t e1 = nullptr; // hop_h; H, P, R; anticausal (csrc/hpri.hip:85-87)
	zen_hip_hpr_t e2 = nullptr; // hop_p; P only; anticausal (csrc/hpri.hip:89-90)
	size_t lag_h = 0, lag_p = 0;
};

// On failure the engines made so far stay in *h: pair_destroy takes them.
int pair_create(HpriPair* h, float fs, size_t hop_h, size_t hop_p, float beta_h, float beta_p, int nocopybord, size_t n_streams)
{
	ZA_ZEN(zen_hip_hpr_create(fs, hop_h, beta_h, ZEN_HIP_OUTPUT_HARMONIC | ZEN_HIP_OUTPUT_PERCUSSIVE | ZEN_HIP_OUTPUT_RESIDUAL,
	                          ZEN_HIP_TIME_ANTICAUSAL, !nocopybord, n_streams, 0, &h->e1));
	ZA_ZEN(zen_hip_hpr_create(fs, hop_p, beta_p, ZEN_HIP_OUTPUT_PERCUSSIVE, ZEN_HIP_TIME_ANTICAUSAL, !nocopybord, n_streams, 0, &h->e2));
	zen_hip_hpr_params p1, p2;
	ZA_ZEN(zen_hip_hpr_get_params(h->e1, &p1));
	ZA_ZEN(zen_hip_hpr_get_params(h->e2, &p2));
	h->lag_h = (size_t)p1.lag;
	h->lag_p = (size_t)p2.lag;
	return ZEN_HIP_OK;
}

void pair_destroy(HpriPair* h)
{
	zen_hip_hpr_destroy(h->e1);
	zen_hip_hpr_destroy(h->e2);
}

int pair_set_stream(HpriPair* h, void* stream)
{
	ZA_ZEN(zen_hip_hpr_set_stream(h->e1, stream)); // (each waits for what the previous stream holds)
	ZA_ZEN(zen_hip_hpr_set_stream(h->e2, stream));
	return ZEN_HIP_OK;
}

int pair_use_sse_filter(HpriPair* h)
{
	ZA_ZEN(zen_hip_hpr_use_sse_filter(h->e1));
	ZA_ZEN(zen_hip_hpr_use_sse_filter(h->e2));
	return ZEN_HIP_OK;
}

int pair_use_soft_mask(HpriPair* h)
{
	ZA_ZEN(zen_hip_hpr_use_soft_mask(h->e1));
	ZA_ZEN(zen_hip_hpr_use_soft_mask(h->e2));
	return ZEN_HIP_OK;
}

int pair_reset_buffers(HpriPair* h)
{
	ZA_ZEN(zen_hip_hpr_reset_buffers(h->e1));
	ZA_ZEN(zen_hip_hpr_reset_buffers(h->e2));
	return ZEN_HIP_OK;
}

int pair_profile(HpriPair* h, int enable)
{
	ZA_ZEN(zen_hip_hpr_profile(h->e1, enable));
	ZA_ZEN(zen_hip_hpr_profile(h->e2, enable));
	return ZEN_HIP_OK;
}

int pair_profile_get_engine(HpriPair* h, int pass, double ms[6], unsigned long long launches[6]) // pass: 1 or 2
{
	ZA_ZEN(zen_hip_hpr_profile_get_all(pass == 1 ? h->e1 : h->e2, ms, launches));
	return ZEN_HIP_OK;
}

} // namespace
} // namespace zen_addon
