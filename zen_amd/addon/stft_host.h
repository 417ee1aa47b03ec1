// stft_host.h -- what the host sources of the spectrogram add-ons share (zen_amd/repet, repsim, nmf) beyond addon_host.h:
// the frame sizes they take, the Hamming window and the divisor of the overlap-add as the contracts state them, and the
// first steps of every call (frame, transform, magnitude).  Header-only with internal linkage, as addon_host.h is.
#pragma once

#include <cmath>
#include <cstdint>

#include "addon_host.h"
#include "stft_args.h"

namespace zen_addon {
namespace {

inline bool frame_ok(size_t nfft) { return is_pow2(nfft) && nfft >= 64 && nfft <= 8192; }
inline size_t frames_of(size_t n, size_t H) { return (n + H - 1) / H + 1; }
inline float window_at(size_t i, size_t N) { return (float)(0.54 - 0.46 * cos(2.0 * M_PI * (double)i / (double)N)); }
inline float divisor_at(size_t i, size_t N) { return (float)((double)N * ((double)window_at(i, N) + (double)window_at(i + N / 2, N))); }
inline bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// a handle's `tables`: the window (N floats), the divisor (N / 2) behind it
inline std::vector<float> stft_tables(size_t N)
{
	std::vector<float> tab(N + N / 2);
	for (size_t i = 0; i < N; ++i)
		tab[i] = window_at(i, N);
	for (size_t i = 0; i < N / 2; ++i)
		tab[N + i] = divisor_at(i, N);
	return tab;
}

typedef hipError_t (*FrameLauncher)(const FrameArgs&, hipStream_t); // a library's own, from its kernel source
typedef hipError_t (*MagLauncher)(const MagArgs&, hipStream_t);

// The spectra X (a.rows) and the magnitudes V of every clip of a call, on `stream`: the library's frame kernel on `a`, the
// N-point transform `fft` over all the frames, the library's magnitude kernel into v; k_frame, k_fft and k_mag are their
// slots in the library's profile.
template <int K>
int spectra(Profiler<K>& prof, hipStream_t stream, zen_hip_fft_t fft, int k_frame, int k_fft, int k_mag, FrameLauncher launch_frame,
            MagLauncher launch_magnitude, const FrameArgs& a, float* v, size_t v_stride)
{
	const size_t N = (size_t)a.N, bins = N / 2 + 1, frames = a.n_clips * a.m;
	{
		auto kt = prof.on_stream(stream);
		ZA_TRY(kt.begin(k_frame, sizeof(float) * (a.n_clips * a.n + frames * 2 * N)));
		ZA_HIP(launch_frame(a, stream));
		ZA_TRY(kt.end());
	}
	{
		auto kt = prof.on_stream(stream);
		ZA_TRY(kt.begin(k_fft, sizeof(float) * frames * 4 * N));
		ZA_ZEN(zen_hip_fft_exec_batched(fft, a.rows, frames, 0, stream));
		ZA_TRY(kt.end());
	}
	{
		const MagArgs mag = {a.rows, v, v_stride, frames, a.N};
		auto kt = prof.on_stream(stream);
		ZA_TRY(kt.begin(k_mag, sizeof(float) * frames * (2 * bins + v_stride)));
		ZA_HIP(launch_magnitude(mag, stream));
		ZA_TRY(kt.end());
	}
	return ZEN_HIP_OK;
}

} // namespace
} // namespace zen_addon
