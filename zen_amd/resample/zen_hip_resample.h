/*
 * zen_hip_resample.h -- band-limited sample-rate conversion of device rows by a rational ratio num / den, and with the time
 * stretch of zen_hip_tsm.h in front the pitch shift (libzen_hip_resample.so, linked against libzen_hip.so).
 *
 * The method is J. O. Smith's band-limited interpolation ("Digital Audio Resampling Home Page", CCRMA; Smith and Gossett, "A
 * flexible sampling-rate conversion method", ICASSP 1984): a windowed sinc tabulated at L phases per sample, two adjacent
 * table rows interpolated linearly to the output's position.  The window is Kaiser's (Kaiser, "Nonrecursive digital filter
 * design using the I0-sinh window function", ISCAS 1974).  DESIGN.md section 22 states it in full and says what was measured.
 *
 * The arithmetic (tests/resample_model.py computes the same bits).  Positions are unsigned 64-bit integers.  Every float
 * operation on the device is one float32 multiply, add or subtract, one rounding each, denormals kept; the table is computed
 * on the host in double (libm sin, sqrt) and rounded once -- zen_hip_resample_table hands it out.
 *
 *   Parameters: the ratio num / den, reduced by the gcd at create; after that 1 <= num, den <= 2^20 and 1/4 <= num / den <= 4;
 *   fs_out = fs_in num / den.  The quality Z, zero crossings per side: 8 (roll 0.85, beta 7.0), 16 (roll 0.91, beta 10.0) or
 *   32 (roll 0.9476, beta 14.77).  Rows are virtual rows of n_total samples, 1 <= n_total <= 2^40;
 *   n_out = ceil(n_total num / den), in integers.
 *
 *   Table: W = Z where num >= den, else ceil(Z den / num) in integers; T = 2 W taps (256 at the most);
 *   c = min(1, num / den) roll, num / den one double division; L = 512.  For p = 0..L and j = 0..T-1, with
 *   d = (double)(j - W + 1) - (double)p / L:  h[p][j] = float32((c s(c d)) w(d / W)),
 *   s(0) = 1, else s(v) = sin(pi v) / (pi v), pi v one product;  w(u) = I0(beta sqrt(max(0, 1 - u u))) / I0(beta);
 *   I0(x): hx = x / 2; term = 1; sum = 1; for k = 1..48: q = hx / k; term = term (q q); sum = sum + term.
 *   Row p is the T floats from h + p T on: rows p and p + 1 are adjacent.
 *
 *   Output t: a = t den; i = a div num; rem = a mod num; f = (rem 2^32) div num; p = f >> 23;
 *   mu = float32(f & 0x7FFFFF) 2^-23 (exact).  For j = 0..T-1: c_j = h[p][j] + mu (h[p + 1][j] - h[p][j]), three operations in
 *   that order; x_j = the sample at index i - W + 1 + j of the virtual row, 0 outside [0, n_total) and outside the window the
 *   call brought.  Eight chains s_k = (...((0 + x_k c_k) + x_{k+8} c_{k+8}) + ...) over j = k mod 8, the product and the sum
 *   each rounded; a chain without a tap is +0;  y[t] = ((s_0 + s_1) + (s_2 + s_3)) + ((s_4 + s_5) + (s_6 + s_7)).
 *   (A tap outside the row may be skipped: adding +-0 to a chain that starts at +0 never changes a bit.)
 *
 *   Windows: a call names its outputs (out_first, out_count), the window of the virtual row it brought (in_first, in_count,
 *   in_dev pointing at sample in_first) and n_total.  zen_hip_resample_span gives the window a range of outputs needs:
 *   [i_first - W + 1, i_last + W] clipped to the row.  A row cut into calls in any way gives the bits of the whole-row call.
 *
 *   Routes, same bits: the interpolating one forms c_j per output from the two table rows; the polyphase one (reduced
 *   num <= 4096) reads them from the num rows c[rem][j] a kernel expanded once at create with the same three operations.  The
 *   polyphase route is taken where it applies; ZEN_HIP_RESAMPLE="poly=0" in the environment at create selects the other.
 *
 * Conventions: those of zen_hip.h and zen_hip_tsm.h -- 0 (ZEN_HIP_OK) or a ZEN_HIP_E_* code, text from
 * zen_hip_resample_last_error() (this library's own thread-local message; failures of the library underneath are copied
 * into it).  All device memory comes from zen_hip_malloc; create allocates the table(s), and no device call allocates
 * afterwards (the host call takes the two rows it copies through for its own duration and gives them back).
 */
#ifndef ZEN_HIP_RESAMPLE_H
#define ZEN_HIP_RESAMPLE_H

#include <stddef.h>

#include "zen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zen_hip_resample* zen_hip_resample_t;

typedef struct zen_hip_resample_stats_t {
	unsigned long long calls;        /* run calls since create, host calls included */
	unsigned long long rows;         /* rows converted since create */
	unsigned long long outputs;      /* output samples written since create */
	unsigned long long poly_calls;   /* calls that took the polyphase route */
	unsigned long long interp_calls; /* calls that took the interpolating route */
	unsigned long long device_bytes; /* device memory the tables take */
	unsigned long long allocations;  /* zen_hip_malloc calls of create */
} zen_hip_resample_stats_t;

/* expand, fir */
enum { ZEN_HIP_RESAMPLE_KERNELS = 2 };
enum { ZEN_HIP_RESAMPLE_TILE = 256 };     /* consecutive outputs of one row a workgroup makes */
enum { ZEN_HIP_RESAMPLE_PHASES = 512 };   /* L: the table has L + 1 rows */
enum { ZEN_HIP_RESAMPLE_MAX_TAPS = 256 };
enum { ZEN_HIP_RESAMPLE_MAX_POLY = 4096 }; /* the largest reduced num of the polyphase route */
enum { ZEN_HIP_RESAMPLE_MAX_ROWS = 65535 };
enum { ZEN_HIP_RESAMPLE_ROUTE_INTERP = 0, ZEN_HIP_RESAMPLE_ROUTE_POLY = 1 };

const char* zen_hip_resample_last_error(void); /* thread-local text of the last failure of this library */
const char* zen_hip_resample_version(void);

/* num, den >= 1, after the reduction each at most 2^20 and 1/4 <= num / den <= 4; quality 8, 16 or 32 (ZEN_HIP_E_BAD_ARG
 * otherwise, before a device is touched).  create computes the table, allocates it ((L + 1) rows of T floats rounded up to a
 * multiple of 8) and, on the polyphase route, the num expanded rows, and runs the expansion. */
int zen_hip_resample_create(unsigned long long num, unsigned long long den, int quality, zen_hip_resample_t* h);
int zen_hip_resample_destroy(zen_hip_resample_t h);
int zen_hip_resample_set_stream(zen_hip_resample_t h, void* stream); /* waits for what the previous stream holds */

/* Outputs out_first .. out_first + out_count of each of n_rows virtual rows of n_total samples.  Row r brought the in_count
 * samples from index in_first on, at in_dev + r * in_stride; its outputs go to out_dev + r * out_stride.  The call writes
 * n_rows rows of out_count floats and nothing outside them, reads no float outside the windows, and is asynchronous on the
 * handle's stream.  ZEN_HIP_E_BAD_ARG, nothing touched: a null or misaligned (4 bytes) pointer; n_total outside 1..2^40;
 * out_count == 0 or outputs beyond n_out; a window outside the row or short of zen_hip_resample_span's; in_stride < in_count
 * or out_stride < out_count; n_rows outside 1..65535; more than 2^31 - 1 tiles; input and output rows that overlap. */
int zen_hip_resample_run_device(zen_hip_resample_t h, const float* in_dev, size_t in_stride, unsigned long long in_first, size_t in_count,
                                unsigned long long n_total, unsigned long long out_first, size_t out_count, float* out_dev, size_t out_stride,
                                size_t n_rows);
/* Whole rows in host memory: n_rows rows of n samples in, n_out samples each out, plain copies up and down around the device
 * call.  Synchronous. */
int zen_hip_resample_run_host(zen_hip_resample_t h, const float* in_host, size_t in_stride, size_t n, float* out_host, size_t out_stride,
                              size_t n_rows);

int zen_hip_resample_stats(zen_hip_resample_t h, zen_hip_resample_stats_t* out);

/* Profiling hooks for the harness (tools/ab_resample.py), as the tsm library's.  enable != 0: HIP events around every launch
 * from now on.  _get synchronises and returns, summed since the last _get, per step (expand, fir) milliseconds, bytes read +
 * written, and launches.  The expansion runs in create: its time is taken there and handed out by the first _get. */
int zen_hip_resample_profile(zen_hip_resample_t h, int enable);
int zen_hip_resample_profile_get(zen_hip_resample_t h, double ms[ZEN_HIP_RESAMPLE_KERNELS], unsigned long long bytes[ZEN_HIP_RESAMPLE_KERNELS],
                                 unsigned long long launches[ZEN_HIP_RESAMPLE_KERNELS]);

/* Host arithmetic, without a device and without a handle; a bad ratio, quality or null pointer is ZEN_HIP_E_BAD_ARG. */
/* n_out = ceil(n_total num / den); n_total in 1..2^40 */
int zen_hip_resample_n_out(unsigned long long num, unsigned long long den, unsigned long long n_total, unsigned long long* n_out);
/* the window [i_first - W + 1, i_last + W], clipped to the row, that outputs out_first .. out_first + out_count need;
 * out_count >= 1 and the outputs within n_out */
int zen_hip_resample_span(unsigned long long num, unsigned long long den, int quality, unsigned long long n_total, unsigned long long out_first,
                          unsigned long long out_count, unsigned long long* in_first, unsigned long long* in_count);
/* W, T and the route the ratio takes by the rule (ZEN_HIP_RESAMPLE_ROUTE_*; the environment is not looked at) */
int zen_hip_resample_geometry(unsigned long long num, unsigned long long den, int quality, size_t* W, size_t* T, int* route);
/* h: (L + 1) T floats; cap, the floats out has room for, must be at least that */
int zen_hip_resample_table(unsigned long long num, unsigned long long den, int quality, float* out, size_t cap);
/* the ratio of a pitch shift by `semitones` (finite, |semitones| <= 24): num = llround(65536 / 2^(semitones / 12)),
 * den = 65536, reduced.  The stretch in front has the ratio alpha = (double)den / (double)num. */
int zen_hip_resample_ratio_for_shift(double semitones, unsigned long long* num, unsigned long long* den);

#ifdef __cplusplus
}
#endif
#endif /* ZEN_HIP_RESAMPLE_H */
