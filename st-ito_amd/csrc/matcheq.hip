// matcheq.hip -- the rule-based style-transfer baseline of the reference (st_ito/style_transfer.py:163-278, run_rule_based)
// on gfx950: matched-EQ design and filtering, then the compressor hill-climb, for a batch of items.
//
// Replaces (reference file:line):
//   smooth_spectrum   style_transfer.py:163-165  scipy.signal.savgol_filter(H, 1025, 2), mode "interp"   -> k_savgol
//   firwin2           style_transfer.py:235-240  scipy.signal.firwin2(n_taps, freqs, sm_ref / sm_in)        -> k_firwin2
//   lfilter           style_transfer.py:243      scipy.signal.lfilter(b, [1.0], x), float64 sums           -> k_fir
//   peak normalise    style_transfer.py:220-223, 247-248, 266-267 (NaN-propagating max, like torch.max)   -> k_peak_nan, k_norm_gain
//   the hill-climb    style_transfer.py:254-268, every item of the batch in lockstep                      -> stito_climb_step
// (get_average_spectrum is k_stft_feature's mode 2 and the meter stito_lufs_raw, both in features.hip.)
//
// Precision follows the reference: the savgol sums, the firwin2 design and the FIR sums are float64 (scipy works in float64
// there), every result is rounded to float32 once where the reference does.  The hill-climb's stopping rule compares a loudness
// difference with 0.25 LU; keeping the filter within float32 rounding of scipy keeps that decision with the reference.
#include "common.h"
#include "dsp_view.h"
#include "juce_comp.h"

namespace stito {

// ---- Savitzky-Golay, mode "interp" ---------------------------------------------------------------------------------------
// Interior (h <= i < n - h, h = W / 2): sum_k c[k] x[i - h + k] with the correlation-order coefficients c (the host passes
// savgol_coeffs reversed); edges: the least-squares polynomial through the first / last W inputs evaluated at the edge
// points, as the linear operator E (W, W): out[i] = sum_j E[r][j] x[w0 + j], r = i - w0 (w0 = 0 left, n - W right).
__global__ __launch_bounds__(256) void k_savgol(const float *__restrict__ x, int n, const double *__restrict__ c, int W,
                                                const double *__restrict__ E, float *__restrict__ y) {
    const int i = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y, h = W / 2;
    if (i >= n) return;
    const float *xr = x + (int64_t)row * n;
    double acc = 0.0;
    if (i >= h && i < n - h) {
        const float *p = xr + i - h;
        for (int k = 0; k < W; ++k) acc = fma(c[k], (double)p[k], acc);
    } else {
        const int w0 = i < h ? 0 : n - W;
        const double *e = E + (int64_t)(i - w0) * W;
        const float *p = xr + w0;
        for (int j = 0; j < W; ++j) acc = fma(e[j], (double)p[j], acc);
    }
    y[(int64_t)row * n + i] = (float)acc;
}

// ---- firwin2 (scipy 1.15, float64) ---------------------------------------------------------------------------------------
// One workgroup per item:
//   gain[j]   = num[j] / den[j] in float32 with gain[n_freq - 1] = 0 (style_transfer.py:232-233), or num[j] when den is NULL;
//   fx[m]     = np.interp(grid[m], freq, gain), operation for operation;
//   Z[m]      = fx[m] * exp(i phase_b * grid[m] * inv_nyq)   (numpy's complex product and Smith division by nyq);
//   taps[t]   = irfft(Z)[t] * window[t], t < n_taps: the Hermitian spectrum of N = 2 (n_grid - 1) points, an in-place radix-2
//               inverse transform in LDS (N <= 8192 double2 = 128 KB), then 1/N.
__device__ __forceinline__ double fw_gain(const float *num, const float *den, int j, int n_freq) {
    if (!den) return (double)num[j];
    return j == n_freq - 1 ? 0.0 : (double)__fdiv_rn(num[j], den[j]);
}

__device__ __forceinline__ int fw_brev(int k, int bits) { return (int)(__brev((unsigned)k) >> (32 - bits)); }

__global__ __launch_bounds__(256) void k_firwin2(const float *__restrict__ num, const float *__restrict__ den, int n_freq,
                                                 const double *__restrict__ freq, const double *__restrict__ grid, int log2N,
                                                 double phase_b, double inv_nyq, const double *__restrict__ window, int n_taps,
                                                 double *__restrict__ taps) {
    extern __shared__ __attribute__((aligned(16))) double2 fw_lds[];
    double2 *Z = fw_lds;
    const int item = blockIdx.x, tid = threadIdx.x, N = 1 << log2N, half = N >> 1;
    const float *nm = num + (int64_t)item * n_freq;
    const float *dn = den ? den + (int64_t)item * n_freq : nullptr;
    for (int m = tid; m <= half; m += 256) {
        const double xv = grid[m];
        // numpy's binary search result: the last j with freq[j] <= xv
        int lo = 0, hi = n_freq - 1;
        if (xv >= freq[hi]) lo = hi;
        else
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (freq[mid] <= xv) lo = mid; else hi = mid;
            }
        const int j = lo;
        double fx;
        const double gj = fw_gain(nm, dn, j, n_freq);
        if (j == n_freq - 1 || freq[j] == xv) {
            fx = gj;
        } else {
            const double gj1 = fw_gain(nm, dn, j + 1, n_freq);
            const double slope = __ddiv_rn(__dsub_rn(gj1, gj), __dsub_rn(freq[j + 1], freq[j]));
            fx = __dadd_rn(__dmul_rn(slope, __dsub_rn(xv, freq[j])), gj);
            if (isnan(fx)) {
                fx = __dadd_rn(__dmul_rn(slope, __dsub_rn(xv, freq[j + 1])), gj1);
                if (isnan(fx) && gj == gj1) fx = gj;
            }
        }
        double s, c;
        sincos(__dmul_rn(__dmul_rn(phase_b, xv), inv_nyq), &s, &c);
        Z[m] = make_double2(__dmul_rn(fx, c), __dmul_rn(fx, s));
    }
    __syncthreads();
    for (int m = tid; m <= half; m += 256) {  // Hermitian completion; irfft ignores the imaginary parts at 0 and N/2
        const double2 v = Z[m];
        if (m == 0 || m == half) Z[m] = make_double2(v.x, 0.0);
        else Z[N - m] = make_double2(v.x, -v.y);
    }
    __syncthreads();
    // inverse DFT, radix-2 decimation in frequency, in place: element n ends at brev(n)
    for (int span = half, sh = 1; span >= 1; span >>= 1, ++sh) {
        for (int i = tid; i < half; i += 256) {
            const int j = i & (span - 1);
            const int a = ((i - j) << 1) + j;
            const double2 u = Z[a], v = Z[a + span];
            double ws, wc;
            sincospi((double)j / (double)span, &ws, &wc);  // exp(+2 pi i j / (2 span))
            const double dx = u.x - v.x, dy = u.y - v.y;
            Z[a] = make_double2(u.x + v.x, u.y + v.y);
            Z[a + span] = make_double2(dx * wc - dy * ws, dx * ws + dy * wc);
        }
        __syncthreads();
    }
    const double invN = 1.0 / (double)N;
    for (int t = tid; t < n_taps; t += 256) taps[(int64_t)item * n_taps + t] = Z[fw_brev(t, log2N)].x * invN * window[t];
}

// ---- causal FIR, float64 sums ---------------------------------------------------------------------------------------------
// y[o] = sum_{k < T} b[k] x[o - k], x before the start = 0 (zero initial state).  Workgroup = FIR_TILE consecutive outputs of
// one (item, channel) row: the item's taps (as doubles) and the input window [t0 - Tp, t0 + FIR_TILE) (as floats, one
// pad slot per 16 so that lanes FIR_R floats apart hit different banks) in LDS.  Thread = FIR_R consecutive outputs; the taps
// are walked in blocks of FIR_R: per block FIR_R new window values enter registers and FIR_R x FIR_R products accumulate, all
// register indices compile-time.  Tp = T rounded up to FIR_R; the last, partial block skips the padded taps, so every output
// is exactly the reference's sum (in another order), rounded to float32 once.
static constexpr int FIR_NT = 128, FIR_R = 16, FIR_TILE = FIR_NT * FIR_R;

__host__ __device__ __forceinline__ int fir_pad(int p) { return p + (p >> 4); }

template <bool TAIL>
__device__ __forceinline__ void fir_block(const double *__restrict__ tb, const float *__restrict__ xs, int q, int kb, int T,
                                          double (&win)[2 * FIR_R], double (&acc)[FIR_R]) {
    // win[FIR_R + j - kk] = x[o_j - (kb + kk)], i.e. win[i] = window value q - kb - FIR_R + i: the previous block's low half
    // moves up, the values entering this block fill the low half
#pragma unroll
    for (int i = 0; i < FIR_R; ++i) win[i + FIR_R] = win[i];
#pragma unroll
    for (int i = 0; i < FIR_R; ++i) win[i] = (double)xs[fir_pad(q - kb - FIR_R + i)];  // (win[0] is read as win[FIR_R] next block)
#pragma unroll
    for (int kk = 0; kk < FIR_R; ++kk) {
        if (TAIL && kb + kk >= T) break;
        const double b = tb[kb + kk];
#pragma unroll
        for (int j = 0; j < FIR_R; ++j) acc[j] = fma(b, win[FIR_R + j - kk], acc[j]);
    }
}

__global__ __launch_bounds__(FIR_NT) void k_fir(const float *__restrict__ x, int C, int64_t n, const double *__restrict__ taps,
                                                int T, int Tp, float *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) double fir_lds[];
    double *tb = fir_lds;                       // Tp doubles
    float *xs = (float *)(fir_lds + Tp);        // fir_pad(FIR_TILE + Tp) floats
    const int row = blockIdx.y, item = row / C, tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * FIR_TILE;
    const float *xr = x + (int64_t)row * n;
    const double *br = taps + (int64_t)item * T;
    for (int k = tid; k < Tp; k += FIR_NT) tb[k] = k < T ? br[k] : 0.0;
    const int nw = FIR_TILE + Tp;               // window value p <-> sample t0 - Tp + p
    for (int p = tid; p < nw; p += FIR_NT) {
        const int64_t t = t0 - Tp + p;
        xs[fir_pad(p)] = (t >= 0 && t < n) ? xr[t] : 0.0f;
    }
    __syncthreads();
    const int q = Tp + tid * FIR_R;             // window index of this thread's first output o_0 = t0 + tid * FIR_R
    double acc[FIR_R], win[2 * FIR_R];
#pragma unroll
    for (int j = 0; j < FIR_R; ++j) { acc[j] = 0.0; win[j] = 0.0; win[FIR_R + j] = 0.0; }
    // prime: win[FIR_R + j] = x[o_j] for the first block (kk = 0 reads win[FIR_R + j])
#pragma unroll
    for (int j = 0; j < FIR_R; ++j) win[j] = (double)xs[fir_pad(q + j)];
    // the first call's shift moves these up; its loads then fill x[o_0 - FIR_R .. o_0 - 1]
    int kb = 0;
    const int full = T / FIR_R * FIR_R;
    for (; kb < full; kb += FIR_R) fir_block<false>(tb, xs, q, kb, T, win, acc);
    if (kb < T) fir_block<true>(tb, xs, q, kb, T, win, acc);
    float *yr = y + (int64_t)row * n;
#pragma unroll
    for (int j = 0; j < FIR_R; ++j) {
        const int64_t o = t0 + tid * FIR_R + j;
        if (o < n) yr[o] = (float)acc[j];
    }
}

// ---- peak normalisation ---------------------------------------------------------------------------------------------------
// max |x| per item that propagates NaN like torch.max / np.max (k_peak in dsp.hip uses fmaxf, which drops it).  |NaN| has
// the sign bit clear, and as an unsigned int it orders above +inf, so the atomicMax on the uint view keeps it.
__device__ __forceinline__ float nan_max(float a, float b) { return (isnan(a) || a > b) ? a : b; }

__global__ __launch_bounds__(256) void k_peak_nan(const float *__restrict__ a, int64_t per_item, float *__restrict__ peaks) {
    __shared__ float red[4];
    const int item = blockIdx.y;
    const float *p = a + (int64_t)item * per_item;
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_item; i += (int64_t)gridDim.x * 256) m = nan_max(fabsf(p[i]), m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
        atomicMax((unsigned int *)&peaks[item], __float_as_uint(fabsf(m)));
    }
}

// x = (x / d) * gain, d = the peak, clamped to clamp_min when clamp_min > 0 (torch.clamp keeps a NaN peak NaN)
__global__ __launch_bounds__(256) void k_norm_gain(float *__restrict__ a, int64_t per_item, const float *__restrict__ peaks,
                                                   float clamp_min, float gain) {
    const int item = blockIdx.y;
    float d = peaks[item];
    if (clamp_min > 0.0f && !isnan(d)) d = fmaxf(d, clamp_min);
    float *p = a + (int64_t)item * per_item;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_item; i += (int64_t)gridDim.x * 256)
        p[i] = __fmul_rn(__fdiv_rn(p[i], d), gain);
}

static int mq_grid_x(int64_t per_item, int n_items) {
    int64_t want = (per_item + 255) / 256, cap = (256 * 16 + n_items - 1) / n_items;
    cap = cap < 1 ? 1 : cap;
    return (int)(want < cap ? want : cap);
}

static int peak_normalize(float *audio, int n_items, int64_t per_item, float clamp_min, float gain, float *peaks, hipStream_t st) {
    STITO_TRY(zero_async(peaks, sizeof(float) * n_items, st));
    const dim3 grid(mq_grid_x(per_item, n_items), n_items);
    hipLaunchKernelGGL(k_peak_nan, grid, dim3(256), 0, st, (const float *)audio, per_item, peaks);
    STITO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_norm_gain, grid, dim3(256), 0, st, audio, per_item, (const float *)peaks, clamp_min, gain);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

// ---- hill-climb -----------------------------------------------------------------------------------------------------------
// Per-item state on the device: threshold (dB), delta (LU), active flag, step count.  One step = compressor coefficients from
// each item's threshold -> compressor_stage(x_prev -> scratch) -> peak -> x / peak * 10^(-12/20) -> raw loudness -> commit
// scratch as x_prev and update the state, for active items only.
constexpr double CLIMB_RATIO = 3.0, CLIMB_ATTACK_MS = 1.0, CLIMB_RELEASE_MS = 100.0, CLIMB_STEP_DB = 0.5, CLIMB_FLOOR_DB = -80.0,
                 CLIMB_TOL_LU = 0.25;

__global__ void k_climb_init(const double *__restrict__ lufs_in, const double *__restrict__ lufs_tgt, int n_items,
                             double *__restrict__ thr, double *__restrict__ delta, int *__restrict__ active, int *__restrict__ steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const double d = lufs_tgt[i] - lufs_in[i];
    thr[i] = 0.0;
    delta[i] = d;
    steps[i] = 0;
    active[i] = (d > CLIMB_TOL_LU && 0.0 > CLIMB_FLOOR_DB) ? 1 : 0;
}

__global__ void k_climb_coef(const double *__restrict__ thr, int n_items, double sr, double *__restrict__ coef) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    juce_compressor_coef(thr[i], CLIMB_RATIO, CLIMB_ATTACK_MS, CLIMB_RELEASE_MS, sr, coef + (int64_t)i * COEF_STRIDE);
}

__global__ __launch_bounds__(256) void k_climb_commit(float *__restrict__ x, const float *__restrict__ scratch, int64_t per_item,
                                                      const int *__restrict__ active) {
    const int item = blockIdx.y;
    if (!active[item]) return;
    float *d = x + (int64_t)item * per_item;
    const float *s = scratch + (int64_t)item * per_item;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_item; i += (int64_t)gridDim.x * 256) d[i] = s[i];
}

__global__ void k_climb_update(const double *__restrict__ lufs, const double *__restrict__ lufs_tgt, int n_items,
                               double *__restrict__ thr, double *__restrict__ delta, int *__restrict__ active, int *__restrict__ steps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items || !active[i]) return;
    const double d = lufs_tgt[i] - lufs[i];
    const double t = thr[i] - CLIMB_STEP_DB;
    delta[i] = d;
    thr[i] = t;
    steps[i] += 1;
    active[i] = (d > CLIMB_TOL_LU && t > CLIMB_FLOOR_DB) ? 1 : 0;
}

struct ClimbLayout : WsLayout { size_t coef, comp, scratch, peaks, lufs, meter; };
static ClimbLayout climb_layout(int n_items, int C, int64_t n, int n_blocks) {
    ClimbLayout l;
    l.coef = l.add((size_t)n_items * COEF_STRIDE * sizeof(double));
    l.comp = l.add(compressor_workspace_bytes(n_items * C, n));
    l.scratch = l.add((size_t)n_items * C * n * sizeof(float));
    l.peaks = l.add((size_t)n_items * sizeof(float));
    l.lufs = l.add((size_t)n_items * sizeof(double));
    l.meter = l.add(stito_lufs_raw_workspace_bytes(n_items, C, n, n_blocks));
    return l;
}

}  // namespace stito

using namespace stito;

static int mq_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

extern "C" int stito_savgol(const float *in_dev, int n_rows, int n_cols, const double *coef_dev, int window, const double *edge_dev,
                            float *out_dev, void *stream) {
    STITO_REQUIRE(n_rows > 0, STITO_E_INVALID, "stito_savgol: empty input");
    STITO_REQUIRE(window >= 1 && (window & 1) == 1, STITO_E_INVALID, "stito_savgol: window %d must be odd", window);
    STITO_REQUIRE(window <= n_cols, STITO_E_INVALID, "stito_savgol: window %d longer than the rows (%d)", window, n_cols);
    STITO_REQUIRE(in_dev != out_dev, STITO_E_INVALID, "stito_savgol: not in place");
    hipLaunchKernelGGL(k_savgol, dim3((n_cols + 255) / 256, n_rows), dim3(256), 0, (hipStream_t)stream, in_dev, n_cols, coef_dev, window,
                       edge_dev, out_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

extern "C" int stito_firwin2(const float *num_dev, const float *den_dev, int n_items, int n_freq, const double *freq_dev,
                             const double *grid_dev, int n_grid, int n_taps, double phase_b, double inv_nyq, const double *window_dev,
                             double *taps_dev, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    STITO_REQUIRE(n_items > 0 && n_freq >= 2, STITO_E_INVALID, "stito_firwin2: empty input");
    STITO_REQUIRE(n_taps >= 16 && n_taps <= 4096, STITO_E_UNSUPPORTED, "stito_firwin2: n_taps %d not in [16, 4096]", n_taps);
    const int log2N = mq_log2(n_taps) + 1;
    STITO_REQUIRE(n_grid == (1 << (log2N - 1)) + 1, STITO_E_INVALID, "stito_firwin2: n_grid %d != 1 + 2**ceil(log2(n_taps))", n_grid);
    const size_t lds = ((size_t)1 << log2N) * sizeof(double2);
    STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_firwin2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_firwin2, dim3(n_items), dim3(256), lds, st, num_dev, den_dev, n_freq, freq_dev, grid_dev, log2N, phase_b, inv_nyq,
                       window_dev, n_taps, taps_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

extern "C" int stito_fir(const float *x_dev, int n_items, int channels, int64_t n_samples, const double *taps_dev, int n_taps,
                         float *y_dev, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    STITO_REQUIRE(n_items > 0 && channels > 0 && n_samples > 0, STITO_E_INVALID, "stito_fir: empty input");
    STITO_REQUIRE(n_taps >= 1 && n_taps <= 4096, STITO_E_UNSUPPORTED, "stito_fir: n_taps %d not in [1, 4096]", n_taps);
    STITO_REQUIRE(x_dev != y_dev, STITO_E_INVALID, "stito_fir: not in place");
    const int Tp = (n_taps + FIR_R - 1) / FIR_R * FIR_R;
    const size_t lds = (size_t)Tp * sizeof(double) + align_up((size_t)fir_pad(FIR_TILE + Tp) * sizeof(float), 16);
    STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_fir, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t gx = (n_samples + FIR_TILE - 1) / FIR_TILE;
    STITO_REQUIRE(gx < (1ll << 31), STITO_E_UNSUPPORTED, "stito_fir: %lld samples", (long long)n_samples);
    hipLaunchKernelGGL(k_fir, dim3((unsigned)gx, n_items * channels), dim3(FIR_NT), lds, st, x_dev, channels, n_samples, taps_dev, n_taps, Tp,
                       y_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

extern "C" int stito_peak_normalize(float *audio_dev, int n_items, int channels, int64_t n_samples, float clamp_min, float gain,
                                    float *peaks_dev, void *stream) {
    STITO_REQUIRE(n_items > 0 && channels > 0 && n_samples > 0, STITO_E_INVALID, "stito_peak_normalize: empty input");
    return peak_normalize(audio_dev, n_items, (int64_t)channels * n_samples, clamp_min, gain, peaks_dev, (hipStream_t)stream);
}

extern "C" int stito_climb_init(const double *input_lufs_dev, const double *target_lufs_dev, int n_items, double *threshold_dev,
                                double *delta_dev, int *active_dev, int *steps_dev, void *stream) {
    STITO_REQUIRE(n_items > 0, STITO_E_INVALID, "stito_climb_init: empty input");
    hipLaunchKernelGGL(k_climb_init, dim3((n_items + 63) / 64), dim3(64), 0, (hipStream_t)stream, input_lufs_dev, target_lufs_dev, n_items,
                       threshold_dev, delta_dev, active_dev, steps_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

extern "C" size_t stito_climb_workspace_bytes(int n_items, int channels, int64_t n_samples, int n_blocks) {
    if (n_items <= 0 || channels <= 0 || n_samples <= 0 || n_blocks <= 0) return 0;
    return climb_layout(n_items, channels, n_samples, n_blocks).total;
}

extern "C" int stito_climb_step(float *audio_dev, int n_items, int channels, int64_t n_samples, double sample_rate,
                                const double *kweight_coef_dev, const int *block_lo_dev, const int *block_hi_dev, int n_blocks,
                                double inv_block_len, const double *target_lufs_dev, double *threshold_dev, double *delta_dev,
                                int *active_dev, int *steps_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    STITO_REQUIRE(n_items > 0 && n_samples > 0 && n_blocks > 0, STITO_E_INVALID, "stito_climb_step: empty input");
    STITO_REQUIRE(channels == 1 || channels == 2, STITO_E_INVALID, "Invalid number of channels: %d", channels);
    const ClimbLayout l = climb_layout(n_items, channels, n_samples, n_blocks);
    STITO_REQUIRE(workspace_dev != nullptr && workspace_bytes >= l.total, STITO_E_WORKSPACE, "stito_climb_step: workspace too small");
    char *ws = (char *)workspace_dev;
    double *coef = (double *)(ws + l.coef), *lufs = (double *)(ws + l.lufs);
    float *scratch = (float *)(ws + l.scratch), *peaks = (float *)(ws + l.peaks);
    const int64_t per = (int64_t)channels * n_samples;
    hipLaunchKernelGGL(k_climb_coef, dim3((n_items + 63) / 64), dim3(64), 0, st, (const double *)threshold_dev, n_items, sample_rate, coef);
    STITO_LAUNCH_CHECK();
    InView in{audio_dev, per, n_samples, channels};
    STITO_TRY(compressor_stage(in, scratch, per, n_items, channels, n_samples, coef, ws + l.comp, st));
    // x_new /= max|x_new| (no clamp); x_new *= 10 ** (-12 / 20) in float32
    STITO_TRY(peak_normalize(scratch, n_items, per, 0.0f, (float)0.25118864315095796, peaks, st));
    STITO_TRY(stito_lufs_raw(scratch, n_items, channels, n_samples, kweight_coef_dev, block_lo_dev, block_hi_dev, n_blocks, inv_block_len,
                             lufs, ws + l.meter, l.total - l.meter, stream));
    hipLaunchKernelGGL(k_climb_commit, dim3(mq_grid_x(per, n_items), n_items), dim3(256), 0, st, audio_dev, (const float *)scratch, per,
                       (const int *)active_dev);
    STITO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_climb_update, dim3((n_items + 63) / 64), dim3(64), 0, st, (const double *)lufs, target_lufs_dev, n_items,
                       threshold_dev, delta_dev, active_dev, steps_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}
