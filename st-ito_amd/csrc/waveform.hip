// waveform.hip -- time-domain distances of a rendered population to target audio, as objectives of the ES: one pass over the rows.
//
// Replaces: the yardsticks auraloss.time ships beside the MR-STFT ones -- ESRLoss, DCLoss, SNRLoss, SISDRLoss, LogCoshLoss --
// restated (auraloss is not installed: parity is unpinned, like the MR-STFT distances').  A row is one channel of one item, x the
// candidate's row after the folded peak normalisation x * (1 / clip(peak, 1e-8)), y the target's.  With a prefilter of n_taps odd
// taps, c = n_taps / 2, both rows first become p[i] = sum_k taps[k] row[i + k - c], row zero outside [0, n) -- conv1d with zero
// padding, the convention of mrstft.hip's prefiltered kernels; without one, p = row.  d = p_x - p_y, eps = 1e-8, per row
//     esr     = sum d^2 / (sum p_y^2 + eps)
//     dc      = (sum d / n)^2 / (sum p_y^2 / n + eps)
//     snr     = -10 log10(sum p_y^2 / (sum d^2 + eps) + eps)
//     sisdr   = -10 log10(sum t^2 / (sum res^2 + eps) + eps),  x' = p_x - mean p_x,  y' = p_y - mean p_y,
//               t = alpha y',  alpha = sum x' y' / (sum y'^2 + eps),  res = x' - t
//     logcosh = (1 / n) sum ln(cosh d + eps)
// and an item's value is the mean over its rows.  ONE deviation from the formula as written: a sample with d == 0 adds exactly 0 to
// the log-cosh sum, not ln(1 + eps) = 1e-8.  That is what makes logcosh(y, table(y)) exactly 0 and lets zero padding add nothing to
// the sums; it moves the value by at most 1e-8 times the share of such samples.
//
// One workgroup = one tile of WF_TILE samples of one row.  Thread t owns the runs of four consecutive samples 4 (t + 256 g) ...,
// g < WF_GROUPS, in both forms of the kernel, and walks them in that order, so the order of every sum is a property of the tile and
// of nothing else.  Without a prefilter the runs come straight from global memory (16-byte loads where the row is aligned and the
// run whole, else sample by sample: the same values either way).  With one, the workgroup stages the raw run it needs in LDS -- the
// tile and c samples on either side, zero outside the row, scaled -- and every thread filters its runs from a sliding register
// window (ad_fir_run of audio_distance.h, shared with mrstft.hip like the slot rule, the folded peak, the tile tree and the host
// checks of a loss call): the chain of each output is fmaf in tap order from 0.0f, the taps come through scalar loads.  The file is
// built without fp contraction and the target's table is written by the same function (template TARGET), so the filtered target
// and a filtered candidate of the same audio have the same bits: esr, dc and logcosh of y against table(y) are exactly 0.
//
// Sums: per lane in float64 (the products of two float32 are exact there), per tile a fixed tree in LDS, per-tile partials to the
// workspace, and a second launch that adds a row's tiles in order, forms the requested kind from the moments in float64 and takes
// the mean over the rows.  No atomics: a candidate's bits depend on its own audio, its peak, its target and the taps only.  The
// log-cosh term is evaluated in float64 (coshf rounds 1 + d^2 / 2 away for small d), and only when that kind is asked for.
#include "audio_distance.h"

namespace stito {

static constexpr int WF_THREADS = 256;
static constexpr int WF_GROUPS = 8;                          // runs of four samples per thread
static constexpr int WF_TILE = 4 * WF_GROUPS * WF_THREADS;   // 8192 samples
static constexpr int WF_MAX_CH = 8;
static constexpr int WF_MOMENTS = 6;                         // sum d^2, d, p_x, p_x^2, p_x p_y, log-cosh term
static constexpr int WF_KINDS = 5;                           // esr, dc, snr, sisdr, logcosh

static bool wf_taps_ok(int n_taps) { return n_taps == 0 || (n_taps >= 1 && n_taps <= AD_MAX_TAPS && (n_taps & 1) == 1); }
static bool wf_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 40); }
static int64_t wf_tiles(int64_t n) { return (n + WF_TILE - 1) / WF_TILE; }
static int64_t wf_row_floats(int64_t n) { return (n + 3) & ~(int64_t)3; }   // rows of the table start on 16 bytes

// Table (floats): rows x wf_row_floats filtered samples (behind n: zeros), then doubles -- rows x {sum p_y, sum p_y^2}, then
// rows x tiles x 2 per-tile partials of those (scratch of stito_waveform_target).
static int64_t wf_table_floats(int64_t rows, int64_t n) { return rows * wf_row_floats(n) + 4 * rows + 4 * rows * wf_tiles(n); }

// ln(cosh d + eps) in float64 as log1p(2 sinh^2(d / 2) + eps), which does not round cosh d - 1 away against the 1; 0 for d == 0
// (see the head of the file)
__device__ __forceinline__ double wf_logcosh(double d) {
    const double s = sinh(0.5 * d);
    return d == 0.0 ? 0.0 : log1p(fma(2.0 * s, s, 1e-8));
}

// TARGET: audio = y (rows, n); writes the filtered rows to the table and the tile's sum p_y, sum p_y^2 (2 partials).
// else:   audio = candidates (pop, C, n); row = cand * C + ch against table row ad_target_of(cand) * C + ch; the tile's WF_MOMENTS
//         partials.  A candidate whose slot names no target reads nothing and writes nothing: k_waveform_final gives it NaN.
// PRE:    the rows go through the taps.  LC: the log-cosh term is evaluated (else its partial is 0 and nobody reads it).
template <bool TARGET, bool PRE, bool LC>
__global__ __launch_bounds__(WF_THREADS) void k_waveform(const float *__restrict__ audio, const float *__restrict__ peaks, int norm_passes,
                                                        const float *__restrict__ taps, int n_taps, float *__restrict__ table,
                                                        int64_t row_floats, int64_t n, int tiles, int C, int per_target,
                                                        const int32_t *__restrict__ slots, int n_targets, double *__restrict__ partial) {
    constexpr int K = TARGET ? 2 : WF_MOMENTS;
    __shared__ __attribute__((aligned(16))) float raw[PRE ? WF_TILE + AD_TAP_REACH : 4];
    __shared__ double red[K][WF_THREADS];

    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - row * tiles);
    const int64_t t0 = (int64_t)tile * WF_TILE;
    const int len = (int)(n - t0 < WF_TILE ? n - t0 : WF_TILE);   // >= 1: tiles = ceil(n / WF_TILE)

    float r1 = 1.0f;
    int64_t trow = row;
    if (!TARGET) {
        const int64_t cand = row / C;
        const int t = ad_target_of(cand, per_target, slots, n_targets);
        if (t < 0) return;  // the whole workgroup (one row, one candidate), before it loads anything
        r1 = ad_peak_scale(peaks, norm_passes, cand);
        trow = (int64_t)t * C + (row - cand * C);
    }
    const float *x = audio + row * n;
    float *py_row = table + trow * row_floats + t0;   // 16-byte aligned: the table is, row_floats and t0 are multiples of 4

    if constexpr (PRE) {
        const int c = n_taps >> 1;
        const int raw_len = ((len + 3) & ~3) + 4 * ((n_taps + 3) >> 2);   // <= WF_TILE + AD_TAP_REACH
        for (int i = tid; i < raw_len; i += WF_THREADS) {
            const int64_t s = t0 - c + i;
            raw[i] = (s >= 0 && s < n) ? x[s] * r1 : 0.0f;
        }
        __syncthreads();
    }
    const bool x_aligned = (((uintptr_t)(x + t0)) & 15) == 0;

    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll
    for (int gi = 0; gi < WF_GROUPS; ++gi) {
        const int g = tid + gi * WF_THREADS;
        const int valid = len - 4 * g < 4 ? len - 4 * g : 4;   // samples of this run inside the row
        if (valid <= 0) continue;
        float px[4];
        if constexpr (PRE) {
            // outputs 4 g .. 4 g + 3 of the tile: raw[j] = row[t0 - c + j], so p[t0 + o] = sum_k taps[k] raw[o + k]
            const float4 v = ad_fir_run(raw, g, taps, n_taps);
            px[0] = v.x; px[1] = v.y; px[2] = v.z; px[3] = v.w;
        } else if (x_aligned && valid == 4) {
            const float4 v = *(const float4 *)(x + t0 + 4 * g);
            px[0] = v.x * r1; px[1] = v.y * r1; px[2] = v.z * r1; px[3] = v.w * r1;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) px[j] = j < valid ? x[t0 + 4 * g + j] * r1 : 0.0f;
        }
        if constexpr (TARGET) {
            // the run behind the row's end is zero in the table: its rows are wf_row_floats long, so the store stays inside
            *(float4 *)(py_row + 4 * g) = make_float4(px[0], valid > 1 ? px[1] : 0.0f, valid > 2 ? px[2] : 0.0f, valid > 3 ? px[3] : 0.0f);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < valid) {
                    const double v = (double)px[j];
                    acc[0] += v;
                    acc[1] = fma(v, v, acc[1]);
                }
            }
        } else {
            const float4 yv = *(const float4 *)(py_row + 4 * g);
            const float py[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < valid) {
                    const double vx = (double)px[j], vy = (double)py[j];
                    const double d = vx - vy;
                    acc[0] = fma(d, d, acc[0]);
                    acc[1] += d;
                    acc[2] += vx;
                    acc[3] = fma(vx, vx, acc[3]);
                    acc[4] = fma(vx, vy, acc[4]);
                    if constexpr (LC) acc[5] += wf_logcosh(d);
                }
            }
        }
    }

    ad_tile_tree<K, WF_THREADS>(red, acc, tid);
    if (tid < K) partial[(row * tiles + tile) * K + tid] = red[tid][0];
}

// sum p_y and sum p_y^2 per target row: the tiles in order
__global__ void k_waveform_target_sum(const double *__restrict__ partial, int64_t rows, int tiles, double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * rows) return;
    const int64_t row = i >> 1;
    const int k = (int)(i & 1);
    const double *p = partial + row * tiles * 2 + k;
    double acc = 0.0;
    for (int t = 0; t < tiles; ++t) acc += p[2 * t];
    sums[i] = acc;
}

// The requested kind of one row from its moments, float64.
__device__ __forceinline__ double wf_value(int kind, const double *m, double sy, double sy2, double n) {
    const double eps = 1e-8;
    const double sd2 = m[0], sd = m[1], sx = m[2], sx2 = m[3], sxy = m[4], slc = m[5];
    switch (kind) {
    case 0: return sd2 / (sy2 + eps);
    case 1: { const double md = sd / n; return md * md / (sy2 / n + eps); }
    case 2: return -10.0 * log10(sy2 / (sd2 + eps) + eps);
    case 3: {
        const double cxy = sxy - sx * sy / n, cyy = sy2 - sy * sy / n, cxx = sx2 - sx * sx / n;   // sums over the centred rows
        const double alpha = cxy / (cyy + eps);
        const double st2 = alpha * alpha * cyy;
        const double sres2 = cxx - 2.0 * alpha * cxy + st2;
        return -10.0 * log10(st2 / (fmax(sres2, 0.0) + eps) + eps);   // fmax: the rounding of a vanishing residual; NaN passes
    }
    default: return slc / n;
    }
}

// one wave per candidate: lane ch adds its row's tiles in order and forms the kind, lane 0 the mean over the rows in order
__global__ __launch_bounds__(64) void k_waveform_final(int kind, const double *__restrict__ partial, const double *__restrict__ ysum,
                                                       int64_t n, int tiles, int C, int per_target, const int32_t *__restrict__ slots,
                                                       int n_targets, float *__restrict__ loss) {
    __shared__ double term[WF_MAX_CH];
    const int cand = blockIdx.x, lane = threadIdx.x;
    const int tgt = ad_target_of(cand, per_target, slots, n_targets);
    if (tgt < 0) {  // the whole wave: no partial was written for this candidate and none is read
        if (lane == 0) loss[cand] = __builtin_nanf("");
        return;
    }
    if (lane < C) {
        const int64_t row = (int64_t)cand * C + lane, trow = (int64_t)tgt * C + lane;
        const double *p = partial + row * tiles * WF_MOMENTS;
        double m[WF_MOMENTS];
#pragma unroll
        for (int k = 0; k < WF_MOMENTS; ++k) m[k] = 0.0;
        for (int t = 0; t < tiles; ++t) {
#pragma unroll
            for (int k = 0; k < WF_MOMENTS; ++k) m[k] += p[(int64_t)t * WF_MOMENTS + k];
        }
        term[lane] = wf_value(kind, m, ysum[2 * trow], ysum[2 * trow + 1], (double)n);
    }
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;
        for (int ch = 0; ch < C; ++ch) acc += term[ch];
        loss[cand] = (float)(acc / C);
    }
}

template <bool TARGET, bool LC>
static void wf_launch(bool pre, unsigned grid, hipStream_t st, const float *audio, const float *peaks, int norm_passes, const float *taps,
                      int n_taps, float *table, int64_t n, int tiles, int C, int per_target, const int32_t *slots, int n_targets,
                      double *partial) {
    if (pre)
        hipLaunchKernelGGL((k_waveform<TARGET, true, LC>), dim3(grid), dim3(WF_THREADS), 0, st, audio, peaks, norm_passes, taps, n_taps, table,
                           wf_row_floats(n), n, tiles, C, per_target, slots, n_targets, partial);
    else
        hipLaunchKernelGGL((k_waveform<TARGET, false, LC>), dim3(grid), dim3(WF_THREADS), 0, st, audio, peaks, norm_passes, taps, n_taps, table,
                           wf_row_floats(n), n, tiles, C, per_target, slots, n_targets, partial);
}

// The one launch path of the loss: populations of pop / n_slots candidates, population k against target target_slot[k] of the
// table's n_targets, or against target k when there is no slot list (then n_slots == n_targets).
static int wf_loss(const char *who, int kind, const float *taps_dev, int n_taps, const float *audio_dev, const float *peaks_dev,
                   int norm_passes, const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots, int pop, int channels,
                   int64_t n, float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    STITO_REQUIRE(kind >= 0 && kind < WF_KINDS, STITO_E_INVALID, "%s: kind %d is none of 0 (esr), 1 (dc), 2 (snr), 3 (sisdr), 4 (logcosh)", who,
                  kind);
    STITO_TRY(ad_taps_check(who, taps_dev, n_taps, true));
    STITO_REQUIRE(wf_n_ok(n), STITO_E_INVALID, "%s: %lld samples", who, (long long)n);
    STITO_TRY(ad_loss_args_check(who, pop, n_targets, n_slots, [&] {
        STITO_REQUIRE(channels >= 1 && channels <= WF_MAX_CH, STITO_E_INVALID, "Invalid number of channels: %d", channels);
        return STITO_OK;
    }, norm_passes, peaks_dev, audio_dev, table_dev, loss_dev));
    STITO_REQUIRE(((uintptr_t)audio_dev & 3) == 0, STITO_E_INVALID, "%s: the audio must be 4-byte aligned", who);
    const int64_t rows = (int64_t)pop * channels, trows = (int64_t)n_targets * channels, tiles = wf_tiles(n);
    STITO_REQUIRE(rows * tiles < ((int64_t)1 << 31), STITO_E_UNSUPPORTED, "%s: too many tiles", who);
    const size_t need = (size_t)rows * tiles * WF_MOMENTS * sizeof(double);
    STITO_TRY(ad_workspace_check(who, workspace_dev, workspace_bytes, need));
    double *partial = (double *)workspace_dev;
    const double *ysum = (const double *)(table_dev + trows * wf_row_floats(n));
    const unsigned grid = (unsigned)(rows * tiles);
    if (kind == 4)
        wf_launch<false, true>(n_taps > 0, grid, st, audio_dev, peaks_dev, norm_passes, taps_dev, n_taps, (float *)table_dev, n, (int)tiles,
                               channels, pop / n_slots, target_slot_dev, n_targets, partial);
    else
        wf_launch<false, false>(n_taps > 0, grid, st, audio_dev, peaks_dev, norm_passes, taps_dev, n_taps, (float *)table_dev, n, (int)tiles,
                                channels, pop / n_slots, target_slot_dev, n_targets, partial);
    STITO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_waveform_final, dim3((unsigned)pop), dim3(64), 0, st, kind, partial, ysum, n, (int)tiles, channels, pop / n_slots,
                       target_slot_dev, n_targets, loss_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

}  // namespace stito

using namespace stito;

extern "C" int stito_waveform_tile_samples(int n_taps) { return wf_taps_ok(n_taps) ? WF_TILE : 0; }

extern "C" int64_t stito_waveform_table_floats(int n_taps, int rows, int64_t n_samples) {
    if (!wf_taps_ok(n_taps) || rows < 1 || !wf_n_ok(n_samples) || (int64_t)rows * wf_tiles(n_samples) >= ((int64_t)1 << 31)) return 0;
    return wf_table_floats(rows, n_samples);
}

extern "C" size_t stito_waveform_workspace_bytes(int n_taps, int pop, int channels, int64_t n_samples) {
    if (!wf_taps_ok(n_taps) || pop < 1 || channels < 1 || channels > WF_MAX_CH || !wf_n_ok(n_samples)) return 0;
    if ((int64_t)pop * channels * wf_tiles(n_samples) >= ((int64_t)1 << 31)) return 0;
    return (size_t)pop * channels * wf_tiles(n_samples) * WF_MOMENTS * sizeof(double);
}

extern "C" int stito_waveform_target(const float *taps_dev, int n_taps, const float *y_dev, int rows, int64_t n_samples, float *table_dev,
                                     void *stream) {
    const char *who = "stito_waveform_target";
    hipStream_t st = (hipStream_t)stream;
    STITO_TRY(ad_taps_check(who, taps_dev, n_taps, true));
    STITO_REQUIRE(wf_n_ok(n_samples), STITO_E_INVALID, "%s: %lld samples", who, (long long)n_samples);
    STITO_REQUIRE(rows >= 1, STITO_E_INVALID, "%s: %d rows", who, rows);
    STITO_REQUIRE(y_dev != nullptr && table_dev != nullptr, STITO_E_INVALID, "%s: null pointer", who);
    STITO_REQUIRE(((uintptr_t)table_dev & 15) == 0, STITO_E_INVALID, "%s: the table must be 16-byte aligned", who);
    STITO_REQUIRE(((uintptr_t)y_dev & 3) == 0, STITO_E_INVALID, "%s: the audio must be 4-byte aligned", who);
    const int64_t tiles = wf_tiles(n_samples);
    STITO_REQUIRE((int64_t)rows * tiles < ((int64_t)1 << 31), STITO_E_UNSUPPORTED, "%s: too many tiles", who);
    double *sums = (double *)(table_dev + (int64_t)rows * wf_row_floats(n_samples));
    double *partial = sums + 2 * (int64_t)rows;
    wf_launch<true, false>(n_taps > 0, (unsigned)(rows * tiles), st, y_dev, nullptr, 0, taps_dev, n_taps, table_dev, n_samples, (int)tiles, 1, 1,
                           nullptr, rows, partial);
    STITO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_waveform_target_sum, dim3((unsigned)((2 * (int64_t)rows + 63) / 64)), dim3(64), 0, st, partial, (int64_t)rows, (int)tiles,
                       sums);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

extern "C" int stito_waveform_loss(int kind, const float *taps_dev, int n_taps, const float *audio_dev, const float *peaks_dev, int norm_passes,
                                   const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples, float *loss_dev,
                                   void *workspace_dev, size_t workspace_bytes, void *stream) {
    return wf_loss("stito_waveform_loss", kind, taps_dev, n_taps, audio_dev, peaks_dev, norm_passes, table_dev, n_targets, nullptr, n_targets,
                   pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int stito_waveform_loss_slots(int kind, const float *taps_dev, int n_taps, const float *audio_dev, const float *peaks_dev,
                                         int norm_passes, const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots,
                                         int pop, int channels, int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes,
                                         void *stream) {
    STITO_REQUIRE(target_slot_dev != nullptr, STITO_E_INVALID, "stito_waveform_loss_slots: null target_slot_dev");
    return wf_loss("stito_waveform_loss_slots", kind, taps_dev, n_taps, audio_dev, peaks_dev, norm_passes, table_dev, n_targets,
                   target_slot_dev, n_slots, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}
