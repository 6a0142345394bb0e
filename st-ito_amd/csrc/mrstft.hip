// mrstft.hip -- multi-resolution STFT distance of a rendered population against target audio, fused.
//
// Replaces (reference file:line): auraloss.freq.MultiResolutionSTFTLoss()(x, y) with the library's defaults, the
// reference's second yardstick -- scripts/eval/eval_synthetic.py:72, 368-369, st_ito/methods/style.py:611 -- as an
// objective of the ES: per resolution (n_fft, hop, win) and (candidate, channel) row
//     sc = || |Y| - |X| ||_F / || |Y| ||_F,   lm = mean | ln|X| - ln|Y| |,   |.| = sqrt(max(re^2 + im^2, 1e-8)),
// torch.stft's framing (centred, reflect padding of n_fft / 2, periodic Hann of `win` points in the middle of the frame,
// one-sided); an item's loss is the mean over resolutions of the mean over its channels of sc + lm.
//
// One workgroup = one tile of F consecutive frames of one (row, resolution).  The tile's sample span (F - 1) hop + n_fft is
// loaded ONCE into LDS (reflected, with x / clip(peak, 1e-8) folded in like stito_logmel's loader): hop is 8.5 - 10 x smaller
// than n_fft, so from HBM / L2 every sample is read about once instead of ten times.  Every wave then owns a frame at a
// time: window, pack the n_fft real samples as n_fft / 2 complex points, an in-place decimation-in-frequency FFT in the
// wave's own LDS buffer (radix 4, one radix-2 stage last when log2 is odd; the spectrum is left in digit-reversed order
// and the unpacking reads it there), magnitudes in registers.  Nothing is shared between waves during the frames, and LDS
// operations of one wave execute in order, so there is no workgroup barrier inside the frame loop.
//
// The target's magnitudes come from a table that the same kernel (template TARGET) writes: the FFT and magnitude code is
// one function compiled without fp contraction (Makefile), so loss(y, table(y)) is exactly 0.  Sums: per lane in float64,
// per tile a fixed-order tree in LDS, per-tile partials to the workspace, one small launch adds the tiles in order -- no
// atomics, and a candidate's loss depends on nothing but its own audio, its target and the resolutions.
//
// The sum / difference variant (template SD; auraloss.freq.SumAndDifferenceSTFTLoss with both weights 1, restated) is the same
// distance of the 2-channel signal [L + R, L - R], no factor 1/2: only the loader differs.  Row 2 item is the sum row and row
// 2 item + 1 the difference row; the workgroup reads the span of BOTH channels of its item and stores xL r1 + xR r1, respectively
// xL r1 - xR r1 (two products and one add, uncontracted).  Table, workspace and everything behind the span are those of C = 2.
//
// The mel variant (template MEL; auraloss's scale="mel", restated) sums the clamped magnitudes into bands before the two terms are
// taken: M = F |X| with a bank F the caller hands in (stito_mel_bank), sc and lm over frames x n_bins.  Loader, frame loop and FFT
// are unchanged.  Once a frame is transformed, lane l takes the bin pairs (k, N/2 - k), k = l, l + 64, ... <= N/4: the two
// magnitudes of a pair read exactly the two points Z[k] and Z[N/2 - k] of the packed transform, so the lane writes them back over
// those two points (no other lane reads them) and the wave's FFT buffer becomes the frame's magnitudes, still in digit-reversed
// order, with NO extra LDS.  Then lane l owns the bands l, l + 64, ...: one banded dot product each, a chain of explicit fmas in
// bin order over the interleaved weights (weight j of band m at w[j * stride + m]: the lanes read consecutive floats per step).
// The table holds frames x n_bins mel magnitudes per (row, resolution) and sum M_y^2; sums, tile tree and final launch are shared.
//
// The prefiltered variants (template PRE; auraloss's perceptual_weighting=True, restated, and any other odd-length FIR) put one stage
// into the loader of each of the three: p[i] = sum_k taps[k] x[i + k - c], c = n_taps / 2, x zero outside the row -- conv1d with
// zero padding -- on the normalised (and, under SD, combined) row, and everything behind the loader sees p: the STFT's reflect
// padding reflects the FILTERED row.  The reflected sample indices of a tile's span form one contiguous run [s_min, s_max] of the
// row, so the workgroup stages the raw run [s_min - c, s_max + c] where the span will lie, every thread filters runs of four
// consecutive outputs from a sliding register window (ad_fir_run of audio_distance.h), keeps them in registers across a barrier,
// writes them over the raw run, and a second register pass lays the span out through the reflection.  LDS grows by the filter's
// reach (256 floats), not by a second span.  audio_distance.h holds what this file shares with waveform.hip: the slot rule, the folded
// peak, that FIR run, the tile tree and the host checks of a loss call and of the taps.
#include "audio_distance.h"

#include <type_traits>

namespace stito {

static constexpr int MR_THREADS = 256, MR_WAVES = MR_THREADS / 64;
static constexpr int MR_MAX_RES = 8;
static constexpr int MR_MAX_CH = 8;  // the final sum gives one lane of a wave to every (resolution, channel)
// The prefilter (up to AD_MAX_TAPS taps, the raw run reaches AD_TAP_REACH samples past its last whole float4): a thread filters
// MR_PF_GROUPS runs of four outputs and holds them in registers, so a prefiltered tile's span has at most MR_PF_MAX_SPAN samples.
static constexpr int MR_PF_GROUPS = 8;
static constexpr int MR_PF_MAX_SPAN = 4 * MR_PF_GROUPS * MR_THREADS;

// Everything the launches of one (resolutions, n) need, worked out once on the host: frames, tiles, LDS, and where the
// pieces of the table and of the workspace lie.  Table (floats; every offset even, so doubles and float2 are aligned):
//   per resolution   n_fft / 2 float2 exp(-2 pi i t / n_fft), then the n_fft window values          at hdr_off[i]
//   per row          per resolution frames x bins magnitudes, bins contiguous                       at mags_base + row * row_floats + mag_off[i]
//   rows x n_res     doubles: sum |Y|^2                                                             at mags_base + rows * row_floats
//   rows x tiles_total doubles: its per-tile partial sums (scratch of stito_mrstft_target)          behind them
struct MrPlan {
    int n_res;
    int nfft[MR_MAX_RES], hop[MR_MAX_RES], win[MR_MAX_RES], log2_n2[MR_MAX_RES], F[MR_MAX_RES];
    int64_t T[MR_MAX_RES], tiles[MR_MAX_RES], bins[MR_MAX_RES];  // bins: the columns of a table row (mel: the bands)
    size_t lds[MR_MAX_RES];
    int64_t hdr_off[MR_MAX_RES], mag_off[MR_MAX_RES], tile_off[MR_MAX_RES];
    int64_t row_floats, mags_base, tiles_total;
};

static size_t mr_lds_bytes(int N, int hop, int F, bool pre = false) {
    // tile sums (2 x MR_THREADS doubles) + one FFT buffer per wave + twiddles + window + sample span
    const size_t plain = (size_t)2 * MR_THREADS * 8 + (size_t)MR_WAVES * (N / 2) * 8 + (size_t)(N / 2) * 8 + (size_t)N * 4 +
                         ((size_t)(F - 1) * hop + N) * 4;
    // prefiltered: the span rounded up to whole float4 and the filter's reach behind the raw run (whole tap blocks)
    return pre ? plain + (size_t)(4 + AD_TAP_REACH) * 4 : plain;
}

// n_bins: 0 for the linear table (a row of a frame is its n_fft / 2 + 1 bins), else the bands of the mel table.  The LDS, the
// tiles and the workspace do not depend on it.  pre: the plan of the prefiltered kernels, whose LDS is larger and whose span is
// bounded, so F, the tiles and with them the table's scratch and the workspace may differ from the plain plan's.
static int mr_plan(const int *res, int n_res, int64_t n, MrPlan &p, int n_bins = 0, bool pre = false) {
    STITO_REQUIRE(res != nullptr, STITO_E_INVALID, "mrstft: null resolutions");
    STITO_REQUIRE(n_res >= 1 && n_res <= MR_MAX_RES, STITO_E_INVALID, "mrstft: %d resolutions, 1 .. %d are supported", n_res, MR_MAX_RES);
    // gfx950's LDS per workgroup: the plan also sizes the table and the workspace, so it asks no device (mr_device_fits does)
    const size_t lds_cap = 160 * 1024;
    p.n_res = n_res;
    int64_t hdr = 0, mag = 0, tl = 0;
    for (int i = 0; i < n_res; ++i) {
        const int N = res[3 * i], hop = res[3 * i + 1], win = res[3 * i + 2];
        STITO_REQUIRE(N >= 256 && N <= 4096 && (N & (N - 1)) == 0, STITO_E_INVALID, "mrstft: n_fft %d must be a power of two in [256, 4096]", N);
        STITO_REQUIRE(hop >= 1, STITO_E_INVALID, "mrstft: hop %d must be at least 1", hop);
        STITO_REQUIRE(win >= 1 && win <= N, STITO_E_INVALID, "mrstft: window of %d points does not fit n_fft %d", win, N);
        STITO_REQUIRE(n > N / 2, STITO_E_INVALID, "mrstft: %lld samples are too few for the reflect padding of n_fft %d", (long long)n, N);
        STITO_REQUIRE(n < ((int64_t)1 << 40), STITO_E_INVALID, "mrstft: %lld samples", (long long)n);
        p.nfft[i] = N; p.hop[i] = hop; p.win[i] = win;
        int l2 = 0;
        while ((1 << l2) < N / 2) ++l2;
        p.log2_n2[i] = l2;
        p.T[i] = 1 + n / hop;
        p.bins[i] = n_bins > 0 ? n_bins : N / 2 + 1;
        // frames per tile: as many as 32 while two workgroups fit a CU's 160 KB of LDS, else what one workgroup can hold
        static const int cand_F[] = {32, 28, 24, 20, 16, 12, 8, 4, 2, 1};
        int F = 0;
        for (size_t budget : {(size_t)80 * 1024, lds_cap}) {
            for (int f : cand_F) {
                if (pre && (int64_t)(f - 1) * hop + N > MR_PF_MAX_SPAN) continue;
                if (mr_lds_bytes(N, hop, f, pre) <= budget && mr_lds_bytes(N, hop, f, pre) <= lds_cap) { F = f; break; }
            }
            if (F) break;
        }
        STITO_REQUIRE(F > 0, STITO_E_UNSUPPORTED, "mrstft: n_fft %d needs %zu bytes of LDS per workgroup, the device has %zu", N,
                      mr_lds_bytes(N, hop, 1, pre), lds_cap);
        p.F[i] = F;
        p.lds[i] = mr_lds_bytes(N, hop, F, pre);
        p.tiles[i] = (p.T[i] + F - 1) / F;
        p.hdr_off[i] = hdr; hdr += 2 * (int64_t)N;
        p.mag_off[i] = mag; mag += (p.T[i] * p.bins[i] + 1) / 2 * 2;
        p.tile_off[i] = tl; tl += p.tiles[i];
    }
    p.mags_base = hdr; p.row_floats = mag; p.tiles_total = tl;
    return STITO_OK;
}

static int mr_device_fits(const MrPlan &p) {
    DeviceInfo di;
    STITO_TRY(device_info(di));
    for (int i = 0; i < p.n_res; ++i)
        STITO_REQUIRE(p.lds[i] <= (size_t)di.lds_per_block, STITO_E_UNSUPPORTED, "mrstft: n_fft %d needs %zu bytes of LDS per workgroup, the device has %d",
                      p.nfft[i], p.lds[i], di.lds_per_block);
    return STITO_OK;
}

static int64_t mr_table_floats(const MrPlan &p, int64_t rows) {
    return p.mags_base + rows * p.row_floats + 2 * rows * p.n_res + 2 * rows * p.tiles_total;
}

struct MrDev {
    int N, N2, log2_n2, hop, F, tiles;
    int64_t T, bins, n;
    const float2 *tw;     // exp(-2 pi i t / N), t < N2
    const float *win;     // N window values (zero outside the Hann of `win` points)
    float *mags;          // the table's row blocks + this resolution's offset; row stride row_floats
    int64_t row_floats;
    double *partial;      // [row][tiles_total][K] + this resolution's tile offset * K
    int64_t tiles_total;
};

// The mel kernels' argument: MrDev (whose `bins` is then n_bins, the columns of the table) and this resolution's bank.  The
// linear kernels keep MrDev itself, so their argument layout and code are what they were.
struct MrDevMel : MrDev {
    int n_bins, w_stride, w_rows;   // weight j < w_rows of band m at w[j * w_stride + m]
    const int32_t *band_start;      // [n_bins] first bin of the band
    const int32_t *band_len;        // [n_bins] its number of consecutive bins
    const float *w;
};
template <bool MEL> using MrDevOf = std::conditional_t<MEL, MrDevMel, MrDev>;

// The prefiltered kernels' argument: the argument of their kind with the taps behind it.  The kernels without PRE keep theirs.
template <class Base> struct MrDevPre : Base {
    const float *taps;   // [n_taps], n_taps odd
    int n_taps;
};
template <bool MEL, bool PRE> using MrArgOf = std::conditional_t<PRE, MrDevPre<MrDevOf<MEL>>, MrDevOf<MEL>>;

__device__ __forceinline__ float2 mr_cmul(float2 a, float2 b) {  // explicit fmas: the file is built with -ffp-contract=off
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ float2 mr_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 mr_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// LDS operations of one wave execute in order; this keeps the compiler from moving them and waits for the reads
#define MR_WAVE_SYNC() { __builtin_amdgcn_wave_barrier(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

// Position in the wave's buffer of bin k of the N2-point transform after the in-place stages: stage s of radix r_s sends
// the bins with k mod r_s = d to sub-block d, so the digits of k (least significant first) become those of the position
// (most significant first).  Radix-4 stages, then one radix-2 stage when log2(N2) is odd.
__device__ __forceinline__ int mr_pos(int k, int log2_n2) {
    const int even = log2_n2 & ~1;
    unsigned v = __brev((unsigned)k & ((1u << even) - 1u)) >> (32 - even);   // bits reversed: digits reversed, each digit's two bits too
    v = ((v & 0x55555555u) << 1) | ((v >> 1) & 0x55555555u);
    return (log2_n2 & 1) ? (int)((v << 1) | ((unsigned)k >> even)) : (int)v;
}

// One frame: samples sp[0 .. N) of the tile's span -> window -> packed complex FFT in buf.  All lanes of the wave.
__device__ __forceinline__ void mr_frame_fft(const MrDev &d, const float *sp, const float *win_s, const float2 *tw_s, float2 *buf, int lane) {
    const int N2 = d.N2;
    for (int m = lane; m < N2; m += 64)
        buf[m] = make_float2(sp[2 * m] * win_s[2 * m], sp[2 * m + 1] * win_s[2 * m + 1]);
    MR_WAVE_SYNC()
    int lm = d.log2_n2;                       // log2 of the current block size
    for (; lm >= 2; lm -= 2) {
        const int q = 1 << (lm - 2);          // quarter of the block
        const int sh = d.log2_n2 + 1 - lm;    // exp(-2 pi i j / block) = tw[j << sh]
        for (int i = lane; i < (N2 >> 2); i += 64) {
            const int j = i & (q - 1);
            const int base = ((i >> (lm - 2)) << lm) + j;
            const float2 w1 = tw_s[j << sh], w2 = tw_s[(2 * j) << sh];
            const float2 w3 = mr_cmul(w1, w2);
            const float2 a0 = buf[base], a1 = buf[base + q], a2 = buf[base + 2 * q], a3 = buf[base + 3 * q];
            const float2 b0 = mr_add(a0, a2), b1 = mr_sub(a0, a2), b2 = mr_add(a1, a3), b3 = mr_sub(a1, a3);
            buf[base] = mr_add(b0, b2);
            buf[base + q] = mr_cmul(make_float2(b1.x + b3.y, b1.y - b3.x), w1);      // (b1 - i b3) w
            buf[base + 2 * q] = mr_cmul(mr_sub(b0, b2), w2);
            buf[base + 3 * q] = mr_cmul(make_float2(b1.x - b3.y, b1.y + b3.x), w3);  // (b1 + i b3) w^3
        }
        MR_WAVE_SYNC()
    }
    if (lm == 1) {
        for (int i = lane; i < (N2 >> 1); i += 64) {
            const float2 a0 = buf[2 * i], a1 = buf[2 * i + 1];
            buf[2 * i] = mr_add(a0, a1);
            buf[2 * i + 1] = mr_sub(a0, a1);
        }
        MR_WAVE_SYNC()
    }
}

// |X[k]| of the real frame from the packed transform Z (digit-reversed in buf): X[k] = E[k] + W^k O[k], clamped like the reference
__device__ __forceinline__ float mr_magnitude(const MrDev &d, const float2 *buf, const float2 *tw_s, int k) {
    const int N2 = d.N2;
    const float2 zk = buf[mr_pos(k & (N2 - 1), d.log2_n2)];
    const float2 zn = buf[mr_pos((N2 - k) & (N2 - 1), d.log2_n2)];
    const float2 E = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    const float2 O = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));  // (zk - conj(zn)) / (2i)
    const float2 w = (k < N2) ? tw_s[k] : make_float2(-1.0f, 0.0f);
    const float2 wo = mr_cmul(w, O);
    const float re = E.x + wo.x, im = E.y + wo.y;
    return sqrtf(fmaxf(fmaf(re, re, im * im), 1e-8f));
}

// The mel variant's two steps on a transformed frame.  mr_mel_magnitudes: buf, as floats, becomes the frame's clamped magnitudes --
// |X[k]|, k < N2, at float 2 mr_pos(k) and |X[N2]| at float 1 (the imaginary slot of point 0, which pairs with itself).  Every
// magnitude is mr_magnitude's value: the linear kernels' float32 bits.
__device__ __forceinline__ void mr_mel_magnitudes(const MrDev &d, float2 *buf, const float2 *tw_s, int lane) {
    const int N2 = d.N2;
    float *mg = (float *)buf;
    for (int k = lane; k <= (N2 >> 1); k += 64) {
        const float a = mr_magnitude(d, buf, tw_s, k), b = mr_magnitude(d, buf, tw_s, N2 - k);
        const int pa = mr_pos(k, d.log2_n2), pb = mr_pos((N2 - k) & (N2 - 1), d.log2_n2);
        mg[2 * pa] = a;  // both points of the pair have been read, and no other lane reads them
        if (k == 0) mg[1] = b; else mg[2 * pb] = b;
    }
    MR_WAVE_SYNC()
}

// Band m of the frame whose magnitudes mr_mel_magnitudes left in buf: sum_j w[j] |X[start + j]|, fmas in bin order.  The run is
// cut to the bins and to the weight rows that exist (the host refuses such a bank; the device tables are not trusted).
__device__ __forceinline__ float mr_mel_band(const MrDevMel &d, const float2 *buf, int m) {
    const float *mg = (const float *)buf;
    const int N2 = d.N2;
    const int s = d.band_start[m];
    int len = d.band_len[m];
    if (s < 0 || s > N2) len = 0;
    if (len > N2 + 1 - s) len = N2 + 1 - s;
    if (len > d.w_rows) len = d.w_rows;
    const float *w = d.w + m;
    float acc = 0.0f;
    // Eight steps at a time, their loads issued together: with two workgroups on a CU nothing else hides the weights' way from L2.
    // A step past the run repeats the run's last bin with weight 0, and fma(0, v, acc) is acc: the bits of the plain chain.
    constexpr int U = 8;
    for (int j0 = 0; j0 < len; j0 += U) {
        float wv[U], mv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u, jc = j < len ? j : len - 1;
            const int k = s + jc;
            const float wl = w[(int64_t)jc * d.w_stride];
            wv[u] = j < len ? wl : 0.0f;
            mv[u] = (k == N2) ? mg[1] : mg[2 * mr_pos(k, d.log2_n2)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = fmaf(wv[u], mv[u], acc);
    }
    return acc;
}

// The prefiltered loader.  span: room for the tile's largest span rounded up to whole float4 and AD_TAP_REACH floats behind it
// (mr_lds_bytes).  On return span[0 .. span_len) holds the reflected FILTERED samples; the caller's barrier
// publishes them.  x, r1, row: as in the plain loader (SD: x is the item's channel 0 and the row's parity picks sum or difference).
template <bool SD>
__device__ __forceinline__ void mr_prefiltered_span(const float *__restrict__ x, int64_t n, float r1, int64_t row, const float *__restrict__ taps,
                                                    int n_taps, float *span, int64_t s0, int span_len, int tid) {
    // the samples the span reflects to: [max(a, 0), min(b, n - 1)], 1 .. -a before the row's start, 2 (n - 1) - b .. n - 2 behind its end
    const int c = n_taps >> 1;
    const int64_t a = s0, b = s0 + span_len - 1;
    int64_t s_min = a < 0 ? 0 : a, s_max = b < n ? b : n - 1;
    if (a < 0 && -a > s_max) s_max = -a;
    if (b >= n && 2 * (n - 1) - b < s_min) s_min = 2 * (n - 1) - b;
    if (s_min < 0) s_min = 0;
    if (s_max > n - 1) s_max = n - 1;
    const int run_len = (int)(s_max - s_min + 1);                 // <= span_len: every sample of the run is some span index's
    const int raw_len = ((run_len + 3) & ~3) + 4 * ((n_taps + 3) >> 2);
    // the raw run [s_min - c, ...), zero outside the row: raw[j] = x[s_min - c + j], so p[s_min + o] = sum_k taps[k] raw[o + k]
    for (int i = tid; i < raw_len; i += MR_THREADS) {
        const int64_t s = s_min - c + i;
        float v = 0.0f;
        if (s >= 0 && s < n) {
            if (SD) {
                const float l = x[s] * r1, r = x[n + s] * r1;
                v = (row & 1) ? l - r : l + r;
            } else {
                v = x[s] * r1;
            }
        }
        span[i] = v;
    }
    __syncthreads();
    // outputs 4 g .. 4 g + 3 of group g; every output's chain runs k = 0 .. n_taps - 1
    float4 out[MR_PF_GROUPS];
#pragma unroll
    for (int gi = 0; gi < MR_PF_GROUPS; ++gi) {
        const int g = tid + gi * MR_THREADS;
        out[gi] = 4 * g < run_len ? ad_fir_run(span, g, taps, n_taps) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();  // the raw run has been read: p goes over it, p[s_min + o] at span[o]
#pragma unroll
    for (int gi = 0; gi < MR_PF_GROUPS; ++gi) {
        const int g = tid + gi * MR_THREADS;
        if (4 * g < run_len) ((float4 *)span)[g] = out[gi];
    }
    __syncthreads();
    // the span through the reflection (no edge repeat), again by way of registers: span index i = padded index s0 + i
    float val[4 * MR_PF_GROUPS];
#pragma unroll
    for (int v = 0; v < 4 * MR_PF_GROUPS; ++v) {
        const int i = tid + v * MR_THREADS;
        val[v] = 0.0f;
        if (i < span_len) {
            int64_t s = s0 + i;
            if (s < 0) s = -s;
            if (s >= n) s = 2 * (n - 1) - s;
            val[v] = span[s - s_min];
        }
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 4 * MR_PF_GROUPS; ++v) {
        const int i = tid + v * MR_THREADS;
        if (i < span_len) span[i] = val[v];
    }
}

// TARGET: audio = y (rows, n); writes the magnitudes and the tile's sum |Y|^2 (K = 1 partial).
// else:   audio = candidates (pop, C, n); row = cand * C + ch is compared with table row ad_target_of(cand) * C + ch;
//         the tile's sum (|Y| - |X|)^2 and sum |ln(|X| / |Y|)| (K = 2 partials).  A candidate whose slot names no target
//         reads nothing from the table and writes no partial: k_mrstft_final gives it NaN.
// SD:     C = 2 and audio = (items, 2, n) on both sides; row 2 item + 0 is the item's L + R, row 2 item + 1 its L - R.
// MEL:    the table's rows are frames x n_bins band sums of the magnitudes, and both terms are taken between those.
// PRE:    the rows are filtered with d.taps in the loader (mr_prefiltered_span) before anything else sees them.
template <bool TARGET, bool SD, bool MEL, bool PRE = false>
__global__ __launch_bounds__(MR_THREADS) void k_mrstft(MrArgOf<MEL, PRE> d, const float *__restrict__ audio, const float *__restrict__ peaks,
                                                      int norm_passes, int C, int per_target, const int32_t *__restrict__ slots,
                                                      int n_targets) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int N = d.N, N2 = d.N2;
    double (*red)[MR_THREADS] = (double (*)[MR_THREADS])smem_raw;   // [2][MR_THREADS]
    float2 *bufs = (float2 *)(red + 2);                             // [MR_WAVES][N2]
    float2 *tw_s = bufs + MR_WAVES * N2;                       // [N2]
    float *win_s = (float *)(tw_s + N2);                       // [N]
    float *span = win_s + N;                                   // [(F - 1) hop + N]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x / d.tiles;
    const int tile = (int)(blockIdx.x - row * d.tiles);
    const int64_t t0 = (int64_t)tile * d.F;
    const int nf = (int)(d.T - t0 < d.F ? d.T - t0 : d.F);

    float r1 = 1.0f;
    int64_t trow = row;
    if (!TARGET) {
        const int64_t cand = row / C;
        const int t = ad_target_of(cand, per_target, slots, n_targets);
        if (t < 0) return;  // the whole workgroup (one row, one candidate), before it loads anything
        r1 = ad_peak_scale(peaks, norm_passes, cand);
        trow = (int64_t)t * C + (row - cand * C);
    }
    const float *x = audio + (SD ? (row & ~(int64_t)1) : row) * d.n;  // SD: the item's channel 0; channel 1 lies behind it

    for (int i = tid; i < N2; i += MR_THREADS) tw_s[i] = d.tw[i];
    for (int i = tid; i < N; i += MR_THREADS) win_s[i] = d.win[i];
    // the span: padded samples [t0 hop, t0 hop + (nf - 1) hop + N), padded index i = sample i - N / 2, reflected (no edge repeat)
    const int span_len = (nf - 1) * d.hop + N;
    const int64_t s0 = t0 * d.hop - N2;
    if constexpr (PRE) {
        mr_prefiltered_span<SD>(x, d.n, r1, row, d.taps, d.n_taps, span, s0, span_len, tid);
    } else {
        for (int i = tid; i < span_len; i += MR_THREADS) {
            int64_t s = s0 + i;
            if (s < 0) s = -s;
            if (s >= d.n) s = 2 * (d.n - 1) - s;
            if (SD) {
                const float l = x[s] * r1, r = x[d.n + s] * r1;
                span[i] = (row & 1) ? l - r : l + r;
            } else {
                span[i] = x[s] * r1;
            }
        }
    }
    __syncthreads();

    double acc0 = 0.0, acc1 = 0.0;
    float2 *buf = bufs + wave * N2;
    float *mags = d.mags + trow * d.row_floats;
    for (int f = wave; f < nf; f += MR_WAVES) {
        mr_frame_fft(d, span + f * d.hop, win_s, tw_s, buf, lane);
        float *mrow = mags + (t0 + f) * d.bins;
        if constexpr (MEL) mr_mel_magnitudes(d, buf, tw_s, lane);
        for (int k = lane; k <= (MEL ? (int)d.bins - 1 : N2); k += 64) {  // k: a bin, or a band of the mel table
            float mx;
            if constexpr (MEL) mx = mr_mel_band(d, buf, k); else mx = mr_magnitude(d, buf, tw_s, k);
            if (TARGET) {
                mrow[k] = mx;
                acc0 += (double)(mx * mx);
            } else {
                const float my = mrow[k];
                const float df = my - mx;
                acc0 += (double)(df * df);
                acc1 += (double)fabsf(logf(mx / my));
            }
        }
        MR_WAVE_SYNC()  // the spectrum has been read before the next frame is packed over it
    }

    const double acc[2] = {acc0, acc1};
    ad_tile_tree<2, MR_THREADS>(red, acc, tid);
    if (tid == 0) {
        constexpr int K = TARGET ? 1 : 2;
        double *out = d.partial + (row * d.tiles_total + tile) * K;
        out[0] = red[0][0];
        if (!TARGET) out[1] = red[1][0];
    }
}

// exp(-2 pi i t / N), t < N / 2, and the periodic Hann of `win` points in the middle of N: float64, rounded once
__global__ void k_mrstft_tables(float2 *tw, float *window, int N, int win) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N / 2) {
        double s, c;
        sincospi(-2.0 * (double)i / (double)N, &s, &c);
        tw[i] = make_float2((float)c, (float)s);
    }
    if (i < N) {
        const int lo = (N - win) / 2, k = i - lo;
        window[i] = (k >= 0 && k < win) ? (float)(0.5 - 0.5 * cospi(2.0 * (double)k / (double)win)) : 0.0f;
    }
}

struct MrSum {
    int n_res;
    int tiles[MR_MAX_RES], tile_off[MR_MAX_RES];
    double count[MR_MAX_RES];  // frames x bins
    int64_t tiles_total;
};

// sum |Y|^2 per (row, resolution): the tiles in order
__global__ void k_mrstft_target_sum(MrSum s, const double *__restrict__ partial, int64_t rows, double *__restrict__ sums) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * s.n_res) return;
    const int64_t row = i / s.n_res;
    const int r = (int)(i - row * s.n_res);
    const double *p = partial + row * s.tiles_total + s.tile_off[r];
    double acc = 0.0;
    for (int t = 0; t < s.tiles[r]; ++t) acc += p[t];
    sums[i] = acc;
}

// one wave per candidate: lane (resolution, channel) adds its tiles in order, lane 0 the means in order
__global__ __launch_bounds__(64) void k_mrstft_final(MrSum s, const double *__restrict__ partial, const double *__restrict__ ysum, int C,
                                                     int per_target, const int32_t *__restrict__ slots, int n_targets,
                                                     float *__restrict__ loss) {
    __shared__ double term[64];
    const int cand = blockIdx.x, lane = threadIdx.x;
    const int tgt = ad_target_of(cand, per_target, slots, n_targets);
    if (tgt < 0) {  // the whole wave: no partial was written for this candidate and none is read
        if (lane == 0) loss[cand] = __builtin_nanf("");
        return;
    }
    if (lane < s.n_res * C) {
        const int r = lane / C, ch = lane - r * C;
        const int64_t row = (int64_t)cand * C + ch, trow = (int64_t)tgt * C + ch;
        const double *p = partial + (row * s.tiles_total + s.tile_off[r]) * 2;
        double d2 = 0.0, lg = 0.0;
        for (int t = 0; t < s.tiles[r]; ++t) { d2 += p[2 * t]; lg += p[2 * t + 1]; }
        term[lane] = sqrt(d2) / sqrt(ysum[trow * s.n_res + r]) + lg / s.count[r];
    }
    __syncthreads();
    if (lane == 0) {
        double total = 0.0;
        for (int r = 0; r < s.n_res; ++r) {
            double acc = 0.0;
            for (int ch = 0; ch < C; ++ch) acc += term[r * C + ch];
            total += acc / C;
        }
        loss[cand] = (float)(total / s.n_res);
    }
}

static MrDev mr_dev(const MrPlan &p, int i, int64_t n, float *table, double *partial, int K) {
    MrDev d;
    d.N = p.nfft[i]; d.N2 = d.N / 2; d.log2_n2 = p.log2_n2[i]; d.hop = p.hop[i]; d.F = p.F[i]; d.tiles = (int)p.tiles[i];
    d.T = p.T[i]; d.bins = p.bins[i]; d.n = n;
    d.tw = (const float2 *)(table + p.hdr_off[i]);
    d.win = table + p.hdr_off[i] + d.N;
    d.mags = table + p.mags_base + p.mag_off[i];
    d.row_floats = p.row_floats;
    d.partial = partial + p.tile_off[i] * K;
    d.tiles_total = p.tiles_total;
    return d;
}

// The bank as the calls take it, checked on the host tables before a device is asked anything.
static int mr_bank_check(const char *who, const stito_mel_bank *b, const int *res, int n_res) {
    STITO_REQUIRE(b != nullptr, STITO_E_INVALID, "%s: null bank", who);
    STITO_REQUIRE(b->n_bins >= 1 && b->n_bins <= 256, STITO_E_INVALID, "%s: n_bins %d, 1 .. 256 are supported", who, b->n_bins);
    STITO_REQUIRE(res != nullptr && n_res >= 1 && n_res <= MR_MAX_RES, STITO_E_INVALID, "%s: %d resolutions, 1 .. %d are supported", who, n_res, MR_MAX_RES);
    STITO_REQUIRE(b->n_res == n_res, STITO_E_INVALID, "%s: the bank covers %d resolutions, the call has %d", who, b->n_res, n_res);
    STITO_REQUIRE(b->band_start != nullptr && b->band_len != nullptr && b->band_start_dev != nullptr && b->band_len_dev != nullptr &&
                      b->weights_dev != nullptr, STITO_E_INVALID, "%s: null bank table", who);
    for (int i = 0; i < n_res; ++i) {
        const int bins = res[3 * i] / 2 + 1;
        STITO_REQUIRE(b->w_offset[i] >= 0 && b->w_rows[i] >= 1 && b->w_stride[i] >= b->n_bins, STITO_E_INVALID,
                      "%s: weights of resolution %d: offset %lld, %d rows of %d floats for %d bands", who, i, (long long)b->w_offset[i],
                      b->w_rows[i], b->w_stride[i], b->n_bins);
        for (int m = 0; m < b->n_bins; ++m) {
            const int s = b->band_start[i * b->n_bins + m], len = b->band_len[i * b->n_bins + m];
            STITO_REQUIRE(len >= 0 && len <= bins && len <= b->w_rows[i], STITO_E_INVALID,
                          "%s: band %d of resolution %d (n_fft %d) is %d bins long: there are %d bins and %d weight rows", who, m, i, res[3 * i],
                          len, bins, b->w_rows[i]);
            STITO_REQUIRE(s >= 0 && s <= bins - len, STITO_E_INVALID, "%s: band %d of resolution %d (n_fft %d) starts at bin %d with %d bins: there are %d",
                          who, m, i, res[3 * i], s, len, bins);
        }
    }
    return STITO_OK;
}

static MrDevMel mr_dev_mel(const MrDev &lin, const stito_mel_bank *b, int i) {
    MrDevMel d;
    static_cast<MrDev &>(d) = lin;
    d.n_bins = b->n_bins; d.w_stride = b->w_stride[i]; d.w_rows = b->w_rows[i];
    d.band_start = b->band_start_dev + (int64_t)i * b->n_bins;
    d.band_len = b->band_len_dev + (int64_t)i * b->n_bins;
    d.w = b->weights_dev + b->w_offset[i];
    return d;
}

// The kernel's argument of resolution i: MrDev, or with the bank's tables behind it.
template <bool MEL>
static MrDevOf<MEL> mr_dev_of(const MrPlan &p, int i, int64_t n, float *table, double *partial, int K, const stito_mel_bank *bank) {
    const MrDev d = mr_dev(p, i, n, table, partial, K);
    if constexpr (MEL) return mr_dev_mel(d, bank, i); else return d;
}

// ... and, for the prefiltered kernels, with the taps behind that.
template <bool MEL, bool PRE>
static MrArgOf<MEL, PRE> mr_arg_of(const MrPlan &p, int i, int64_t n, float *table, double *partial, int K, const stito_mel_bank *bank,
                                   const float *taps_dev, int n_taps) {
    const MrDevOf<MEL> d = mr_dev_of<MEL>(p, i, n, table, partial, K, bank);
    if constexpr (PRE) {
        MrDevPre<MrDevOf<MEL>> a;
        static_cast<MrDevOf<MEL> &>(a) = d;
        a.taps = taps_dev; a.n_taps = n_taps;
        return a;
    } else {
        return d;
    }
}

static MrSum mr_sum(const MrPlan &p) {
    MrSum s;
    s.n_res = p.n_res; s.tiles_total = p.tiles_total;
    for (int i = 0; i < MR_MAX_RES; ++i) {
        const bool live = i < p.n_res;
        s.tiles[i] = live ? (int)p.tiles[i] : 0;
        s.tile_off[i] = live ? (int)p.tile_off[i] : 0;
        s.count[i] = live ? (double)p.T[i] * (double)p.bins[i] : 1.0;
    }
    return s;
}

}  // namespace stito

using namespace stito;

extern "C" int64_t stito_mrstft_table_floats(const int *res, int n_res, int rows, int64_t n_samples) {
    MrPlan p;
    if (rows < 1 || mr_plan(res, n_res, n_samples, p) != STITO_OK) return 0;
    return mr_table_floats(p, rows);
}

extern "C" size_t stito_mrstft_workspace_bytes(const int *res, int n_res, int pop, int channels, int64_t n_samples) {
    MrPlan p;
    if (pop < 1 || channels < 1 || mr_plan(res, n_res, n_samples, p) != STITO_OK) return 0;
    return (size_t)pop * channels * p.tiles_total * 2 * sizeof(double);
}

// The sum / difference variant takes 2-channel items only: its rows are an item's L + R and L - R.
static int mr_sd_channels(const char *who, int channels) {
    STITO_REQUIRE(channels == 2, STITO_E_INVALID, "%s: the sum / difference distance needs 2 channels, got %d", who, channels);
    return STITO_OK;
}

// The one launch path of the table.  SD: y_dev is (rows / 2, 2, n) and row 2 t + 0 / 1 of the table is target t's L + R / L - R.
// MEL: the rows of the table are band sums through `bank`, which has been checked.
// PRE: the rows are filtered with the n_taps taps at taps_dev, which have been checked.
template <bool SD, bool MEL, bool PRE>
static int mr_target(const char *who, const int *res, int n_res, const float *y_dev, int rows, int64_t n_samples, float *table_dev,
                     void *stream, const stito_mel_bank *bank, const float *taps_dev, int n_taps) {
    hipStream_t st = (hipStream_t)stream;
    MrPlan p;
    STITO_TRY(mr_plan(res, n_res, n_samples, p, MEL ? bank->n_bins : 0, PRE));
    STITO_TRY(mr_device_fits(p));
    STITO_REQUIRE(rows >= 1, STITO_E_INVALID, "%s: %d rows", who, rows);
    STITO_REQUIRE(y_dev != nullptr && table_dev != nullptr, STITO_E_INVALID, "%s: null pointer", who);
    STITO_REQUIRE(((uintptr_t)table_dev & 15) == 0, STITO_E_INVALID, "%s: the table must be 16-byte aligned", who);
    double *sums = (double *)(table_dev + p.mags_base + (int64_t)rows * p.row_floats);
    double *partial = sums + (int64_t)rows * p.n_res;
    for (int i = 0; i < p.n_res; ++i) {
        STITO_REQUIRE((int64_t)rows * p.tiles[i] < ((int64_t)1 << 31), STITO_E_UNSUPPORTED, "%s: too many tiles", who);
        const MrArgOf<MEL, PRE> d = mr_arg_of<MEL, PRE>(p, i, n_samples, table_dev, partial, 1, bank, taps_dev, n_taps);
        hipLaunchKernelGGL(k_mrstft_tables, dim3((d.N + 255) / 256), dim3(256), 0, st, (float2 *)d.tw, (float *)d.win, d.N, p.win[i]);
        STITO_LAUNCH_CHECK();
        STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_mrstft<true, SD, MEL, PRE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds[i]));
        hipLaunchKernelGGL((k_mrstft<true, SD, MEL, PRE>), dim3((unsigned)(rows * p.tiles[i])), dim3(MR_THREADS), p.lds[i], st, d, y_dev,
                           (const float *)nullptr, 0, 1, 1, (const int32_t *)nullptr, rows);
        STITO_LAUNCH_CHECK();
    }
    const int64_t n_sums = (int64_t)rows * p.n_res;
    hipLaunchKernelGGL(k_mrstft_target_sum, dim3((unsigned)((n_sums + 63) / 64)), dim3(64), 0, st, mr_sum(p), partial, (int64_t)rows, sums);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

// The one launch path of the loss: populations of pop / n_slots candidates, population k against target target_slot[k] of the
// table's n_targets, or against target k when there is no slot list (then n_slots == n_targets).
template <bool SD, bool MEL, bool PRE>
static int mr_loss(const char *who, const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                   const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots, int pop, int channels,
                   int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream,
                   const stito_mel_bank *bank, const float *taps_dev, int n_taps) {
    hipStream_t st = (hipStream_t)stream;
    MrPlan p;
    STITO_TRY(mr_plan(res, n_res, n_samples, p, MEL ? bank->n_bins : 0, PRE));
    STITO_TRY(mr_device_fits(p));
    STITO_TRY(ad_loss_args_check(who, pop, n_targets, n_slots, [&] {
        if (SD) STITO_TRY(mr_sd_channels(who, channels));
        STITO_REQUIRE(channels >= 1 && channels <= MR_MAX_CH && n_res * channels <= 64, STITO_E_INVALID, "Invalid number of channels: %d", channels);
        return STITO_OK;
    }, norm_passes, peaks_dev, audio_dev, table_dev, loss_dev));
    const int64_t rows = (int64_t)pop * channels, trows = (int64_t)n_targets * channels;
    STITO_TRY(ad_workspace_check(who, workspace_dev, workspace_bytes, (size_t)rows * p.tiles_total * 2 * sizeof(double)));
    for (int i = 0; i < p.n_res; ++i)
        STITO_REQUIRE(rows * p.tiles[i] < ((int64_t)1 << 31), STITO_E_UNSUPPORTED, "%s: too many tiles", who);
    double *partial = (double *)workspace_dev;
    const double *ysum = (const double *)(table_dev + p.mags_base + trows * p.row_floats);
    for (int i = 0; i < p.n_res; ++i) {
        const MrArgOf<MEL, PRE> d = mr_arg_of<MEL, PRE>(p, i, n_samples, (float *)table_dev, partial, 2, bank, taps_dev, n_taps);
        STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_mrstft<false, SD, MEL, PRE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds[i]));
        hipLaunchKernelGGL((k_mrstft<false, SD, MEL, PRE>), dim3((unsigned)(rows * p.tiles[i])), dim3(MR_THREADS), p.lds[i], st, d, audio_dev,
                           peaks_dev, norm_passes, channels, pop / n_slots, target_slot_dev, n_targets);
        STITO_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_mrstft_final, dim3((unsigned)pop), dim3(64), 0, st, mr_sum(p), partial, ysum, channels, pop / n_slots,
                       target_slot_dev, n_targets, loss_dev);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

// The prefiltered calls' own arguments (ABI 10.9): kind -- 0 the L/R distance, 1 sum / difference, 2 mel (with its bank) -- and the
// taps.  The table does not record the taps: table and loss calls take the same.
static int mr_pf_check(const char *who, int kind, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res, int n_res) {
    STITO_REQUIRE(kind >= 0 && kind <= 2, STITO_E_INVALID, "%s: kind %d is none of 0 (L/R), 1 (sum / difference), 2 (mel)", who, kind);
    STITO_TRY(ad_taps_check(who, taps_dev, n_taps, false));
    if (kind == 2) return mr_bank_check(who, bank, res, n_res);
    STITO_REQUIRE(bank == nullptr, STITO_E_INVALID, "%s: kind %d takes no bank", who, kind);
    return STITO_OK;
}

// (kind, prefiltered) -> the <SD, MEL, PRE> instantiation, stated once: f(sd, mel, pre) with three std::bool_constant.
template <class F>
static auto mr_dispatch(int kind, bool pre, F &&f) {
    using Y = std::true_type; using N = std::false_type;
    switch (kind) {
        case 1: return pre ? f(Y{}, N{}, Y{}) : f(Y{}, N{}, N{});
        case 2: return pre ? f(N{}, Y{}, Y{}) : f(N{}, Y{}, N{});
        default: return pre ? f(N{}, N{}, Y{}) : f(N{}, N{}, N{});
    }
}

// What every table export ends in, its own arguments checked: the table of `rows` rows of that kind, prefiltered or not.
static int mr_target_call(const char *who, int kind, bool pre, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res,
                          int n_res, const float *y_dev, int rows, int64_t n_samples, float *table_dev, void *stream) {
    return mr_dispatch(kind, pre, [&](auto sd, auto mel, auto pf) {
        return mr_target<sd.value, mel.value, pf.value>(who, res, n_res, y_dev, rows, n_samples, table_dev, stream, bank, taps_dev, n_taps);
    });
}

// What every loss export is: the checks of its own arguments in the order they have always been made -- a prefiltered call's kind,
// taps and (sum / difference) 2 channels, a mel call's bank, the slot list where the call takes one -- and mr_loss of that kind.
static int mr_loss_call(const char *who, int kind, bool pre, bool slots, const stito_mel_bank *bank, const float *taps_dev, int n_taps,
                        const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes, const float *table_dev,
                        int n_targets, const int32_t *target_slot_dev, int n_slots, int pop, int channels, int64_t n_samples, float *loss_dev,
                        void *workspace_dev, size_t workspace_bytes, void *stream) {
    if (pre) STITO_TRY(mr_pf_check(who, kind, bank, taps_dev, n_taps, res, n_res));
    if (pre && kind == 1) STITO_TRY(mr_sd_channels(who, channels));
    if (!pre && kind == 2) STITO_TRY(mr_bank_check(who, bank, res, n_res));
    if (slots) STITO_REQUIRE(target_slot_dev != nullptr, STITO_E_INVALID, "%s: null target_slot_dev", who);
    return mr_dispatch(kind, pre, [&](auto sd, auto mel, auto pf) {
        return mr_loss<sd.value, mel.value, pf.value>(who, res, n_res, audio_dev, peaks_dev, norm_passes, table_dev, n_targets,
                                                      slots ? target_slot_dev : nullptr, slots ? n_slots : n_targets, pop, channels, n_samples,
                                                      loss_dev, workspace_dev, workspace_bytes, stream, bank, taps_dev, n_taps);
    });
}

extern "C" int stito_mrstft_target(const int *res, int n_res, const float *y_dev, int rows, int64_t n_samples, float *table_dev,
                                   void *stream) {
    return mr_target_call("stito_mrstft_target", 0, false, nullptr, nullptr, 0, res, n_res, y_dev, rows, n_samples, table_dev, stream);
}

extern "C" int stito_mrstft_loss(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                                 const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples, float *loss_dev,
                                 void *workspace_dev, size_t workspace_bytes, void *stream) {
    return mr_loss_call("stito_mrstft_loss", 0, false, false, nullptr, nullptr, 0, res, n_res, audio_dev, peaks_dev, norm_passes, table_dev,
                        n_targets, nullptr, 0, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int stito_mrstft_loss_slots(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                                       const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots, int pop,
                                       int channels, int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes,
                                       void *stream) {
    return mr_loss_call("stito_mrstft_loss_slots", 0, false, true, nullptr, nullptr, 0, res, n_res, audio_dev, peaks_dev, norm_passes, table_dev,
                        n_targets, target_slot_dev, n_slots, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

// The sum / difference variants (ABI 10.7): the same calls on the 2-channel signal [L + R, L - R] of every item, against a table
// that stito_mrstft_target_sd wrote.
extern "C" int stito_mrstft_target_sd(const int *res, int n_res, const float *y_dev, int n_targets, int channels, int64_t n_samples,
                                      float *table_dev, void *stream) {
    const char *who = "stito_mrstft_target_sd";
    STITO_TRY(mr_sd_channels(who, channels));
    STITO_REQUIRE(n_targets >= 1 && n_targets < (1 << 30), STITO_E_INVALID, "%s: %d targets", who, n_targets);
    return mr_target_call(who, 1, false, nullptr, nullptr, 0, res, n_res, y_dev, 2 * n_targets, n_samples, table_dev, stream);
}

extern "C" int stito_mrstft_loss_sd(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                                    const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples, float *loss_dev,
                                    void *workspace_dev, size_t workspace_bytes, void *stream) {
    return mr_loss_call("stito_mrstft_loss_sd", 1, false, false, nullptr, nullptr, 0, res, n_res, audio_dev, peaks_dev, norm_passes, table_dev,
                        n_targets, nullptr, 0, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int stito_mrstft_loss_slots_sd(const int *res, int n_res, const float *audio_dev, const float *peaks_dev, int norm_passes,
                                          const float *table_dev, int n_targets, const int32_t *target_slot_dev, int n_slots, int pop,
                                          int channels, int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes,
                                          void *stream) {
    return mr_loss_call("stito_mrstft_loss_slots_sd", 1, false, true, nullptr, nullptr, 0, res, n_res, audio_dev, peaks_dev, norm_passes,
                        table_dev, n_targets, target_slot_dev, n_slots, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

// The mel variants (ABI 10.8): the L/R calls with band sums M = F |X| in the place of the magnitudes, F the caller's bank.
extern "C" int64_t stito_mrstft_table_floats_mel(const int *res, int n_res, int n_bins, int rows, int64_t n_samples) {
    MrPlan p;
    if (rows < 1 || n_bins < 1 || n_bins > 256 || mr_plan(res, n_res, n_samples, p, n_bins) != STITO_OK) return 0;
    return mr_table_floats(p, rows);
}

extern "C" int stito_mrstft_target_mel(const int *res, int n_res, const stito_mel_bank *bank, const float *y_dev, int rows,
                                       int64_t n_samples, float *table_dev, void *stream) {
    STITO_TRY(mr_bank_check("stito_mrstft_target_mel", bank, res, n_res));
    return mr_target_call("stito_mrstft_target_mel", 2, false, bank, nullptr, 0, res, n_res, y_dev, rows, n_samples, table_dev, stream);
}

extern "C" int stito_mrstft_loss_mel(const int *res, int n_res, const stito_mel_bank *bank, const float *audio_dev, const float *peaks_dev,
                                     int norm_passes, const float *table_dev, int n_targets, int pop, int channels, int64_t n_samples,
                                     float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return mr_loss_call("stito_mrstft_loss_mel", 2, false, false, bank, nullptr, 0, res, n_res, audio_dev, peaks_dev, norm_passes, table_dev,
                        n_targets, nullptr, 0, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int stito_mrstft_loss_slots_mel(const int *res, int n_res, const stito_mel_bank *bank, const float *audio_dev,
                                           const float *peaks_dev, int norm_passes, const float *table_dev, int n_targets,
                                           const int32_t *target_slot_dev, int n_slots, int pop, int channels, int64_t n_samples,
                                           float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return mr_loss_call("stito_mrstft_loss_slots_mel", 2, false, true, bank, nullptr, 0, res, n_res, audio_dev, peaks_dev, norm_passes,
                        table_dev, n_targets, target_slot_dev, n_slots, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

// The prefiltered variants (ABI 10.9): one trio for the three kinds of rows that the loader filters with n_taps taps.
static bool mr_pf_sizes_ok(int kind, int n_bins, int n_taps) {
    if (kind < 0 || kind > 2 || n_taps < 1 || n_taps > AD_MAX_TAPS || (n_taps & 1) == 0) return false;
    return kind == 2 ? (n_bins >= 1 && n_bins <= 256) : n_bins == 0;
}

extern "C" int64_t stito_mrstft_table_floats_pf(int kind, int n_bins, int n_taps, const int *res, int n_res, int rows, int64_t n_samples) {
    MrPlan p;
    if (!mr_pf_sizes_ok(kind, n_bins, n_taps) || rows < 1 || (kind == 1 && (rows & 1))) return 0;
    if (mr_plan(res, n_res, n_samples, p, n_bins, true) != STITO_OK) return 0;
    return mr_table_floats(p, rows);
}

extern "C" size_t stito_mrstft_workspace_bytes_pf(int kind, int n_taps, const int *res, int n_res, int pop, int channels, int64_t n_samples) {
    MrPlan p;
    if (!mr_pf_sizes_ok(kind, kind == 2 ? 1 : 0, n_taps) || pop < 1 || channels < 1 || channels > MR_MAX_CH || (kind == 1 && channels != 2))
        return 0;
    if (mr_plan(res, n_res, n_samples, p, 0, true) != STITO_OK || n_res * channels > 64) return 0;
    return (size_t)pop * channels * p.tiles_total * 2 * sizeof(double);
}

extern "C" int stito_mrstft_target_pf(int kind, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res, int n_res,
                                      const float *y_dev, int n_targets, int channels, int64_t n_samples, float *table_dev, void *stream) {
    const char *who = "stito_mrstft_target_pf";
    STITO_TRY(mr_pf_check(who, kind, bank, taps_dev, n_taps, res, n_res));
    if (kind == 1) STITO_TRY(mr_sd_channels(who, channels));
    STITO_REQUIRE(n_targets >= 1 && channels >= 1 && (int64_t)n_targets * channels < (1 << 30), STITO_E_INVALID, "%s: %d targets of %d channels",
                  who, n_targets, channels);
    return mr_target_call(who, kind, true, bank, taps_dev, n_taps, res, n_res, y_dev, n_targets * channels, n_samples, table_dev, stream);
}

extern "C" int stito_mrstft_loss_pf(int kind, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res, int n_res,
                                    const float *audio_dev, const float *peaks_dev, int norm_passes, const float *table_dev, int n_targets,
                                    int pop, int channels, int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes,
                                    void *stream) {
    return mr_loss_call("stito_mrstft_loss_pf", kind, true, false, bank, taps_dev, n_taps, res, n_res, audio_dev, peaks_dev, norm_passes, table_dev,
                        n_targets, nullptr, 0, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int stito_mrstft_loss_slots_pf(int kind, const stito_mel_bank *bank, const float *taps_dev, int n_taps, const int *res, int n_res,
                                          const float *audio_dev, const float *peaks_dev, int norm_passes, const float *table_dev,
                                          int n_targets, const int32_t *target_slot_dev, int n_slots, int pop, int channels,
                                          int64_t n_samples, float *loss_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    return mr_loss_call("stito_mrstft_loss_slots_pf", kind, true, true, bank, taps_dev, n_taps, res, n_res, audio_dev, peaks_dev, norm_passes,
                        table_dev, n_targets, target_slot_dev, n_slots, pop, channels, n_samples, loss_dev, workspace_dev, workspace_bytes, stream);
}

