// fft_mixed.hip -- the bark spectrum of features.hip (k_stft_feature MODE 0) for FFT sizes that are not powers of two:
// any even length in [128, 96000] whose prime factors lie in {2, 3, 5, 7}.  The reference's MIR metric calls
// compute_barkspectrum(x, sample_rate, mode="mono") (st_ito/utils.py:83), which binds the sample rate to fft_size: a 48 000- or
// 44 100-point rectangular-window STFT.  A real frame of 48 000 samples is 24 000 packed complex points = 192 KB, more than the
// 160 KB of LDS, so the one-frame-in-LDS radix-2 kernel cannot serve it.
//
// One workgroup per (item, signal) walks the frames of its signal.  Per frame, with N2 = fft_size / 2 = na * nb packed points
// z[nb n1 + n2] and the output index k1 + na k2 (the four-step scheme):
//   1. nb transforms of length na over n1, B columns at a time in LDS (Stockham autosort, radix 4 / 2 / 3 / 5 / 7 stages,
//      ping-pong buffers, element i of column b at i * (B + 1) + b: the lanes of a wave work on consecutive columns);
//   2. times exp(-2 pi i n2 k1 / N2);
//   3. stored transposed, slab[n2 * na + k1], to a workgroup-private slab of N2 float2 in the workspace (L2 / Infinity Cache);
//   4. na transforms of length nb over n2, B rows k1 at a time; Z[k1 + na k2] goes back to slab[k2 * na + k1] -- the very set
//      of addresses the batch was read from, so the slab is transformed in place and ends in natural order.
// Then every thread unpacks the real spectrum of its own bins (the E/O split of ft_mag) and adds |X| to its bins' sums in a
// private row of the workspace: one owner per bin, frames in order, no atomics -- deterministic, and independent of the batch.
// Every twiddle comes from host-built float64 tables (stito_hip.h has the layout).  Bound by the LDS butterfly traffic plus
// one round trip of the slab per frame.
#include "common.h"

namespace stito {

int l2norm_rows(float *x, int n_rows, int n_cols, hipStream_t st);  // features.hip: k_l2norm_rows

enum { MX_MONO = 0, MX_STEREO = 1, MX_MIDSIDE = 2 };
constexpr int MX_MAX_SUB = 512;     // longest sub-transform (na; nb <= na)
constexpr int MX_LDS_PTS = 8192;    // float2 per ping-pong buffer: 2 x 64 KB, below the 128 KB + 64 B of k_stft_feature
constexpr int MX_MAX_B = 32;        // sub-transforms per LDS batch
constexpr int MX_MAX_RAD = 16;

struct MxPlan {
    int na, nb, n_rad_a, n_rad_b;
    int rad[MX_MAX_RAD];  // the radices of na, then those of nb
};

// nb = the largest divisor of N2 not above sqrt(N2); radices: 4s, then a 2, then 3s, 5s, 7s.  0 on success.
static int mx_factor(int n, int *rad, int cap) {
    int c = 0;
    auto put = [&](int r) { if (c < cap) rad[c] = r; ++c; };
    while (n % 4 == 0) { put(4); n /= 4; }
    for (int p : {2, 3, 5, 7})
        while (n % p == 0) { put(p); n /= p; }
    return n == 1 ? c : -1;
}

static int mx_plan(int fft_size, MxPlan &pl) {
    if (fft_size < 128 || fft_size > 96000 || (fft_size & 1)) return -1;
    const int N2 = fft_size / 2;
    int m = N2;
    for (int p : {2, 3, 5, 7})
        while (m % p == 0) m /= p;
    if (m != 1) return -1;
    int nb = 1;
    for (int d = 1; d * d <= N2; ++d)
        if (N2 % d == 0) nb = d;
    pl.na = N2 / nb;
    pl.nb = nb;
    if (pl.na > MX_MAX_SUB) return -1;
    pl.n_rad_a = mx_factor(pl.na, pl.rad, MX_MAX_RAD);
    if (pl.n_rad_a < 0 || pl.n_rad_a > MX_MAX_RAD) return -1;
    pl.n_rad_b = mx_factor(pl.nb, pl.rad + pl.n_rad_a, MX_MAX_RAD - pl.n_rad_a);
    if (pl.n_rad_b < 0 || pl.n_rad_a + pl.n_rad_b > MX_MAX_RAD) return -1;
    return 0;
}

static int mx_batch(int n, int count) {  // sub-transforms of length n per LDS batch: (B + 1) * n <= MX_LDS_PTS
    int b = MX_LDS_PTS / n - 1;
    if (b > MX_MAX_B) b = MX_MAX_B;
    return b < count ? b : count;
}

static size_t mx_ws_per_block(int N2) { return align_up((size_t)N2 * sizeof(float2), 256) + align_up((size_t)(N2 + 1) * sizeof(float), 256); }

__device__ __forceinline__ float2 mx_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 mx_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 mx_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mx_mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // -i a

__device__ __forceinline__ int64_t mx_reflect(int64_t i, int64_t L) {
    if (i < 0) i = -i;
    if (i >= L) i = 2 * (L - 1) - i;
    return i;
}

__device__ __forceinline__ float mx_signal(const float *xl, const float *xr, int64_t i, int mode, int sig) {
    if (mode == MX_MONO) return xr ? (xl[i] + xr[i]) / 2.0f : xl[i];  // torch mean over the channel axis
    if (mode == MX_STEREO) return sig == 0 ? xl[i] : xr[i];
    return sig == 0 ? xl[i] + xr[i] : xl[i] - xr[i];                  // "mid-side" without halving (features.py:201-203)
}

// cos / sin of 2 pi q / P, q < P, for the odd radices (float64 values rounded)
template <int P> struct MxRoots;
template <> struct MxRoots<3> {
    static constexpr float c[3] = {1.0f, -0.5f, -0.5f};
    static constexpr float s[3] = {0.0f, 0.86602540378443865f, -0.86602540378443865f};
};
template <> struct MxRoots<5> {
    static constexpr float c[5] = {1.0f, 0.30901699437494742f, -0.80901699437494742f, -0.80901699437494742f, 0.30901699437494742f};
    static constexpr float s[5] = {0.0f, 0.95105651629515357f, 0.58778525229247313f, -0.58778525229247313f, -0.95105651629515357f};
};
template <> struct MxRoots<7> {
    static constexpr float c[7] = {1.0f, 0.62348980185873353f, -0.22252093395631440f, -0.90096886790241913f,
                                   -0.90096886790241913f, -0.22252093395631440f, 0.62348980185873353f};
    static constexpr float s[7] = {0.0f, 0.78183148246802981f, 0.97492791218182361f, 0.43388373911755812f,
                                   -0.43388373911755812f, -0.97492791218182361f, -0.78183148246802981f};
};

// forward DFT of R points in registers: v[m] <- sum_j v[j] exp(-2 pi i j m / R)
template <int R>
__device__ __forceinline__ void mx_butterfly(float2 *v) {
    if constexpr (R == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = mx_add(a, b);
        v[1] = mx_sub(a, b);
    } else if constexpr (R == 4) {
        const float2 a = mx_add(v[0], v[2]), b = mx_sub(v[0], v[2]), c = mx_add(v[1], v[3]), d = mx_mul_mi(mx_sub(v[1], v[3]));
        v[0] = mx_add(a, c);
        v[1] = mx_add(b, d);
        v[2] = mx_sub(a, c);
        v[3] = mx_sub(b, d);
    } else {
        // odd prime: the terms j and R - j share their cosine and have opposite sines
        constexpr int H = (R - 1) / 2;
        float2 p[H], q[H];
        float2 sum = v[0];
#pragma unroll
        for (int j = 1; j <= H; ++j) {
            p[j - 1] = mx_add(v[j], v[R - j]);
            q[j - 1] = mx_mul_mi(mx_sub(v[j], v[R - j]));
            sum = mx_add(sum, p[j - 1]);
        }
        const float2 x0 = v[0];
        v[0] = sum;
#pragma unroll
        for (int m = 1; m <= H; ++m) {
            float2 a = x0, b = make_float2(0.0f, 0.0f);
#pragma unroll
            for (int j = 1; j <= H; ++j) {
                const float cc = MxRoots<R>::c[(j * m) % R], ss = MxRoots<R>::s[(j * m) % R];
                a.x = fmaf(cc, p[j - 1].x, a.x); a.y = fmaf(cc, p[j - 1].y, a.y);
                b.x = fmaf(ss, q[j - 1].x, b.x); b.y = fmaf(ss, q[j - 1].y, b.y);
            }
            v[m] = mx_add(a, b);
            v[R - m] = mx_sub(a, b);
        }
    }
}

// One Stockham stage of radix R over B interleaved transforms of length n (element i of transform b at [i * ld + b]); ns = the
// product of the radices already done; root[m] = exp(-2 pi i m / n).
template <int NT, int R>
__device__ __forceinline__ void mx_stage(const float2 *x, float2 *y, const float2 *__restrict__ root, int n, int ns, int B, int ld, int tid) {
    const int m = n / R, tstep = m / ns;
    for (int w = tid; w < m * B; w += NT) {
        const int j = w / B, b = w - j * B;
        const int k = j % ns;
        float2 v[R];
#pragma unroll
        for (int t = 0; t < R; ++t) v[t] = x[(j + t * m) * ld + b];
        if (ns > 1) {
#pragma unroll
            for (int t = 1; t < R; ++t) v[t] = mx_cmul(v[t], root[t * k * tstep]);  // t k tstep < n
        }
        mx_butterfly<R>(v);
        const int j0 = (j - k) * R + k;
#pragma unroll
        for (int t = 0; t < R; ++t) y[(j0 + t * ns) * ld + b] = v[t];
    }
}

// B transforms of length n from buffer a (a and b ping-pong); returns the buffer that holds the result, natural order.
// Ends with a barrier.
template <int NT>
__device__ float2 *mx_fft(float2 *a, float2 *b, const float2 *__restrict__ root, int n, const int *rad, int n_rad, int B, int ld, int tid) {
    int ns = 1;
    for (int s = 0; s < n_rad; ++s) {
        const int R = rad[s];
        switch (R) {
        case 2: mx_stage<NT, 2>(a, b, root, n, ns, B, ld, tid); break;
        case 3: mx_stage<NT, 3>(a, b, root, n, ns, B, ld, tid); break;
        case 4: mx_stage<NT, 4>(a, b, root, n, ns, B, ld, tid); break;
        case 5: mx_stage<NT, 5>(a, b, root, n, ns, B, ld, tid); break;
        default: mx_stage<NT, 7>(a, b, root, n, ns, B, ld, tid); break;
        }
        __syncthreads();
        float2 *t = a; a = b; b = t;
        ns *= R;
    }
    return a;
}

// |X[k]| of the 2 N2 real samples whose packed transform is Z (natural order), k in [0, N2]: the E/O split of ft_mag
__device__ __forceinline__ float mx_mag(const float2 *Z, const float2 *__restrict__ tw, int k, int N2) {
    const float2 zk = Z[k == N2 ? 0 : k], zn = Z[(k == 0 || k == N2) ? 0 : N2 - k];
    const float2 E = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
    const float2 O = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
    const float2 w = k < N2 ? tw[k] : make_float2(-1.0f, 0.0f);
    const float2 wo = mx_cmul(w, O);
    const float re = E.x + wo.x, im = E.y + wo.y;
    return sqrtf(re * re + im * im);
}

template <int NT>
__global__ __launch_bounds__(NT) void k_bark_mixed(const float *__restrict__ audio, int C, int64_t L, int mode, int n_sig, MxPlan pl,
                                                    int Ba, int Bb, int hop, int64_t T, const float2 *__restrict__ tables,
                                                    const float *__restrict__ fb, int n_bands, char *ws, size_t ws_per_block,
                                                    float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float2 mx_lds[];
    float2 *buf0 = mx_lds, *buf1 = mx_lds + MX_LDS_PTS;
    const int na = pl.na, nb = pl.nb, N2 = na * nb;
    const int item = blockIdx.x / n_sig, sig = blockIdx.x % n_sig, tid = threadIdx.x;
    const float *xl = audio + (int64_t)item * C * L;
    const float *xr = C == 2 ? xl + L : nullptr;
    const float2 *root_a = tables, *root_b = tables + na, *four = tables + na + nb, *unpack = tables + na + nb + N2;
    float2 *slab = (float2 *)(ws + (size_t)blockIdx.x * ws_per_block);
    float *sum = (float *)(ws + (size_t)blockIdx.x * ws_per_block + (((size_t)N2 * sizeof(float2) + 255) & ~(size_t)255));

    for (int64_t t = 0; t < T; ++t) {
        const int64_t base = t * hop - N2;  // center=True: frame t covers [t hop - fft_size/2, t hop + fft_size/2)
        // steps 1 - 3: columns n2 = c0 .. c0 + B - 1
        for (int c0 = 0; c0 < nb; c0 += Ba) {
            const int B = min(Ba, nb - c0), ld = Ba + 1;
            for (int w = tid; w < na * B; w += NT) {
                const int n1 = w / B, b = w - n1 * B;
                const int64_t s0 = base + 2 * (int64_t)(nb * n1 + c0 + b);
                const int64_t i0 = mx_reflect(s0, L), i1 = mx_reflect(s0 + 1, L);
                buf0[n1 * ld + b] = make_float2(mx_signal(xl, xr, i0, mode, sig), mx_signal(xl, xr, i1, mode, sig));
            }
            __syncthreads();
            const float2 *r = mx_fft<NT>(buf0, buf1, root_a, na, pl.rad, pl.n_rad_a, B, ld, tid);
            for (int w = tid; w < na * B; w += NT) {  // k1 fastest: the batch is one contiguous run of the slab
                const int b = w / na, k1 = w - b * na;
                const int o = (c0 + b) * na + k1;
                slab[o] = mx_cmul(r[k1 * ld + b], four[o]);
            }
            __syncthreads();
        }
        // step 4: rows k1 = r0 .. r0 + B - 1, in place in the slab
        for (int r0 = 0; r0 < na; r0 += Bb) {
            const int B = min(Bb, na - r0), ld = Bb + 1;
            for (int w = tid; w < nb * B; w += NT) {
                const int n2 = w / B, b = w - n2 * B;
                buf0[n2 * ld + b] = slab[n2 * na + r0 + b];
            }
            __syncthreads();
            const float2 *r = mx_fft<NT>(buf0, buf1, root_b, nb, pl.rad + pl.n_rad_a, pl.n_rad_b, B, ld, tid);
            for (int w = tid; w < nb * B; w += NT) {
                const int k2 = w / B, b = w - k2 * B;
                slab[k2 * na + r0 + b] = r[k2 * ld + b];  // Z[k1 + na k2]
            }
            __syncthreads();
        }
        // a thread owns its bins for the whole signal: sums in frame order
        for (int k = tid; k <= N2; k += NT) {
            const float mg = mx_mag(slab, unpack, k, N2);
            sum[k] = t == 0 ? mg : sum[k] + mg;
        }
        __syncthreads();  // the slab is rewritten by the next frame
    }
    // mean over frames, then one filterbank row per wave at a time
    const float inv_t = 1.0f / (float)T;
    const int wv = tid >> 6, lane = tid & 63, nfreq = N2 + 1;
    for (int b = wv; b < n_bands; b += NT / 64) {
        const float *row = fb + (int64_t)b * nfreq;
        float s = 0.0f;
        for (int k = lane; k < nfreq; k += 64) s = fmaf(row[k], sum[k] * inv_t, s);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        // band-major, like k_stft_feature MODE 0
        if (lane == 0) out[((int64_t)item * n_bands + b) * n_sig + sig] = logf(s + 1e-8f);
    }
}

}  // namespace stito

using namespace stito;

extern "C" int stito_fft_mixed_plan(int fft_size, int *na, int *nb, int *radices, int max_radices) {
    STITO_REQUIRE(na != nullptr && nb != nullptr && radices != nullptr && max_radices > 0, STITO_E_INVALID, "stito_fft_mixed_plan: null argument");
    MxPlan pl;
    STITO_REQUIRE(mx_plan(fft_size, pl) == 0, STITO_E_UNSUPPORTED,
                  "mixed-radix bark spectrum: fft_size %d must be even, in [128, 96000], with no prime factor above 7", fft_size);
    const int n = pl.n_rad_a + pl.n_rad_b;
    STITO_REQUIRE(n <= max_radices, STITO_E_INVALID, "stito_fft_mixed_plan: %d radices do not fit max_radices %d", n, max_radices);
    *na = pl.na;
    *nb = pl.nb;
    for (int i = 0; i < n; ++i) radices[i] = pl.rad[i];
    return n;
}

extern "C" int64_t stito_barkspectrum_mixed_workspace_bytes(int n_items, int n_sig, int fft_size) {
    MxPlan pl;
    if (n_items <= 0 || n_sig <= 0 || mx_plan(fft_size, pl) != 0) return 0;
    return (int64_t)((size_t)n_items * n_sig * mx_ws_per_block(fft_size / 2));
}

extern "C" int stito_barkspectrum_mixed(const float *audio_dev, int n_items, int channels, int64_t n_samples, int mode, int fft_size,
                                        const void *tables_dev, int64_t tables_len, const float *fb_dev, int n_bands, float *out_dev,
                                        void *ws_dev, int64_t ws_bytes, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    MxPlan pl;
    STITO_REQUIRE(mx_plan(fft_size, pl) == 0, STITO_E_UNSUPPORTED,
                  "mixed-radix bark spectrum: fft_size %d must be even, in [128, 96000], with no prime factor above 7", fft_size);
    STITO_REQUIRE(n_items > 0 && n_bands > 0, STITO_E_INVALID, "stito_barkspectrum_mixed: empty input");
    STITO_REQUIRE(mode >= 0 && mode <= 2, STITO_E_INVALID, "Invalid mode %d", mode);
    STITO_REQUIRE(channels == 2 || (channels == 1 && mode == MX_MONO), STITO_E_INVALID, "mode %d needs a stereo input", mode);
    STITO_REQUIRE(n_samples > fft_size / 2, STITO_E_INVALID, "reflect padding needs n_samples > fft_size/2");
    const int N2 = fft_size / 2, n_sig = mode == MX_MONO ? 1 : 2, hop = fft_size / 4;
    STITO_REQUIRE(tables_dev != nullptr && tables_len == (int64_t)pl.na + pl.nb + 2 * (int64_t)N2, STITO_E_INVALID,
                  "stito_barkspectrum_mixed: tables_len %lld, fft_size %d needs %lld", (long long)tables_len, fft_size,
                  (long long)pl.na + pl.nb + 2 * (long long)N2);
    const size_t per_block = mx_ws_per_block(N2);
    STITO_REQUIRE(ws_dev != nullptr && ws_bytes >= (int64_t)((size_t)n_items * n_sig * per_block), STITO_E_WORKSPACE,
                  "stito_barkspectrum_mixed: workspace too small");
    STITO_REQUIRE(((uintptr_t)ws_dev & 7) == 0, STITO_E_INVALID, "stito_barkspectrum_mixed: workspace not 8-byte aligned");
    const int64_t T = n_samples / hop + 1;
    const int Ba = mx_batch(pl.na, pl.nb), Bb = mx_batch(pl.nb, pl.na);
    const size_t lds = (size_t)2 * MX_LDS_PTS * sizeof(float2);
    if (N2 >= 2048) {
        STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_bark_mixed<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_bark_mixed<1024>), dim3(n_items * n_sig), dim3(1024), lds, st, audio_dev, channels, n_samples, mode, n_sig, pl,
                           Ba, Bb, hop, T, (const float2 *)tables_dev, fb_dev, n_bands, (char *)ws_dev, per_block, out_dev);
    } else {
        STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_bark_mixed<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_bark_mixed<256>), dim3(n_items * n_sig), dim3(256), lds, st, audio_dev, channels, n_samples, mode, n_sig, pl,
                           Ba, Bb, hop, T, (const float2 *)tables_dev, fb_dev, n_bands, (char *)ws_dev, per_block, out_dev);
    }
    STITO_LAUNCH_CHECK();
    return l2norm_rows(out_dev, n_items, n_sig * n_bands, st);
}
