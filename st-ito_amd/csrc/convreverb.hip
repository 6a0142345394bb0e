// convreverb.hip -- noise-shaped convolution reverb (BASELINE.json configs[4]).
//
// Replaces (reference file:line): apply_reverb st_ito/effects.py:558-620, which forwards 12 band
// gains, 12 band decays and a mix to dasp_pytorch.noise_shaped_reverberation (un-vendored, un-pinned
// dependency, setup.py:51 -- restated from its published algorithm, PARITY UNPINNED):
//     IR[c][t] = mean_b( noise_b[c][t] * exp(-(10 decay_b + 1) t/(N-1)) * gain_b ),  b = 0..11
//     wet      = causal convolution of x with IR (x left-padded by N-1, output length = len(x))
//     y        = (1 - mix) x + mix wet
// The library draws fresh unseeded white noise per call and band-passes it with a 12-band octave
// FIR bank; that part is setup, not arithmetic of the path: the caller supplies the band-filtered
// noise bank (2, 12, N) once (st_ito.effects.NoiseShapedReverb builds a seeded one), exactly like
// it supplies packed weights.  Mono input is duplicated to stereo by the chain's channel rule.
//
// Every candidate has its own IR (N = 65 536 by default, 96 000 in configs[4]), so the convolution
// is a uniformly partitioned overlap-save FFT convolution, entirely on the GPU:
//   k_cr_ir_fft   one workgroup per (stream, IR partition k): synthesise the partition from the
//                 noise bank (12 expf per tap), zero-pad to 2B, real FFT in LDS -> H[s][k]
//   k_cr_in_fft   one workgroup per (input stream, block j): x[(j-1)B, (j+1)B) -> X[s][j]
//                 (an input shared by the population is transformed once, not per candidate)
//   k_cr_mac_ifft one workgroup per (stream, block j): Y = sum_k X[j-k] .* H[k] in registers
//                 (8 bins per thread), inverse real FFT in LDS, keep the last B samples, mix, store.
// B = 4096: a 2B-point real FFT is a 4096-point complex radix-2 Stockham FFT, 2 x 32 KB of LDS.
// Spectra are stored as B complex bins with the (real) Nyquist bin packed into the imaginary part
// of bin 0.  Bound: the spectral multiply-accumulate streams K spectra of X and H per output block;
// H[s] (K x 32 KB) and the sliding X window are L2-resident across the J blocks of a stream, so the
// algorithmic HBM traffic is one read of x, one write of y and one pass over H per stream.
#include "dsp_view.h"

namespace stito {

static constexpr int CR_B = 4096;
static constexpr int CR_LOG2B = 12;
static constexpr int CR_THREADS = 512;
static constexpr int CR_BPT = CR_B / CR_THREADS;  // bins per thread in the MAC kernel

__device__ __forceinline__ float2 cr_cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// tw[k] = exp(-2 pi i k / (2B)), k < B  (float64 sincospi, rounded once)
__global__ void k_cr_twiddle(float2 *__restrict__ tw) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= CR_B) return;
    double s, c;
    sincospi(-(double)k / (double)CR_B, &s, &c);
    tw[k] = make_float2((float)c, (float)s);
}

// In-LDS radix-2 Stockham autosort FFT of B complex points; returns the buffer holding the result.
// INV: e^{+...} twiddles (unnormalised inverse).
template <bool INV>
__device__ float2 *cr_fft(float2 *src, float2 *dst, const float2 *__restrict__ tw, int tid) {
    constexpr int half = CR_B >> 1;
    for (int p = 1, sh = CR_LOG2B; p < CR_B; p <<= 1, --sh) {
        // stage twiddle exp(-+ i pi k / p) = tw[k * B / p] = tw[k << sh], sh = log2(B) - log2(p)
        for (int i = tid; i < half; i += CR_THREADS) {
            const int k = i & (p - 1);
            const int j = ((i - k) << 1) + k;
            float2 w = tw[k << sh];
            if (INV) w.y = -w.y;
            const float2 u0 = src[i];
            const float2 u1 = cr_cmul(src[i + half], w);
            dst[j] = make_float2(u0.x + u1.x, u0.y + u1.y);
            dst[j + p] = make_float2(u0.x - u1.x, u0.y - u1.y);
        }
        __syncthreads();
        float2 *t = src; src = dst; dst = t;
    }
    return src;
}

// Z = FFT_B(even + i odd) -> one-sided spectrum of the 2B real samples, bins 0..B-1 (+ Nyquist in out[0].y)
__device__ void cr_unpack_store(const float2 *Z, const float2 *__restrict__ tw, float2 *__restrict__ out, int tid) {
    for (int k = tid; k < CR_B; k += CR_THREADS) {
        const float2 zk = Z[k], zn = Z[(CR_B - k) & (CR_B - 1)];
        const float2 E = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
        const float2 O = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));  // (zk - conj(zn)) / (2i)
        if (k == 0) {
            out[0] = make_float2(E.x + O.x, E.x - O.x);  // X[0] = E0 + O0, X[B] = E0 - O0 (both real)
        } else {
            const float2 wo = cr_cmul(tw[k], O);
            out[k] = make_float2(E.x + wo.x, E.y + wo.y);
        }
    }
}

// torch.linspace(0, 1, N)[t] in float32 (symmetric evaluation about the midpoint)
__device__ __forceinline__ float cr_linspace01(int64_t t, int64_t N) {
    const float step = 1.0f / (float)(N - 1);
    return t < N / 2 ? (float)t * step : 1.0f - (float)(N - 1 - t) * step;
}

__global__ __launch_bounds__(CR_THREADS) void k_cr_ir_fft(const float *__restrict__ noise, int64_t N, int K,
                                                          const double *__restrict__ coef, const float2 *__restrict__ tw,
                                                          float2 *__restrict__ H) {
    extern __shared__ __attribute__((aligned(16))) float2 cr_lds[];
    float2 *bufA = cr_lds, *bufB = cr_lds + CR_B;
    const int k = blockIdx.x, s = blockIdx.y, cand = s >> 1, c = s & 1, tid = threadIdx.x;
    const double *cf = coef + (int64_t)cand * COEF_STRIDE;
    float g[12], d[12];
#pragma unroll
    for (int b = 0; b < 12; ++b) { g[b] = (float)cf[b]; d[b] = (float)cf[12 + b]; }
    const float *nz = noise + (int64_t)c * 12 * N;
    // partition k = taps [kB, (k+1)B), zero-padded to 2B; packed (even, odd) -> only m < B/2 is non-zero
    for (int m = tid; m < CR_B; m += CR_THREADS) {
        float v[2] = {0.f, 0.f};
        if (m < CR_B / 2) {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int64_t t = (int64_t)k * CR_B + 2 * m + e;
                if (t < N) {
                    const float tt = cr_linspace01(t, N);
                    float acc = 0.0f;
#pragma unroll
                    for (int b = 0; b < 12; ++b) acc += nz[(int64_t)b * N + t] * (expf(-d[b] * tt) * g[b]);
                    v[e] = acc / 12.0f;
                }
            }
        }
        bufA[m] = make_float2(v[0], v[1]);
    }
    __syncthreads();
    const float2 *Z = cr_fft<false>(bufA, bufB, tw, tid);
    cr_unpack_store(Z, tw, H + ((int64_t)s * K + k) * CR_B, tid);
}

__global__ __launch_bounds__(CR_THREADS) void k_cr_in_fft(InView in, int C, int64_t L, int J, int shared_group,
                                                          const float2 *__restrict__ tw, float2 *__restrict__ X) {
    extern __shared__ __attribute__((aligned(16))) float2 cr_lds[];
    float2 *bufA = cr_lds, *bufB = cr_lds + CR_B;
    const int j = blockIdx.x, xs = blockIdx.y, tid = threadIdx.x;
    // xs indexes the distinct input streams: (input, channel) when the input is shared, else (cand, channel)
    const int unit = xs / C, ch = xs % C;
    const float *x = in_ptr(in, shared_group ? unit * shared_group : unit, ch);
    const int64_t base = ((int64_t)j - 1) * CR_B;
    for (int m = tid; m < CR_B; m += CR_THREADS) {
        const int64_t i0 = base + 2 * m, i1 = i0 + 1;
        bufA[m] = make_float2((i0 >= 0 && i0 < L) ? x[i0] : 0.0f, (i1 >= 0 && i1 < L) ? x[i1] : 0.0f);
    }
    __syncthreads();
    const float2 *Z = cr_fft<false>(bufA, bufB, tw, tid);
    cr_unpack_store(Z, tw, X + ((int64_t)xs * J + j) * CR_B, tid);
}

__global__ __launch_bounds__(CR_THREADS) void k_cr_mac_ifft(InView in, float *__restrict__ out, int64_t cand_stride,
                                                            int64_t L, int J, int K, int shared_group,
                                                            const double *__restrict__ coef, const float2 *__restrict__ tw,
                                                            const float2 *__restrict__ X, const float2 *__restrict__ H) {
    extern __shared__ __attribute__((aligned(16))) float2 cr_lds[];
    float2 *bufA = cr_lds, *bufB = cr_lds + CR_B;
    const int j = blockIdx.x, s = blockIdx.y, cand = s >> 1, c = s & 1, tid = threadIdx.x;
    const int xs = (shared_group ? cand / shared_group : cand) * 2 + c;
    const float2 *Xs = X + (int64_t)xs * J * CR_B;
    const float2 *Hs = H + (int64_t)s * K * CR_B;
    float2 acc[CR_BPT];
#pragma unroll
    for (int u = 0; u < CR_BPT; ++u) acc[u] = make_float2(0.f, 0.f);
    const int kmax = j < K - 1 ? j : K - 1;
    for (int k = 0; k <= kmax; ++k) {
        const float2 *xp = Xs + (int64_t)(j - k) * CR_B, *hp = Hs + (int64_t)k * CR_B;
#pragma unroll
        for (int u = 0; u < CR_BPT; ++u) {
            const int bin = tid + u * CR_THREADS;
            const float2 a = xp[bin], b = hp[bin];
            if (bin == 0) {  // packed DC / Nyquist: two real products
                acc[u].x = fmaf(a.x, b.x, acc[u].x);
                acc[u].y = fmaf(a.y, b.y, acc[u].y);
            } else {
                acc[u].x += a.x * b.x - a.y * b.y;
                acc[u].y += a.x * b.y + a.y * b.x;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < CR_BPT; ++u) bufA[tid + u * CR_THREADS] = acc[u];
    __syncthreads();
    // pack for the inverse: E[k] = (Y[k] + conj(Y[B-k]))/2, O[k] = conj(w^k) (Y[k] - conj(Y[B-k]))/2, Z = E + i O
    for (int k = tid; k < CR_B; k += CR_THREADS) {
        float2 Z;
        if (k == 0) {
            const float y0 = bufA[0].x, yB = bufA[0].y;
            Z = make_float2(0.5f * (y0 + yB), 0.5f * (y0 - yB));  // E0 = (Y0+YB)/2, O0 = (Y0-YB)/2, both real
        } else {
            const float2 yk = bufA[k], yn = bufA[CR_B - k];
            const float2 E = make_float2(0.5f * (yk.x + yn.x), 0.5f * (yk.y - yn.y));
            const float2 D = make_float2(0.5f * (yk.x - yn.x), 0.5f * (yk.y + yn.y));
            float2 w = tw[k];
            w.y = -w.y;
            const float2 O = cr_cmul(w, D);
            Z = make_float2(E.x - O.y, E.y + O.x);
        }
        bufB[k] = Z;
    }
    __syncthreads();
    const float2 *z = cr_fft<true>(bufB, bufA, tw, tid);
    // samples n in [B, 2B) of the 2B-point block = z[m], m in [B/2, B): (re, im) = (x[2m], x[2m+1])
    const float mix = (float)coef[(int64_t)cand * COEF_STRIDE + 24];
    const float scale = 1.0f / (float)CR_B;
    const float *xd = in_ptr(in, cand, c);
    float *o = out + (int64_t)cand * cand_stride + (int64_t)c * L;
    for (int m = tid; m < CR_B / 2; m += CR_THREADS) {
        const float2 v = z[CR_B / 2 + m];
        const int64_t n0 = (int64_t)j * CR_B + 2 * m;
        if (n0 < L) o[n0] = (1.0f - mix) * xd[n0] + mix * (v.x * scale);
        if (n0 + 1 < L) o[n0 + 1] = (1.0f - mix) * xd[n0 + 1] + mix * (v.y * scale);
    }
}

static inline int cr_blocks(int64_t n) { return (int)((n + CR_B - 1) / CR_B); }

static constexpr size_t CR_SPEC = (size_t)CR_B * sizeof(float2);   // bytes of one spectrum
struct ConvReverbLayout : WsLayout { size_t tw, X, H; };   // twiddles | spectra of the input blocks | of the IR partitions
static ConvReverbLayout conv_reverb_layout(int n_streams, int64_t n_samples, int64_t n_taps) {
    ConvReverbLayout l;
    l.tw = l.add(CR_SPEC);
    l.X = l.add((size_t)n_streams * cr_blocks(n_samples) * CR_SPEC);
    l.H = l.add((size_t)n_streams * cr_blocks(n_taps) * CR_SPEC);
    return l;
}
size_t conv_reverb_workspace_bytes(int n_streams, int64_t n_samples, int64_t n_taps) { return conv_reverb_layout(n_streams, n_samples, n_taps).total; }

int conv_reverb_stage(const InView &in, float *audio_dev, int64_t cand_stride, int pop, int64_t n_samples,
                      const double *coef, const float *noise_bank, int64_t n_taps, void *workspace, hipStream_t st) {
    STITO_REQUIRE(noise_bank != nullptr && n_taps >= 2, STITO_E_INVALID,
                  "NoiseShapedReverb needs its noise bank (aux_dev, (2, 12, n_taps) float32) and n_taps >= 2");
    const int S = pop * 2, J = cr_blocks(n_samples), K = cr_blocks(n_taps);
    const ConvReverbLayout l = conv_reverb_layout(S, n_samples, n_taps);
    char *ws = (char *)workspace;
    float2 *tw = (float2 *)(ws + l.tw), *X = (float2 *)(ws + l.X), *H = (float2 *)(ws + l.H);
    // an input shared by groups of candidates (first effect of the chain) is transformed once per group
    const bool shared = in.cand_stride == 0;
    const int group = shared ? (in.group < pop ? in.group : pop) : 0;
    const int n_in_streams = shared ? (pop / group) * 2 : S;
    const size_t lds = 2 * CR_SPEC;
    STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_cr_ir_fft, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_cr_in_fft, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    STITO_HIP_CHECK(hipFuncSetAttribute((const void *)k_cr_mac_ifft, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_cr_twiddle, dim3(CR_B / 256), dim3(256), 0, st, tw);
    STITO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cr_ir_fft, dim3(K, S), dim3(CR_THREADS), lds, st, noise_bank, n_taps, K, coef, tw, H);
    STITO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cr_in_fft, dim3(J, n_in_streams), dim3(CR_THREADS), lds, st, in, 2, n_samples, J, group, tw, X);
    STITO_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cr_mac_ifft, dim3(J, S), dim3(CR_THREADS), lds, st, in, audio_dev, cand_stride, n_samples, J, K, group,
                       coef, tw, X, H);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

}  // namespace stito
