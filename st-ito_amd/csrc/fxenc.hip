// fxenc.hip -- the FX-Encoder (Koo et al., "Music Mixing Style Transfer") on gfx950: a stack of one-dimensional convolutions
// with reflection padding, folded eval-mode batch norm, ReLU and an optional residual, then the mean over positions (ABI 10.11).
//
// One layer is  y[b][co][p] = relu(scale[co] * sum_{ci, t} w[co][ci][t] * x[b][ci][reflect(p * stride + t - l_pad)] + shift[co]) (+ x[b][co][p])
// on (B, C, L) float32 maps as torch lays them out.  Two kernels:
//
//   k_conv_mfma   the implicit GEMM on the matrix pipe with exact f32 products (v_mfma_f32_32x32x2_f32).  M = cout, N = the
//                 flattened (item, output position) index -- so a weight tile is read once per population, not once per item --
//                 and the reduction runs over r = ci * K + t in ascending order.  A workgroup of four waves owns a BM x BN tile
//                 of the output; per step of BK = 16 reduction indices it stages a BK x BM slab of the packed weights and a
//                 BK x BN slab of gathered inputs in LDS (k-major: the 32 lanes of a half-wave read 32 consecutive floats of one
//                 k row, one bank each), double buffered, the next step's global loads in flight under this step's products.
//                 The loader forms the reflected source index per (item, position, tap): column j of the tile is position
//                 n % Lout of item n / Lout, so a tile that straddles two items reflects inside each and never reads across.
//                 Products of SEG reduction indices go into a fresh accumulator that is then added to the running sum: the
//                 rounding error grows with SEG + R / SEG instead of R = cin * K (up to 10 240 here).  Nothing in this order
//                 depends on the batch: an item has the same bits alone and at any place of any batch.
//   k_conv_valu   cin <= 2 (block 0: the 2 -> 2 layer at full length and 2 -> 16 at stride 4; no GEMM worth the pipe).  A
//                 workgroup stages its reflected input span in LDS; a thread owns RUN consecutive outputs, holds their
//                 (RUN - 1) * S + K inputs per channel in registers and slides over the taps for one output channel after the other.
//
// The mean over positions is one wave per (item, channel) row: lanes stride over the row, then a fixed butterfly.  No atomics.
#include "common.h"

namespace stito {
namespace fxenc {

constexpr int BK = 16;          // reduction indices per LDS slab
constexpr int SEG_STEPS = 16;   // slabs per accumulator segment (256 reduction indices)
constexpr int THREADS = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the M tile of the implicit GEMM for a layer, 0 for the VALU kernel (plain (cout, cin, K) weights).  The one launch rule: the
// packing, the size query and the launch all ask it.
constexpr int VALU_RUN = 4;
static inline bool valu_shape(int K, int S) { return (K == 25 || K == 15 || K == 10 || K == 5) && (S == 1 || S == 2 || S == 4); }
static inline int tile_m(int cout, int cin, int K, int S) {
    if (cin <= 2 && valu_shape(K, S)) return 0;
    return cout <= 32 ? 32 : cout <= 64 ? 64 : 128;
}
static inline int64_t out_len(int64_t L, int S) { return (L + S - 1) / S; }
static inline size_t packed_floats(int cout, int cin, int K, int S) {
    const int bm = tile_m(cout, cin, K, S);
    if (bm == 0) return (size_t)cout * cin * K;
    const size_t R = (size_t)cin * K, Rpad = (R + BK - 1) / BK * BK;
    return (size_t)((cout + bm - 1) / bm) * Rpad * bm;
}

__device__ __forceinline__ int reflect(int s, int L) {   // one fold each side suffices: L > r_pad >= l_pad
    s = s < 0 ? -s : s;
    return s >= L ? 2 * (L - 1) - s : s;
}

// wp: [m tile][r < Rpad][BM] (zero padded in r and m).  grid (N tiles, M tiles).
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(THREADS) void k_conv_mfma(const float *__restrict__ x, const float *__restrict__ wp,
                                                       const float *__restrict__ scale, const float *__restrict__ shift,
                                                       float *__restrict__ y, int B, int Cin, int Cout, int K, int S, int L, int Lout,
                                                       int residual) {
    static_assert(WM * WN == 4, "four waves");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int A_F4 = BK * BM / 4 / THREADS > 0 ? BK * BM / 4 / THREADS : 1;   // float4 loads of the weight slab per thread
    constexpr bool A_PART = BK * BM / 4 < THREADS;                                 // fewer float4 than threads (BM = 32)
    constexpr int B_STEP = THREADS / BN;                                           // k rows between a thread's elements
    constexpr int B_PER = BK / B_STEP;                                             // gathered inputs per thread and slab
    static_assert(B_STEP >= 1 && B_PER * B_STEP == BK, "slab shape");
    __shared__ __attribute__((aligned(16))) float As[2][BK * BM];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK * BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int R = Cin * K, n_steps = (R + BK - 1) / BK, Rpad = n_steps * BK;
    const int N = B * Lout;
    const int n0 = blockIdx.x * BN, mt = blockIdx.y;
    const int l_pad = (K - 1) / 2;

    // this thread's column of the input slab: one (item, position) for the whole launch
    const int j = tid % BN, n = n0 + j;
    const bool col_ok = n < N;
    const int b = col_ok ? n / Lout : 0, p = col_ok ? n - b * Lout : 0;
    const float *xb = x + (size_t)b * Cin * L;
    const int s_base = p * S - l_pad;
    int ci = 0, tap = tid / BN;   // (ci, tap) of this thread's next element; advances by B_STEP per element, for ever
    while (tap >= K) { tap -= K; ++ci; }

    const float *wa = wp + (size_t)mt * Rpad * BM;
    static_assert(A_F4 <= 2, "weight slab");
    float4 a_reg0 = {0.f, 0.f, 0.f, 0.f}, a_reg1 = {0.f, 0.f, 0.f, 0.f};
    float b_reg[B_PER];
    auto load_slab = [&](int step) __attribute__((always_inline)) {
        const float *ws = wa + (size_t)step * BK * BM + 4 * tid;
        if (!A_PART || tid < BK * BM / 4) a_reg0 = *reinterpret_cast<const float4 *>(ws);
        if constexpr (A_F4 == 2) a_reg1 = *reinterpret_cast<const float4 *>(ws + 4 * THREADS);
#pragma unroll
        for (int i = 0; i < B_PER; ++i) {
            b_reg[i] = (col_ok && ci < Cin) ? xb[(size_t)ci * L + reflect(s_base + tap, L)] : 0.f;
            tap += B_STEP;
            while (tap >= K) { tap -= K; ++ci; }
        }
    };
    auto store_slab = [&](int buf) __attribute__((always_inline)) {
        if (!A_PART || tid < BK * BM / 4) *reinterpret_cast<float4 *>(&As[buf][4 * tid]) = a_reg0;
        if constexpr (A_F4 == 2) *reinterpret_cast<float4 *>(&As[buf][4 * (tid + THREADS)]) = a_reg1;
#pragma unroll
        for (int i = 0; i < B_PER; ++i) Bs[buf][(tid / BN + i * B_STEP) * BN + j] = b_reg[i];
    };

    f32x16 acc[TM][TN], sum[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int c = 0; c < TN; ++c)
#pragma unroll
            for (int v = 0; v < 16; ++v) { acc[a][c][v] = 0.f; sum[a][c][v] = 0.f; }

    load_slab(0);
    store_slab(0);
    __syncthreads();
    const int a_off = wm * TM * 32 + (lane & 31), b_off = wn * TN * 32 + (lane & 31), kh = lane >> 5;
    for (int step = 0; step < n_steps; ++step) {
        const int buf = step & 1;
        if (step + 1 < n_steps) load_slab(step + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const int k = 2 * kk + kh;
            float av[TM], bv[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) av[a] = As[buf][k * BM + a_off + a * 32];
#pragma unroll
            for (int c = 0; c < TN; ++c) bv[c] = Bs[buf][k * BN + b_off + c * 32];
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int c = 0; c < TN; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[c], acc[a][c], 0, 0, 0);
        }
        if ((step + 1) % SEG_STEPS == 0 || step + 1 == n_steps) {
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int c = 0; c < TN; ++c)
#pragma unroll
                    for (int v = 0; v < 16; ++v) { sum[a][c][v] += acc[a][c][v]; acc[a][c][v] = 0.f; }
        }
        if (step + 1 < n_steps) store_slab(buf ^ 1);
        __syncthreads();
    }

    // epilogue: register v of a 32 x 32 tile is row (v & 3) + 8 (v >> 2) + 4 (lane >> 5), column lane & 31: per register a
    // half-wave writes 32 consecutive positions of one output row
#pragma unroll
    for (int c = 0; c < TN; ++c) {
        const int ne = n0 + wn * TN * 32 + c * 32 + (lane & 31);
        if (ne >= N) continue;
        const int be = ne / Lout, pe = ne - be * Lout;
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int m = mt * BM + wm * TM * 32 + a * 32 + (v & 3) + 8 * (v >> 2) + 4 * kh;
                if (m >= Cout) continue;
                float o = fmaxf(fmaf(sum[a][c][v], scale[m], shift[m]), 0.f);
                if (residual) o += x[((size_t)be * Cin + m) * L + pe];   // cin == cout, stride 1: the same row of the input
                y[((size_t)be * Cout + m) * Lout + pe] = o;
            }
    }
}

// cin <= 2.  grid (position tiles of THREADS * RUN outputs, B); w plain (cout, cin, K).
template <int K, int S>
__global__ __launch_bounds__(THREADS) void k_conv_valu(const float *__restrict__ x, const float *__restrict__ w,
                                                       const float *__restrict__ scale, const float *__restrict__ shift,
                                                       float *__restrict__ y, int Cin, int Cout, int L, int Lout, int residual) {
    constexpr int RUN = VALU_RUN, TP = THREADS * RUN, SPAN = (TP - 1) * S + K, WIN = (RUN - 1) * S + K;
    __shared__ float xs[2][SPAN];
    const int tid = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * TP;
    const int l_pad = (K - 1) / 2;
    const float *xb = x + (size_t)b * Cin * L;
    const int s0 = p0 * S - l_pad;
    // positions past the row's end feed outputs that are never stored: clamp their source inside the row
    for (int ci = 0; ci < Cin; ++ci)
        for (int i = tid; i < SPAN; i += THREADS) {
            int s = s0 + i;
            s = s < 0 ? -s : s;
            s = s >= L ? 2 * (L - 1) - s : s;
            s = s < 0 ? 0 : s;
            xs[ci][i] = xb[(size_t)ci * L + s];
        }
    __syncthreads();
    const int q0 = tid * RUN;   // first output of this thread inside the tile
    float win[2][WIN];
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
        for (int i = 0; i < WIN; ++i) win[ci][i] = ci < Cin ? xs[ci][q0 * S + i] : 0.f;
    for (int co = 0; co < Cout; ++co) {
        float acc[RUN];
#pragma unroll
        for (int r = 0; r < RUN; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            if (ci < Cin) {
                const float *wr = w + ((size_t)co * Cin + ci) * K;
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    const float wt = wr[t];
#pragma unroll
                    for (int r = 0; r < RUN; ++r) acc[r] = fmaf(wt, win[ci][r * S + t], acc[r]);
                }
            }
        }
        const float sc = scale[co], sh = shift[co];
#pragma unroll
        for (int r = 0; r < RUN; ++r) {
            const int p = p0 + q0 + r;
            if (p < Lout) {
                float o = fmaxf(fmaf(acc[r], sc, sh), 0.f);
                if (residual) o += xb[(size_t)co * L + p];
                y[((size_t)b * Cout + co) * Lout + p] = o;
            }
        }
    }
}

// one wave per row of (rows, L): lanes stride over the row in order, then a fixed butterfly; out[row] = sum / L
__global__ __launch_bounds__(THREADS) void k_pool(const float *__restrict__ y, int rows, int L, float *__restrict__ out) {
    const int row = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *r = y + (size_t)row * L;
    float s = 0.f;
    for (int i = lane; i < L; i += 64) s += r[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) out[row] = s / (float)L;
}

static int check_layer(const stito_fxenc_layer *ly, int idx, int B, int64_t L) {
    STITO_REQUIRE(ly != nullptr, STITO_E_INVALID, "fxenc: layer %d is NULL", idx);
    STITO_REQUIRE(ly->dilation == 1, STITO_E_UNSUPPORTED, "fxenc: layer %d has dilation %d; only dilation 1 is built", idx, ly->dilation);
    STITO_REQUIRE(ly->cin >= 1 && ly->cout >= 1 && ly->kernel >= 1 && ly->stride >= 1 && ly->cin <= 65536 && ly->cout <= 65536 &&
                      ly->kernel <= 4096 && ly->stride <= 4096,
                  STITO_E_INVALID, "fxenc: layer %d: cin %d, cout %d, kernel %d, stride %d", idx, ly->cin, ly->cout, ly->kernel, ly->stride);
    STITO_REQUIRE(!ly->residual || (ly->cin == ly->cout && ly->stride == 1), STITO_E_INVALID,
                  "fxenc: layer %d adds its input but maps %d to %d channels at stride %d", idx, ly->cin, ly->cout, ly->stride);
    STITO_REQUIRE(B >= 1 && L >= 1, STITO_E_INVALID, "fxenc: layer %d: B = %d, L = %lld", idx, B, (long long)L);
    const int r_pad = ly->kernel - 1 - (ly->kernel - 1) / 2;
    STITO_REQUIRE(L > r_pad, STITO_E_INVALID, "fxenc: layer %d (kernel %d) reflects %d samples and needs more than that; its input has %lld",
                  idx, ly->kernel, r_pad, (long long)L);
    const int64_t Lout = out_len(L, ly->stride);
    STITO_REQUIRE((int64_t)B * std::max<int64_t>(ly->cin, ly->cout) * L < (int64_t)1 << 40 && (int64_t)B * Lout < ((int64_t)1 << 31) - 512 &&
                      L < ((int64_t)1 << 30),
                  STITO_E_UNSUPPORTED, "fxenc: layer %d: %d items of %lld positions are more than one launch indexes", idx, B, (long long)L);
    return STITO_OK;
}

template <int BM, int BN, int WM, int WN>
static void launch_mfma(const stito_fxenc_layer *ly, const float *x, int B, int L, int Lout, float *y, hipStream_t st) {
    const int N = B * Lout;
    dim3 grid((unsigned)((N + BN - 1) / BN), (unsigned)((ly->cout + BM - 1) / BM));
    hipLaunchKernelGGL((k_conv_mfma<BM, BN, WM, WN>), grid, dim3(THREADS), 0, st, x, ly->w_packed_dev, ly->scale_dev, ly->shift_dev, y, B,
                       ly->cin, ly->cout, ly->kernel, ly->stride, L, Lout, ly->residual);
}

template <int K>
static void launch_valu(const stito_fxenc_layer *ly, const float *x, int B, int L, int Lout, float *y, hipStream_t st) {
    dim3 grid((unsigned)((Lout + THREADS * VALU_RUN - 1) / (THREADS * VALU_RUN)), (unsigned)B);
#define STITO_FXENC_VALU(S)                                                                                                       \
    hipLaunchKernelGGL((k_conv_valu<K, S>), grid, dim3(THREADS), 0, st, x, ly->w_packed_dev, ly->scale_dev, ly->shift_dev, y, ly->cin, \
                       ly->cout, L, Lout, ly->residual)
    if (ly->stride == 1) STITO_FXENC_VALU(1);
    else if (ly->stride == 2) STITO_FXENC_VALU(2);
    else STITO_FXENC_VALU(4);
#undef STITO_FXENC_VALU
}

static int conv1d(const stito_fxenc_layer *ly, int idx, const float *x, int B, int64_t L64, float *y, hipStream_t st) {
    STITO_TRY(check_layer(ly, idx, B, L64));
    STITO_REQUIRE(x && y && ly->w_packed_dev && ly->scale_dev && ly->shift_dev, STITO_E_INVALID, "fxenc: layer %d: NULL pointer", idx);
    const int L = (int)L64, Lout = (int)out_len(L64, ly->stride);
    const int bm = tile_m(ly->cout, ly->cin, ly->kernel, ly->stride);
    if (bm == 0) {
        STITO_REQUIRE(B <= 65535, STITO_E_UNSUPPORTED, "fxenc: layer %d: %d items exceed the grid of the %d-channel kernel", idx, B, ly->cin);
        switch (ly->kernel) {
            case 25: launch_valu<25>(ly, x, B, L, Lout, y, st); break;
            case 15: launch_valu<15>(ly, x, B, L, Lout, y, st); break;
            case 10: launch_valu<10>(ly, x, B, L, Lout, y, st); break;
            default: launch_valu<5>(ly, x, B, L, Lout, y, st); break;
        }
    } else if (bm == 32) {
        launch_mfma<32, 256, 1, 4>(ly, x, B, L, Lout, y, st);
    } else if (bm == 64) {
        launch_mfma<64, 128, 2, 2>(ly, x, B, L, Lout, y, st);
    } else {
        launch_mfma<128, 128, 2, 2>(ly, x, B, L, Lout, y, st);
    }
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

static int pool(const float *y, int B, int C, int64_t L, float *out, hipStream_t st) {
    STITO_REQUIRE(y && out && B >= 1 && C >= 1 && L >= 1 && L < ((int64_t)1 << 31) && (int64_t)B * C < ((int64_t)1 << 31), STITO_E_INVALID,
                  "fxenc pool: B = %d, C = %d, L = %lld", B, C, (long long)L);
    const int rows = B * C;
    hipLaunchKernelGGL(k_pool, dim3((unsigned)((rows + 3) / 4)), dim3(THREADS), 0, st, y, rows, (int)L, out);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

// walks the stack's shapes: every layer checked, the largest map any layer writes -> floats of one ping-pong buffer
static int plan(const stito_fxenc_model *m, int B, int64_t L, size_t *buf_floats, int64_t *L_last) {
    STITO_REQUIRE(m != nullptr && m->n_layers >= 1 && m->layers != nullptr, STITO_E_INVALID, "fxenc: empty model");
    size_t most = 0;
    int c = m->layers[0].cin;
    for (int i = 0; i < m->n_layers; ++i) {
        const stito_fxenc_layer *ly = &m->layers[i];
        STITO_TRY(check_layer(ly, i, B, L));
        STITO_REQUIRE(ly->cin == c, STITO_E_INVALID, "fxenc: layer %d takes %d channels, the layer before gives %d", i, ly->cin, c);
        L = out_len(L, ly->stride);
        c = ly->cout;
        most = std::max(most, (size_t)B * c * (size_t)L);
    }
    *buf_floats = most;
    *L_last = L;
    return STITO_OK;
}

}  // namespace fxenc
}  // namespace stito

using namespace stito;

extern "C" int64_t stito_fxenc_out_len(int64_t n_positions, int stride) {
    return n_positions >= 1 && stride >= 1 ? fxenc::out_len(n_positions, stride) : 0;
}

extern "C" int stito_fxenc_tile_m(int cout, int cin, int kernel, int stride) {
    if (cout < 1 || cin < 1 || kernel < 1 || stride < 1) return STITO_E_INVALID;
    return fxenc::tile_m(cout, cin, kernel, stride);
}

extern "C" int stito_fxenc_tile_k(void) { return fxenc::BK; }

extern "C" size_t stito_fxenc_packed_floats(int cout, int cin, int kernel, int stride) {
    if (cout < 1 || cin < 1 || kernel < 1 || stride < 1) return 0;
    return fxenc::packed_floats(cout, cin, kernel, stride);
}

extern "C" int stito_fxenc_conv1d(const stito_fxenc_layer *layer, const float *x_dev, int n_items, int64_t n_positions, float *y_dev,
                                  void *stream) {
    return fxenc::conv1d(layer, 0, x_dev, n_items, n_positions, y_dev, (hipStream_t)stream);
}

extern "C" int stito_fxenc_pool(const float *y_dev, int n_items, int channels, int64_t n_positions, float *out_dev, void *stream) {
    return fxenc::pool(y_dev, n_items, channels, n_positions, out_dev, (hipStream_t)stream);
}

extern "C" size_t stito_fxenc_workspace_bytes(const stito_fxenc_model *model, int n_items, int64_t n_samples) {
    size_t buf = 0;
    int64_t L_last = 0;
    if (fxenc::plan(model, n_items, n_samples, &buf, &L_last) != STITO_OK) return 0;
    WsLayout ws;
    ws.add(buf * sizeof(float));
    ws.add(buf * sizeof(float));
    return ws.total;
}

extern "C" int stito_fxenc_forward(const stito_fxenc_model *model, const float *x_dev, int n_items, int64_t n_samples, void *workspace_dev,
                                   size_t workspace_bytes, float *out_dev, void *stream) {
    size_t buf = 0;
    int64_t L_last = 0;
    STITO_TRY(fxenc::plan(model, n_items, n_samples, &buf, &L_last));   // every layer's length rule, before anything is launched
    STITO_REQUIRE(x_dev && out_dev && workspace_dev, STITO_E_INVALID, "stito_fxenc_forward: NULL pointer");
    WsLayout ws;
    const size_t off[2] = {ws.add(buf * sizeof(float)), ws.add(buf * sizeof(float))};
    STITO_REQUIRE(workspace_bytes >= ws.total, STITO_E_WORKSPACE, "stito_fxenc_forward: workspace %zu < %zu bytes", workspace_bytes, ws.total);
    hipStream_t st = (hipStream_t)stream;
    const float *cur = x_dev;
    int64_t L = n_samples;
    for (int i = 0; i < model->n_layers; ++i) {
        float *dst = reinterpret_cast<float *>(static_cast<char *>(workspace_dev) + off[i & 1]);
        STITO_TRY(fxenc::conv1d(&model->layers[i], i, cur, n_items, L, dst, st));
        L = fxenc::out_len(L, model->layers[i].stride);
        cur = dst;
    }
    return fxenc::pool(cur, n_items, model->layers[model->n_layers - 1].cout, L, out_dev, st);
}
