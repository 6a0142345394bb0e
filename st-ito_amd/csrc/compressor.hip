// compressor.hip -- juce::dsp::Compressor<float> (peak ballistics + VCA) for a population of streams,
// time-parallel.  Replaces BasicCompressor.process (reference st_ito/effects.py:873-897, pedalboard.Compressor =
// juce::dsp::Compressor: BallisticsFilter::processSample + the gain computer) inside the per-candidate loop of
// st_ito/style_transfer.py:512-521.
//
// The envelope is a switching one-pole,
//     y' = v + c (y - v),   c = (v > y) ? c_att : c_rel,   v = |x|,
// serial in time and not linear, so it has no associative scan in the usual sense.  It does have one over the
// (max, +) structure.  Both candidates are increasing affine maps of y and the selected one is the larger
// (c_att <= c_rel) or the smaller (c_att > c_rel; then run the same thing on z = -y), so one step is
//     z' = max(c_att z + a, c_rel z + r),      (a, r) = s ((1 - c_att) v, (1 - c_rel) v),  s = +-1,  env = |z|.
// A step is a max of two increasing affine maps; a composition of K steps is a max over the 2^K attack/release
// paths, and all paths with the same number j of attack steps share the slope c_att^j c_rel^(K-j): only the
// largest intercept of each slope can ever win.  A block of K samples therefore IS the function
//     F(z) = max_{j=0..K} (S_j z + B_j),        S_j = c_att^j c_rel^(K-j),
// with K+1 intercepts that build up by   B'_j = max(c_att B_{j-1} + a_n, c_rel B_j + r_n)   -- K+1 lanes, K steps,
// independent of every other block.  With K = 15 a block is a 16-lane DPP row:
//
//   k_comp_blockfn   (parallel over all blocks)  intercepts B_0..B_15 of every full 15-sample block,
//   k_comp_blockscan (serial over blocks, 4 lanes per stream) z at every block boundary: 16 terms per 15 samples
//                    instead of 15 dependent steps -- ~9 instructions of the one serial wave per block, where
//                    walking the samples costs 3 per SAMPLE (the kernel this replaces: 6.5 ms at 512 x 480 000),
//   k_comp_apply     (parallel over all blocks)  re-walks each block from its boundary state with the reference's
//                    own per-sample operations, v + c (y - v), each rounded, and applies the VCA in the same pass
//                    (no envelope buffer in HBM).
//   k_comp_stage     all three as wave roles of one workgroup per one or two streams, segment by segment through LDS: what
//                    compressor_stage launches; same bits.
//
// Rounding: inside a block every sample goes through the reference's float operations in the reference's order (the
// first block is bit-identical to a sequential walk); the boundary states come out of a different, shorter
// sequence -- every term a sum of same-signed products, no cancellation -- and the map is contractive, so a
// boundary's few ulp decay instead of accumulating.  Parity bound of the effect stays 2e-5 of peak.
#include "common.h"
#include "dsp_view.h"
#include "comp_scan.inc"
#include "comp_stage.inc"

namespace stito {

static constexpr int CB_K = 15;        // samples per block; K + 1 = 16 intercepts = one DPP row
static constexpr int CB_TILE = 128;    // blocks per workgroup of k_comp_blockfn (4 waves x 8 iterations x 4 rows)
static constexpr int CB_D = STITO_COMP_SCAN_DEPTH;  // blocks in flight per lane in k_comp_blockscan (register ring)
static constexpr int CA_TILE = 256;    // blocks per workgroup of k_comp_apply (one block per thread)
static constexpr float CB_CMIN = 1.0e-30f;  // c = 0 (times below 1e-3 ms) would turn -inf * c into NaN in the intercept
                                            // recurrence; 1e-30 z is below every ulp that matters and -inf stays -inf

typedef float cb_f2 __attribute__((ext_vector_type(2)));
typedef float cb_f4 __attribute__((ext_vector_type(4)));

struct CompGeom {
    int64_t L;
    int64_t n_blocks;   // ceil(L / K): blocks k_comp_apply walks
    int64_t n_fn;       // n_blocks - 1: blocks whose function is needed (every one but the last is full)
    int64_t fn_stride;  // floats between streams in the intercept array: (n_fn + 2 CB_D) * 16 (the ring over-reads)
    int64_t z_stride;   // floats between streams in the boundary-state array: round_up(n_fn, CB_D) + CB_D
};

static CompGeom comp_geometry(int64_t L) {
    CompGeom g;
    g.L = L;
    g.n_blocks = (L + CB_K - 1) / CB_K;
    g.n_fn = g.n_blocks - 1;
    g.fn_stride = (g.n_fn + 2 * CB_D) * 16;
    g.z_stride = (g.n_fn + CB_D - 1) / CB_D * CB_D + CB_D;
    return g;
}

struct CompLayout : WsLayout { size_t fn, z_end; };   // block functions | boundary states
static CompLayout comp_layout(int n_streams, const CompGeom &g) {
    CompLayout l;
    l.fn = l.add((size_t)n_streams * g.fn_stride * sizeof(float));
    l.z_end = l.add((size_t)n_streams * g.z_stride * sizeof(float));
    return l;
}
size_t compressor_workspace_bytes(int n_streams, int64_t n_samples) { return comp_layout(n_streams, comp_geometry(n_samples)).total; }

struct CompCoef {
    float thr, thr_inv, p, cat, crl, sg;
};
__device__ __forceinline__ CompCoef comp_coef(const double *coef, int cand) {
    const double *cf = coef + (int64_t)cand * COEF_STRIDE;
    CompCoef c;
    c.thr = (float)cf[0];
    c.thr_inv = (float)cf[1];
    c.p = (float)cf[2];
    c.cat = (float)cf[3];
    c.crl = (float)cf[4];
    c.sg = c.cat <= c.crl ? 1.0f : -1.0f;
    return c;
}

template <int CTRL>
__device__ __forceinline__ float dpp(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                                 CTRL, 0xf, 0xf, false));
}

// ------------------------------------------------------------------------------------------------
// A. intercepts of every full block.  Workgroup = CB_TILE consecutive blocks of one stream: the samples are
// expanded to (a, r) pairs in LDS once (coalesced loads), then every 16-lane row of every wave walks one
// block: lane j keeps B_j; per sample one row_shr:1 (B_{j-1}), one packed FMA, one max.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_comp_blockfn(InView in, float *__restrict__ fn, CompGeom g, int C,
                                                       const double *__restrict__ coef) {
    __shared__ cb_f2 pairs[CB_TILE * CB_K];
    const int s = blockIdx.y, cand = s / C, ch = s % C;
    const float *x = in_ptr(in, cand, ch);
    const CompCoef cc = comp_coef(coef, cand);
    const float sa = cc.sg * (1.0f - cc.cat), sr = cc.sg * (1.0f - cc.crl);
    const cb_f2 c2 = {fmaxf(cc.cat, CB_CMIN), fmaxf(cc.crl, CB_CMIN)};
    const int64_t blk0 = (int64_t)blockIdx.x * CB_TILE, t0 = blk0 * CB_K;
    for (int i = threadIdx.x; i < CB_TILE * CB_K; i += 256) {
        const float v = t0 + i < g.L ? fabsf(x[t0 + i]) : 0.0f;
        pairs[i] = (cb_f2){sa * v, sr * v};
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, row = lane >> 4, j = lane & 15;
    const float ninf = -__builtin_inff();
    float *out = fn + (int64_t)s * g.fn_stride;
#pragma unroll 2
    for (int it = 0; it < CB_TILE / 16; ++it) {
        const int bl = w * (CB_TILE / 4) + it * 4 + row;
        const cb_f2 *pr = pairs + bl * CB_K;
        float B = j == 0 ? 0.0f : ninf;
#pragma unroll
        for (int n = 0; n < CB_K; ++n) {
            const float sh = dpp<0x111>(ninf, B);  // row_shr:1, lane 0 of the row keeps -inf
            const cb_f2 t = __builtin_elementwise_fma(c2, (cb_f2){sh, B}, pr[n]);
            B = fmaxf(t.x, t.y);
        }
        if (blk0 + bl < g.n_fn) out[(blk0 + bl) * 16 + j] = B;
    }
}

// ------------------------------------------------------------------------------------------------
// B. boundary states.  Four lanes per stream, four terms per lane; the 16-term max closes over the quad with two
// DPP quad_perm steps.  Intercepts come straight from HBM through a CB_D-deep register ring (one b128 per
// block per lane); states leave as one b128 per four blocks.  z_end[k] = state after block k.  The loop body
// is generated asm (comp_scan.inc, tools/gen/gen_comp_scan_asm.py): 9.6 instructions per block.
// ------------------------------------------------------------------------------------------------
// spw = streams per wave (a power of two <= 16): with fewer than sixteen, the upper quads shadow the lower ones (same values from and to
// the same addresses, like the idle quads past the last stream) and the launch has 16 / spw times as many waves.  The scan is one
// dependent chain per stream, but at sixteen streams a wave also pulls 16 x 2 MB of intercepts through ONE CU's memory pipe (35 GB/s
// per CU at 512 streams: 0.93 ms against a chain of ~0.72); spreading the streams over more CUs takes that off the chain.
__global__ __launch_bounds__(64) void k_comp_blockscan(const float *__restrict__ fn, float *__restrict__ z_end, CompGeom g,
                                                        int C, int S, const double *__restrict__ coef, int spw) {
    const int lane = threadIdx.x, q = lane & 3;
    const int s_raw = blockIdx.x * spw + ((lane >> 2) & (spw - 1));
    const int s = s_raw < S ? s_raw : S - 1;  // idle quads shadow the last stream (same values to the same addresses)
    const CompCoef cc = comp_coef(coef, s / C);
    const double ca = fmaxf(cc.cat, CB_CMIN), cr = fmaxf(cc.crl, CB_CMIN);
    float S4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int jj = 4 * q + u;
        S4[u] = (float)(pow(ca, (double)jj) * pow(cr, (double)(CB_K - jj)));
    }
    const cb_f2 S01 = {S4[0], S4[1]}, S23 = {S4[2], S4[3]};
    const cb_f4 *src = (const cb_f4 *)(fn + (int64_t)s * g.fn_stride) + q;  // block k at src[4 k]
    float *dst = z_end + (int64_t)s * g.z_stride;
    const int64_t n_ring = (g.n_fn + CB_D - 1) / CB_D;
    STITO_COMP_SCAN_PROLOGUE(src, dst + n_ring * CB_D);
    float z = 0.0f;
    for (int64_t r = 0; r < n_ring; ++r) {
        STITO_COMP_SCAN_PASS(z, S01, S23, src, dst);
        src += 4 * CB_D;
        dst += CB_D;
    }
    STITO_COMP_SCAN_DRAIN();
}

// ------------------------------------------------------------------------------------------------
// C. envelope + VCA.  gain = env < thr ? 1 : pow(env/thr, 1/ratio - 1); y = gain * x.  The power goes through
// v_log_f32 / v_exp_f32 (1 ulp each; base >= 1, |exponent| < 1: relative error < 2e-6 against powf, inside the
// 2e-5 parity bound of the effect).  One thread = one block: its 15 samples come out of an LDS tile that was
// loaded and is stored coalesced (stride 15 floats between lanes: conflict-free), so the kernel is bound by its
// 8 bytes per sample of HBM traffic.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vca_gain(float e, float thr, float thr_inv, float p) {
    return e < thr ? 1.0f : __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(e * thr_inv));
}

__global__ __launch_bounds__(CA_TILE) void k_comp_apply(InView in, float *out, const float *__restrict__ z_end,
                                                         CompGeom g, int64_t cand_stride, int C,
                                                         const double *__restrict__ coef) {
    __shared__ float tile[CA_TILE * CB_K];
    const int s = blockIdx.y, cand = s / C, ch = s % C;
    const float *x = in_ptr(in, cand, ch);
    float *y = out + (int64_t)cand * cand_stride + (int64_t)ch * g.L;
    const CompCoef cc = comp_coef(coef, cand);
    const int64_t blk0 = (int64_t)blockIdx.x * CA_TILE, t0 = blk0 * CB_K;
    const int n_here = (int)((g.L - t0 < CA_TILE * CB_K) ? g.L - t0 : CA_TILE * CB_K);
    for (int i = threadIdx.x; i < n_here; i += CA_TILE) tile[i] = x[t0 + i];
    const int64_t k = blk0 + threadIdx.x;
    float env = (k > 0 && k < g.n_blocks) ? fabsf(z_end[(int64_t)s * g.z_stride + k - 1]) : 0.0f;  // env = |z|
    __syncthreads();
    float *mine = tile + threadIdx.x * CB_K;
    if (threadIdx.x * CB_K < n_here) {  // samples past L inside the last block: computed on stale LDS, never stored
#pragma unroll
        for (int n = 0; n < CB_K; ++n) {
            // inside a block: the reference's own operations in the reference's order, each rounded (no contraction)
            const float xv = mine[n], v = fabsf(xv);
            const float c = v > env ? cc.cat : cc.crl;
            env = __fadd_rn(v, __fmul_rn(c, __fsub_rn(env, v)));
            mine[n] = vca_gain(env, cc.thr, cc.thr_inv, cc.p) * xv;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_here; i += CA_TILE) y[t0 + i] = tile[i];
}

// ------------------------------------------------------------------------------------------------
// A + B + C in one kernel (the default; STITO_COMP_FUSED=0 selects the three passes above, which stay as the reference of the
// bitwise test).  The three passes leave the device to 64 waves for as long as B's chain runs and carry the intercepts (16 floats
// per 15 samples) and a second read of the audio through HBM.  Here one workgroup owns NS streams and walks them in segments of
// CS_G blocks, ONE workgroup barrier per step, the roles on separate waves (as in k_reverb):
//   scan wave (wave 0, alone on its SIMD)  B on segment t - 1: the same chain on the same packed FMAs (comp_stage.inc), its block
//                   functions out of LDS, the boundary states into LDS;
//   A waves         k_comp_blockfn's recurrence on segment t, two units of four blocks at a time (comp_stage.inc); the samples
//                   come out of registers loaded two steps ahead, so no wave waits for HBM inside a step;
//   C waves         k_comp_apply's statements on segment t - 2, on the samples A staged and the states the scan left.
// Every dependency between waves is closed by the step's barrier; nothing waits for another workgroup.  The audio is read once
// and written once, intercepts and states never leave the CU.  The bits are those of the three passes (tested): the same
// operations on the same values; only the places the values wait in differ.
// What bounds it: a wave issues one instruction every ~7.5 cycles whatever it is, so a step lasts as long as its longest wave --
// the scan's 612 instructions per segment (2.0 us) once no helper wave has more (hence twelve of them).
// ------------------------------------------------------------------------------------------------
static constexpr int CS_G = STITO_COMP_STAGE_G;   // blocks per segment
static constexpr int CS_SEG = CS_G * CB_K;        // samples per segment
static constexpr int CS_NH = 12;                  // helper waves, four on each SIMD but the scan wave's: ONE wave issues an instruction every ~7.5 cycles whatever it
                                                  // is (measured: 612 instructions of the scan, 155 of a helper's pair of units), so a step is as long as its longest wave
static constexpr int CS_THREADS = 16 * 64;        // + the scan wave + waves 4, 8 and 12, which would share its SIMD and only keep the barrier count
static constexpr int CS_UNIT = 4 * CB_K;          // samples per unit of A: one wave iteration = four blocks, one per DPP row
static constexpr int CS_UPS = CS_G / 4;           // units per stream and segment
static constexpr int CS_ZS = 4 + CS_G;            // floats per row of states: [3] = state entering the segment, [4 + i] = after block i

// LDS only: the A waves' loads for the steps ahead stay in flight across the barrier
#define CS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
// orders a wave's own LDS accesses (written by some lanes, read by others) for the compiler; the hardware keeps them in issue order
#define CS_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

__device__ __forceinline__ uint32_t cs_lds_addr(const void *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

// units of A per helper wave (C on one stream segment costs about five of them): helper h owns units [first, first + count) of
// the NS * CS_UPS of a step and C of stream `c_stream` (-1: none)
template <int NS> struct CsSplit;
// helpers 0, 3, 6, 9 share a SIMD, as do 1, 4, 7, 10 and 2, 5, 8, 11; a wave's units never cross a stream
template <> struct CsSplit<1> { static constexpr int MAXU = 2; static constexpr int first[CS_NH] = {0, 4, 10, 2, 6, 12, 14, 8, 14, 14, 14, 14}, count[CS_NH] = {2, 2, 2, 2, 2, 2, 0, 2, 2, 0, 0, 0}, c_stream[CS_NH] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, 0, -1, -1}; };
template <> struct CsSplit<2> { static constexpr int MAXU = 4; static constexpr int first[CS_NH] = {0, 16, 10, 4, 20, 26, 8, 24, 14, 28, 28, 30}, count[CS_NH] = {4, 4, 4, 4, 4, 4, 2, 2, 2, 0, 0, 2}, c_stream[CS_NH] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 1, -1}; };

// LDS of k_comp_stage<NS>, in floats
template <int NS> struct CsLds {
    static constexpr int fn = 0;                                   // [2][NS][CS_G * 16] intercepts of segment t: A writes, the scan reads
    static constexpr int z = fn + 2 * NS * CS_G * 16;              // [2][NS][CS_ZS]     states: the scan writes, C reads
    static constexpr int cf = z + 2 * NS * CS_ZS;                  // [NS][4]            sa, sr, c_att, c_rel of each stream
    static constexpr int x = cf + NS * 4;                          // [3][NS][CS_SEG]    samples: A stages, C works in place two steps later
    static constexpr int total = x + 3 * NS * CS_SEG;
    static_assert(z % 4 == 0 && cf % 4 == 0, "b128 alignment");
    static_assert(total * 4 <= 64 * 1024, "beyond this a launch has to raise hipFuncAttributeMaxDynamicSharedMemorySize first");
};

template <int NS>
__global__ __launch_bounds__(CS_THREADS) void k_comp_stage(InView in, float *out, CompGeom g, int64_t cand_stride, int C, int S,
                                                     const double *__restrict__ coef) {
    typedef CsSplit<NS> SP;
    typedef CsLds<NS> LD;
    extern __shared__ __attribute__((aligned(16))) float cs_smem[];
    float (*s_fn)[NS][CS_G * 16] = (float (*)[NS][CS_G * 16])(cs_smem + LD::fn);
    float (*s_z)[NS][CS_ZS] = (float (*)[NS][CS_ZS])(cs_smem + LD::z);
    float (*s_cf)[4] = (float (*)[4])(cs_smem + LD::cf);
    float (*s_x)[NS][CS_SEG] = (float (*)[NS][CS_SEG])(cs_smem + LD::x);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int s0 = blockIdx.x * NS;
    // every wave runs the same steps: A is two segments ahead of C, and the count is a whole number of turns of A's three register sets
    const int n_seg = (int)((g.n_blocks + CS_G - 1) / CS_G), n_steps = (n_seg + 2 + 2) / 3 * 3;
    if (threadIdx.x < NS) {
        const int s = s0 + threadIdx.x < S ? s0 + threadIdx.x : S - 1;   // a stream past the last one shadows it and stores nothing
        const CompCoef cc = comp_coef(coef, s / C);
        s_cf[threadIdx.x][0] = cc.sg * (1.0f - cc.cat);
        s_cf[threadIdx.x][1] = cc.sg * (1.0f - cc.crl);
        s_cf[threadIdx.x][2] = fmaxf(cc.cat, CB_CMIN);
        s_cf[threadIdx.x][3] = fmaxf(cc.crl, CB_CMIN);
    }
    CS_BARRIER();
    if (w == 0) {
        // ---- scan role: four lanes per stream
        const int q = lane & 3, sl = (lane >> 2) % NS;
        const int s = s0 + sl < S ? s0 + sl : S - 1;
        const CompCoef cc = comp_coef(coef, s / C);
        const double ca = fmaxf(cc.cat, CB_CMIN), cr = fmaxf(cc.crl, CB_CMIN);
        float S4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = 4 * q + u;
            S4[u] = (float)(pow(ca, (double)jj) * pow(cr, (double)(CB_K - jj)));
        }
        const cb_f2 S01 = {S4[0], S4[1]}, S23 = {S4[2], S4[3]};
        const uint32_t fn0 = cs_lds_addr(&s_fn[0][sl][4 * q]), fn1 = cs_lds_addr(&s_fn[1][sl][4 * q]);
        const uint32_t z0 = cs_lds_addr(&s_z[0][sl][0]), z1 = cs_lds_addr(&s_z[1][sl][0]);
        float z = 0.0f;
        // only the streams' own quads run (the wave meets the barrier whatever its exec mask): a full wave's ds_read_b128 costs the
        // LDS sixteen times the bytes the streams need, and the helpers live on that bandwidth
        if (lane < 4 * NS) {
            for (int t = 0; t < n_steps; ++t) {
                if (t >= 1 && t <= n_seg) {   // segment t - 1
                    const uint32_t fa = (t - 1) & 1 ? fn1 : fn0, za = (t - 1) & 1 ? z1 : z0;
                    STITO_COMP_STAGE_SEGMENT(z, S01, S23, fa, za);
                }
                CS_BARRIER();
            }
        }
    } else if ((w & 3) == 0) {
        // ---- waves 4, 8 and 12 land on the scan wave's SIMD: they only meet the barriers
        for (int t = 0; t < n_steps; ++t) CS_BARRIER();
    } else {
        // ---- helper roles: a wave has units of A or one stream's C, never both -- an A wave's vmcnt then holds only its loads
        // and a C wave's only its stores
        const int h = w - 1 - (w >> 2), u0 = SP::first[h], un = SP::count[h], c_sl = SP::c_stream[h];
        if (c_sl >= 0) {
            // ---- C on segment t - 2: one lane = one block, from the state the scan left in front of it; in place in s_x, stored coalesced
            const int c_s = s0 + c_sl;
            const bool c_on = c_s < S;
            const int c_sc = c_on ? c_s : S - 1;
            const CompCoef cc = comp_coef(coef, c_sc / C);
            float *y = out + (int64_t)(c_sc / C) * cand_stride + (int64_t)(c_sc % C) * g.L;
            float cat = cc.cat, crl = cc.crl;
            asm volatile("" : "+v"(cat), "+v"(crl));   // floats here: left alone, hipcc selects between the doubles and converts per sample
            for (int t = 0; t < n_steps; ++t) {
                if (c_on && t >= 2 && t - 2 < n_seg) {
                    const int seg = t - 2;
                    float *xb = &s_x[seg % 3][c_sl][0];
                    float env = fabsf(s_z[seg & 1][c_sl][3 + lane]);  // env = |z|
                    float *mine = xb + lane * CB_K;
                    float xv[CB_K];   // all reads first: behind the in-place writes hipcc would wait for each one in turn
#pragma unroll
                    for (int n = 0; n < CB_K; ++n) xv[n] = mine[n];
#pragma unroll
                    for (int n = 0; n < CB_K; ++n) {
                        // inside a block: the reference's own operations in the reference's order, each rounded (no contraction)
                        const float v = fabsf(xv[n]);
                        const float c = v > env ? cat : crl;
                        env = __fadd_rn(v, __fmul_rn(c, __fsub_rn(env, v)));
                        xv[n] = vca_gain(env, cc.thr, cc.thr_inv, cc.p) * xv[n];
                    }
#pragma unroll
                    for (int n = 0; n < CB_K; ++n) mine[n] = xv[n];
                    CS_WAVE_SYNC();
                    const int64_t t0 = (int64_t)seg * CS_SEG;
                    const int64_t left = g.L - t0;
                    const int n_here = (int)(left < CS_SEG ? left : CS_SEG);
                    float *yb = y + t0;
#pragma unroll
                    for (int n = 0; n < CB_K; ++n) xv[n] = xb[n * 64 + lane];
                    if (n_here == CS_SEG) {   // a whole segment: no condition per store
#pragma unroll
                        for (int n = 0; n < CB_K; ++n) yb[n * 64 + lane] = xv[n];
                    } else {
#pragma unroll
                        for (int n = 0; n < CB_K; ++n) {
                            const int i = n * 64 + lane;
                            if (i < n_here) yb[i] = xv[n];
                        }
                    }
                }
                CS_BARRIER();
            }
        } else {
            // ---- A on segment t.  All of this wave's units belong to one stream, so its coefficients and its input pointer are
            // wave constants
            const int row = lane >> 4, j = lane & 15;
            const float ninf = -__builtin_inff();
            const int a_sl = u0 / CS_UPS < NS ? u0 / CS_UPS : NS - 1;
            const int a_s = s0 + a_sl < S ? s0 + a_sl : S - 1;
            const float *xa = in_ptr(in, a_s / C, a_s % C);
            const cb_f4 cf = *(const cb_f4 *)s_cf[a_sl];
            const cb_f2 c2 = {cf.z, cf.w};
            const int off0 = (u0 % CS_UPS) * CS_UNIT + lane;   // this lane's sample of unit 0 inside the stream's segment; unit i: + i CS_UNIT

            // The samples come out of registers loaded two steps ahead.  The loads carry no condition (a clamped index instead) so
            // that they stay countable in vmcnt; what a lane must not use is zeroed where it is used
            float r0[SP::MAXU], r1[SP::MAXU], r2[SP::MAXU];   // segment t in set t % 3: no copies, so no wait for the newest loads
            auto fetch = [&](float (&dst)[SP::MAXU], int seg) {
                const int segc = seg < n_seg ? seg : n_seg - 1;   // the last segment holds at least one sample
                const int64_t left = g.L - (int64_t)segc * CS_SEG;
                const int last = (int)(left < CS_SEG ? left : CS_SEG) - 1;
                const float *xb = xa + (int64_t)segc * CS_SEG;
#pragma unroll
                for (int i = 0; i < SP::MAXU; ++i) {
                    const int o = off0 + i * CS_UNIT;
                    dst[i] = xb[o < last ? o : last];
                }
            };
            fetch(r0, 0);
            fetch(r1, 1);
            auto step = [&](int t, const float (&cur)[SP::MAXU], float (&ahead)[SP::MAXU]) {
                fetch(ahead, t + 2);
                // the samples to s_x, for the recurrence now and for C two steps on.  Units are consecutive, so unit i sits i units
                // behind unit 0 in s_x ([NS][CS_UPS units]) and in s_fn alike
                const int64_t left_t = g.L - (int64_t)t * CS_SEG;
                const int n_t = (int)(left_t < 0 ? 0 : left_t < CS_SEG ? left_t : CS_SEG);   // samples of segment t
                float *xs = &s_x[t % 3][0][0] + u0 * CS_UNIT;
                float *fo = &s_fn[t & 1][0][0] + u0 * 64 + lane;   // unit u = blocks 4 u .. 4 u + 3 of [NS][CS_G]: block 4 u + row, intercept j
#pragma unroll
                for (int i = 0; i < SP::MAXU; ++i)
                    if (i < un && lane < CS_UNIT) xs[i * CS_UNIT + lane] = off0 + i * CS_UNIT < n_t ? cur[i] : 0.0f;
                CS_WAVE_SYNC();
                // two units at a time: one chain alone is bound by its latency, two fill each other's hazard slots.  A wave with an
                // odd count would run its last second chain on another wave's samples and not store it
                const uint32_t x_row = cs_lds_addr(xs + row * CB_K);
#pragma unroll 1
                for (int i = 0; i < un; i += 2) {
                    // k_comp_blockfn's recurrence on the same operands (comp_stage.inc): (a, r) = (sa |x|, sr |x|); lane j forms
                    // c_att B_j + a for lane j + 1 and c_rel B_j + r for itself, then takes the max across row_shr:1 -- the shift after
                    // the FMA instead of before it
                    float Ba, Bb;
                    STITO_COMP_STAGE_BLOCKFN2(Ba, Bb, c2, cf.x, cf.y, j == 0 ? 0.0f : ninf, x_row + i * (CS_UNIT * 4));
                    fo[i * 64] = Ba;
                    if (i + 1 < un) fo[(i + 1) * 64] = Bb;
                }
                CS_BARRIER();
            };
            for (int t = 0; t < n_steps; t += 3) {
                step(t, r0, r2);
                step(t + 1, r1, r0);
                step(t + 2, r2, r1);
            }
        }
    }
}

int compressor_stage(const InView &in, float *audio_dev, int64_t cand_stride, int pop, int C, int64_t n_samples,
                     const double *coef, void *workspace, hipStream_t st) {
    const CompGeom g = comp_geometry(n_samples);
    const int S = pop * C;
    DeviceInfo dinfo;
    STITO_TRY(device_info(dinfo));
    const char *fused = getenv("STITO_COMP_FUSED");   // "0": the three passes (the reference of the bitwise test, and the A/B)
    if (!(fused && atoi(fused) == 0)) {
        // streams per workgroup: one while that gives every workgroup its own CU, two beyond (the bits do not depend on it)
        int ns = S > dinfo.cus ? 2 : 1;
        if (const char *e = getenv("STITO_COMP_NS")) { const int v = atoi(e); if (v == 1 || v == 2) ns = v; }  // tuning and test aid
        if (ns == 2) {
            hipLaunchKernelGGL(k_comp_stage<2>, dim3((S + 1) / 2), dim3(CS_THREADS), CsLds<2>::total * 4, st, in, audio_dev, g, cand_stride, C, S, coef);
        } else {
            hipLaunchKernelGGL(k_comp_stage<1>, dim3(S), dim3(CS_THREADS), CsLds<1>::total * 4, st, in, audio_dev, g, cand_stride, C, S, coef);
        }
        STITO_LAUNCH_CHECK();
        return STITO_OK;
    }
    const CompLayout l = comp_layout(S, g);
    float *fn = (float *)((char *)workspace + l.fn), *z_end = (float *)((char *)workspace + l.z_end);
    if (g.n_fn > 0) {
        hipLaunchKernelGGL(k_comp_blockfn, dim3((unsigned)((g.n_fn + CB_TILE - 1) / CB_TILE), S), dim3(256), 0, st, in, fn, g, C, coef);
        STITO_LAUNCH_CHECK();
        // streams per wave: eight (measured at 512 streams x 480 000 samples, the whole stage: 2.06 ms with sixteen, 1.85 with eight,
        // 1.86 with four or two, 1.93 with one), fewer while that leaves three quarters of the CUs without a wave
        int spw = 8;
        while (spw > 1 && (S + spw - 1) / spw < dinfo.cus / 4) spw >>= 1;
        if (const char *e = getenv("STITO_COMP_SPW")) { const int v = atoi(e); if (v >= 1 && v <= 16 && (v & (v - 1)) == 0) spw = v; }  // tuning aid
        hipLaunchKernelGGL(k_comp_blockscan, dim3((S + spw - 1) / spw), dim3(64), 0, st, fn, z_end, g, C, S, coef, spw);
        STITO_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_comp_apply, dim3((unsigned)((g.n_blocks + CA_TILE - 1) / CA_TILE), S), dim3(CA_TILE), 0, st, in, audio_dev,
                       z_end, g, cand_stride, C, coef);
    STITO_LAUNCH_CHECK();
    return STITO_OK;
}

}  // namespace stito
