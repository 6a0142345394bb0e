// conv_layout.h -- pieces shared by the 3x3-conv kernels of the Cnn14 trunk (cnn14.hip, conv_wino43.hip): the
// channel-blocked activation layout, native vector types, explicit packed-f32 arithmetic and the LDS-DMA copy.
#pragma once
#include "common.h"

namespace stito {

// Activation layout: channel-blocked NC8HW8 -- element (stream s, channel c, row h, column w) of a map
// with C channels lives at (((s * C/8 + c/8) * H + h) * W + w) * 8 + c%8.  Eight consecutive
// channels of a pixel are 32 B, and for one channel block consecutive pixels are contiguous: a
// K-chunk's halo patch rows are dense 32-B-per-pixel runs (NHWC would touch one 32-B piece out of
// every 4*C-byte pixel vector per chunk: 4x line over-fetch, measured as the Winograd limiter).
__device__ __forceinline__ int64_t act_off(int64_t s, int c, int h, int w, int C, int H, int W) {
    return ((((s * (C >> 3)) + (c >> 3)) * H + h) * (int64_t)W + w) * 8 + (c & 7);
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct ConvShape {
    int S, H, W, Cin, Cout;
};

// Packed f32 arithmetic, issued explicitly: inside the MFMA loops hipcc splits native-vector f32x4 expressions into
// scalar v_fma / v_sub (twice the VALU instructions, and every VALU instruction is taken out of the MFMA stream's time).
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) {
    f32x2 d;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ f32x2 pk_mul(f32x2 a, f32x2 b) {
    f32x2 d;
    asm("v_pk_mul_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
    f32x2 d;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {  // a + (-b): exact, bit-identical to v_sub_f32
    f32x2 d;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
    return d;
}

// LDS-DMA: 16 B per lane, global (sbase SGPR pair, wave-uniform, + voff per-lane byte offset) -> LDS at M0 + lane * 16,
// no VGPR round trip and no VALU instruction.  M0 is not saved: nothing else in the kernels that use this reads it
// (gfx950 LDS instructions do not, and they have no movrel / sendmsg / interp); hipcc rejects "m0" in a clobber list as
// reserved, so that is checked by inspection of the ISA (grep m0: only these statements and w43_xch_put of conv_wino43.hip, which
// sets it in front of its own stores in the same way, write it).
__device__ __forceinline__ void glds16_m0(const float *sbase, unsigned voff, unsigned lds_byte_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(sbase), "s"(lds_byte_addr) : "memory");
}

// Division by a runtime divisor that is fixed per launch (map height, tile rows per stream, ...).  hipcc turns `a / d`
// into a ~35-instruction sequence; a conv workgroup does ten of them before it can issue its first copy (measured: 700 of
// its ~7 400 prologue cycles).  For 0 <= a < 2^22 and 1 <= d < 2^22 the float quotient is off by at most one, which the
// remainder check repairs exactly; larger operands take the compiler's division.
struct FDiv {
    int d;
    float rcp;
};
static inline FDiv make_fdiv(int d) { return FDiv{d, 1.0f / (float)d}; }
__device__ __forceinline__ int fdiv(int a, const FDiv f, int &rem) {
    if ((unsigned)(a | f.d) >= (1u << 22)) {
        rem = a % f.d;
        return a / f.d;
    }
    int q = (int)(__int2float_rn(a) * f.rcp);
    int r = a - q * f.d;
    if (r < 0) { --q; r += f.d; }
    else if (r >= f.d) { ++q; r -= f.d; }
    rem = r;
    return q;
}

// ---- the 3x3-conv algorithms (the STITO_CONV_* ids of stito_hip.h): what the C entry points and the trunk know about each ----

// One launch: `w` is the algorithm's packing; `ws` its workspace (stito_conv3x3_workspace_bytes) or NULL.
// amax_out (or NULL): per stream, the layer's largest output as a bit pattern (atomicMax into a buffer the caller zeroed);
// amax_in (or NULL): the same of the layer that produced `in` -- without it the algorithms that read maxima scan `in` themselves
struct ConvArgs {
    const float *in, *w, *scale, *shift;
    float *out;
    ConvShape c;
    bool pool;
    void *ws;
    size_t ws_bytes;
    hipStream_t st;
    const unsigned *amax_in;
    unsigned *amax_out;
    long long *trace;   // stito_debug_wino_trace buffer or NULL (the float32 Winograd kernels' timeline builds)
};

struct ConvAlgo {
    const char *name;            // in error messages
    bool retired;                // (ABI version 9) unsupported, no packing, refused by the workspace entry
    bool winograd;               // a packing stito_cnn14_weights.conv_wino_dev can hold
    bool reads_amax;             // scales its transformed input by per-stream maxima of its input (amax_in)
    bool reports_amax;           // can report per-stream maxima of its output (amax_out)
    int same_packing = -1;       // the id that runs the same packing where this one does not cover the shape (-1: none)
    // shape and channel checks of this algorithm; the C entry points have checked n, H, W > 0, cout % 4 and the pooled size
    bool (*supported)(const ConvShape &c, bool pool);
    size_t (*packed_floats)(int cout, int cin);
    int (*pack)(const float *w_oihw, int cout, int cin, float *packed, hipStream_t st);
    double (*issued_flops)(const ConvShape &c, bool pool);      // for a supported shape with cin % 8 == 0
    size_t (*workspace_bytes)(const ConvShape &c, bool pool);   // for a supported shape; NULL: needs no workspace
    // without a workspace: after the checks of stito_conv3x3_bn_relu; with one: checks the shape and the workspace itself
    int (*launch)(const ConvArgs &a);
    bool needs_workspace() const { return workspace_bytes != nullptr; }
};

const ConvAlgo &conv_algo(int id);   // cnn14.hip; unknown ids: the direct kernel
// (functions, not objects: hipcc would also emit a constant-initialised global on the device, host function pointers and all)
const ConvAlgo &wino43_algo(), &wino43_pre_algo(), &wino43_split_algo(), &wino43_split2_algo(), &wino43_split3_algo();   // conv_wino43.hip
const ConvAlgo &wino23r_algo();                                                                                            // conv_wino23r.hip

// conv_wino43.hip: workgroups of the six-sweep kernel that have work (the trunk's choice between it and the two-sweep kernel)
int64_t wino43_split3_workgroups(const ConvShape &c, bool pool);
// conv_block1 in one launch on the register-resident F(2x2,3x3) kernel (conv_wino23r.hip): the first conv (1 -> 64 channels, bn1,
// ReLU) is computed on the matrix pipe into the patch ring in the slots where the unfused kernel issues its copies (c: the second
// conv's shape)
bool wino23r_fused1_supported(const ConvShape &c, bool pool);
size_t wino23r_fused1_workspace_bytes(const ConvShape &c, bool pool);
size_t conv1_f2reg_packed_floats();
int pack_conv1_f2reg(const float *w_dev, const float *scale_dev, const float *shift_dev, int c1, float *packed, hipStream_t st);
int launch_wino23r_fused1(const float *logmel, const float *c1pk, const float *wpk, const float *scale, const float *shift, float *out,
                          const ConvShape &c, bool pool, void *ws, size_t ws_bytes, hipStream_t st, unsigned *amax_out);

}  // namespace stito
