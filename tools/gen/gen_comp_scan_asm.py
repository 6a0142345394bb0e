#!/usr/bin/env python
"""Generates st-ito_amd/csrc/comp_scan.inc: the serial wave's code of k_comp_blockscan (compressor.hip) as inline asm
with fixed registers -- a register ring of D block-function quads fed straight from HBM.

Why asm: one wave issues an instruction every ~7 cycles whatever it is, so the time per block is the instruction
count.  hipcc needs ~15 per block for this chain (it cannot fold the quad_perm into v_max_f32, canonicalises before
every max, moves results around) and waits for ALL loads at the top of its loop.  Here a block is

    v_pk_fma_f32 x2      16 terms S_j z + B_j, four per lane
    v_max3_f32, v_max_f32
    global_load_dwordx4  refill of this ring slot (block + D) -- sits in the first DPP hazard slot
    s_nop 0
    v_max_f32_dpp        quad_perm [1,0,3,2]
    s_nop 1 / the state store every fourth block
    v_max_f32_dpp        quad_perm [2,3,0,1]  -> z, written straight into the store quad

= 9 instructions, and one s_waitcnt vmcnt(N) per four blocks with N constant: loads and stores retire in issue
order, and between the load of a slot and its use exactly D - 1 loads and D / 4 stores are issued (the prologue
issues D / 4 stores of its own so that this also holds in the first pass).

Operands: %0 = z (in/out), %1 = (S0, S1), %2 = (S2, S3), %3 = 64-bit load address of this lane (block 0 of the pass),
%4 = 64-bit store address (state of block 0 of the pass).

The committed file (tests/test_generated_sources.py holds it to this output byte for byte; the instruction count per block goes
to stderr):

    python tools/gen/gen_comp_scan_asm.py > st-ito_amd/csrc/comp_scan.inc

With the argument `stage` it prints st-ito_amd/csrc/comp_stage.inc instead: the same chain for the scan wave of k_comp_stage,
which reads the block functions from LDS (ds_read_b128, a short register look-ahead) where helper waves of the same
workgroup put them, and leaves the boundary states in LDS (tests/test_gpu_comp_stage.py holds that file to this output):

    python tools/gen/gen_comp_scan_asm.py stage > st-ito_amd/csrc/comp_stage.inc"""
import sys

D = 32            # ring depth in blocks (compressor.hip: CB_D)
BUF = 100         # v100 .. v100 + 4 D - 1: ring
ZQ = [BUF + 4 * D, BUF + 4 * D + 4]   # two store quads (even bases)
T = ZQ[1] + 4     # t01 pair, t23 pair, m, m2
NREG = T + 6 - BUF
WAIT = D - 1 + D // 4 - 3   # all four loads of a group: the youngest allowed outstanding count

def pair(r): assert r % 2 == 0; return f"v[{r}:{r + 1}]"
def quad(r): return f"v[{r}:{r + 3}]"

def zsrc(reg):
    """(pair, op_sel text) broadcasting VGPR `reg` as both halves of src1."""
    if reg % 2 == 0:
        return pair(reg), "op_sel_hi:[1,0,1]"
    return pair(reg - 1), "op_sel:[0,1,0] op_sel_hi:[1,1,1]"

def ring_pass():
    L = []
    zreg = None  # None: z is %0
    for g in range(D // 4):
        zq = ZQ[g & 1]
        L.append(f"s_waitcnt vmcnt({WAIT})")
        for u in range(4):
            i = 4 * g + u
            b = BUF + 4 * i
            if zreg is None:
                L.append(f"v_mov_b32 v{T + 4}, %0")
                zreg = T + 4
            zp, sel = zsrc(zreg)
            L.append(f"v_pk_fma_f32 {pair(T)}, %1, {zp}, {pair(b)} {sel}")
            L.append(f"v_pk_fma_f32 {pair(T + 2)}, %2, {zp}, {pair(b + 2)} {sel}")
            L.append(f"v_max_f32 v{T + 4}, v{T}, v{T + 1}")              # one instruction after each v_pk_fma before its
            L.append(f"v_max3_f32 v{T + 4}, v{T + 4}, v{T + 2}, v{T + 3}")  # result is read (packed-result forwarding hazard)
            L.append(f"global_load_dwordx4 {quad(b)}, %3, off offset:{(D + i) * 64}")
            L.append("s_nop 0")
            L.append(f"v_max_f32_dpp v{T + 5}, v{T + 4}, v{T + 4} quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
            if u == 3 and g > 0:   # the previous group's states (its quad is not written again before the next group)
                L.append(f"global_store_dwordx4 %4, {quad(ZQ[(g - 1) & 1])}, off offset:{(g - 1) * 16}")
                L.append("s_nop 0")
            else:
                L.append("s_nop 1")
            L.append(f"v_max_f32_dpp v{zq + u}, v{T + 5}, v{T + 5} quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
            zreg = zq + u
    L.append(f"global_store_dwordx4 %4, {quad(ZQ[(D // 4 - 1) & 1])}, off offset:{(D // 4 - 1) * 16}")
    L.append(f"v_mov_b32 %0, v{zreg}")
    return L

def prologue():
    L = [f"global_load_dwordx4 {quad(BUF + 4 * i)}, %0, off offset:{i * 64}" for i in range(D)]
    # D / 4 stores into the pad behind the stream's states, so that the in-flight count matches a steady-state pass
    L += [f"v_mov_b32 v{ZQ[0] + u}, 0" for u in range(4)]
    L += [f"global_store_dwordx4 %1, {quad(ZQ[0])}, off offset:{g * 16}" for g in range(D // 4)]
    return L

# ---- mode "stage": the scan wave of k_comp_stage -- one segment of G blocks per asm statement, block functions out of LDS ----
G = 64            # blocks per segment (compressor.hip: CS_G)
DL = 8            # look-ahead in blocks: ds_read_b128 of block k + DL sits where the HBM ring's refill sat
SBUF = 40         # v40 .. v40 + 4 DL - 1: look-ahead ring; every register lives inside the one statement (clobbers say it all)
SZQ = [SBUF + 4 * DL, SBUF + 4 * DL + 4]
ST = SZQ[1] + 4
SNREG = ST + 6 - SBUF
ZOFF = 16         # bytes: state after block i of the segment at float 4 + i of the stream's state row, the incoming state at float 3

def stage_segment():
    """Operands: %0 = z (in/out), %1 = (S0, S1), %2 = (S2, S3), %3 = LDS byte address of this lane's quad of block 0,
    %4 = LDS byte address of the stream's state row.  LDS operations retire in issue order: `issued` counts them and
    every wait is the number issued after the youngest one it needs."""
    L, issued, idx = [], 0, {}
    L.append("ds_write_b32 %4, %0 offset:12")
    issued += 1
    for k in range(DL):
        L.append(f"ds_read_b128 {quad(SBUF + 4 * k)}, %3 offset:{k * 64}")
        idx[k] = issued
        issued += 1
    zreg = None
    for g in range(G // 4):
        zq = SZQ[g & 1]
        wait = issued - 1 - idx[4 * g + 3]
        assert 0 <= wait <= 15
        L.append(f"s_waitcnt lgkmcnt({wait})")
        for u in range(4):
            k = 4 * g + u
            b = SBUF + 4 * (k % DL)
            if zreg is None:
                L.append(f"v_mov_b32 v{ST + 4}, %0")
                zreg = ST + 4
            zp, sel = zsrc(zreg)
            L.append(f"v_pk_fma_f32 {pair(ST)}, %1, {zp}, {pair(b)} {sel}")
            L.append(f"v_pk_fma_f32 {pair(ST + 2)}, %2, {zp}, {pair(b + 2)} {sel}")
            L.append(f"v_max_f32 v{ST + 4}, v{ST}, v{ST + 1}")
            L.append(f"v_max3_f32 v{ST + 4}, v{ST + 4}, v{ST + 2}, v{ST + 3}")
            if k + DL < G:
                L.append(f"ds_read_b128 {quad(b)}, %3 offset:{(k + DL) * 64}")
                idx[k + DL] = issued
                issued += 1
                L.append("s_nop 0")
            else:
                L.append("s_nop 1")
            L.append(f"v_max_f32_dpp v{ST + 5}, v{ST + 4}, v{ST + 4} quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf")
            if u == 3 and g > 0:
                L.append(f"ds_write_b128 %4, {quad(SZQ[(g - 1) & 1])} offset:{ZOFF + (g - 1) * 16}")
                issued += 1
                L.append("s_nop 0")
            else:
                L.append("s_nop 1")
            L.append(f"v_max_f32_dpp v{zq + u}, v{ST + 5}, v{ST + 5} quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
            zreg = zq + u
    L.append(f"ds_write_b128 %4, {quad(SZQ[(G // 4 - 1) & 1])} offset:{ZOFF + (G // 4 - 1) * 16}")
    L.append(f"v_mov_b32 %0, v{zreg}")
    L.append("s_waitcnt lgkmcnt(0)")
    return L

K = 15            # samples per block (compressor.hip: CB_K)
XBUF = 40         # v40 .. v40 + 2 K - 1: the samples of both chains, step n at v[40 + 2 n : 41 + 2 n]
PP = XBUF + 2 * K  # two sets of (a, r) pairs for chain a and chain b: the set of step n + 1 is formed under step n
PT = PP + 8       # two pairs (c_att B + a, c_rel B + r); B lives in the high half

def stage_blockfn2():
    """The helpers' block-function recurrence for TWO units (2 x 4 blocks, one per 16-lane row) at once: per step and chain two
    v_mul_f32 ((a, r) = (sa |x|, sr |x|), off the chain), one v_pk_fma_f32 (lane j: c_att B_j + a for lane j + 1, c_rel B_j + r for
    itself) and one v_max_f32_dpp row_shr:1 (lane 0 of a row has no source lane and keeps c_rel B_0 + r = max(-inf, .)).  The two
    chains and the next step's products fill each other's hazard slots.  A row reads ONE float per step and chain from LDS (the
    sample, broadcast): the pairs themselves, 16 bytes a lane, made the LDS the kernel's limit.
    Operands: %0, %1 = B_0.. of chain a, b (out), %2 = (c_att, c_rel), %3 = sa, %4 = sr, %5 = B at the start (0 in lane 0 of a row, -inf
    elsewhere), %6 = LDS byte address of chain a's samples of this lane's row; chain b's sit 4 K floats behind."""
    L = [f"ds_read2_b32 {pair(XBUF + 2 * n)}, %6 offset0:{n} offset1:{4 * K + n}" for n in range(K)]
    L.append(f"v_mov_b32 v{PT + 1}, %5")
    L.append(f"v_mov_b32 v{PT + 3}, %5")
    hi = "op_sel:[0,1,0] op_sel_hi:[1,1,1]"
    def muls(n, chain):
        x, p = XBUF + 2 * n + chain, PP + 4 * (n & 1) + 2 * chain
        return [f"v_mul_f32_e64 v{p}, %3, |v{x}|", f"v_mul_f32_e64 v{p + 1}, %4, |v{x}|"]
    L.append(f"s_waitcnt lgkmcnt({K - 1})")
    L += muls(0, 0) + muls(0, 1)
    for n in range(K):
        p = PP + 4 * (n & 1)
        L.append(f"v_pk_fma_f32 {pair(PT)}, %2, {pair(PT)}, {pair(p)} {hi}")
        L.append(f"v_pk_fma_f32 {pair(PT + 2)}, %2, {pair(PT + 2)}, {pair(p + 2)} {hi}")
        if n + 1 < K:
            L.append(f"s_waitcnt lgkmcnt({K - 2 - n})")
            L += muls(n + 1, 0)
        else:
            L.append("s_nop 1")
        L.append(f"v_max_f32_dpp v{PT + 1}, v{PT}, v{PT + 1} row_shr:1 row_mask:0xf bank_mask:0xf")
        L.append(f"v_max_f32_dpp v{PT + 3}, v{PT + 2}, v{PT + 3} row_shr:1 row_mask:0xf bank_mask:0xf")
        if n + 1 < K:
            L += muls(n + 1, 1)
    L.append(f"v_mov_b32 %0, v{PT + 1}")
    L.append(f"v_mov_b32 %1, v{PT + 3}")
    return L

if sys.argv[1:] == ["stage"]:
    sclob = ", ".join(f'"v{r}"' for r in range(SBUF, SBUF + SNREG))
    f = sys.stdout
    f.write("// GENERATED by tools/gen/gen_comp_scan_asm.py stage -- do not edit.  k_comp_stage's scan wave: one segment of\n")
    f.write(f"// {G} block functions read from LDS {DL} blocks ahead (v{SBUF}-v{SBUF + 4 * DL - 1}), states written to LDS; no register outlives the statement.\n")
    f.write(f"#define STITO_COMP_STAGE_G {G}\n")
    f.write("#define STITO_COMP_STAGE_SEGMENT(z, s01, s23, fn_lds, z_lds) \\\n    asm volatile( \\\n")
    body = stage_segment()
    for l in body:
        f.write(f'        "{l}\\n\\t" \\\n')
    f.write(f'        : "+v"(z) : "v"(s01), "v"(s23), "v"(fn_lds), "v"(z_lds) : "memory", {sclob})\n')
    print(len(body), "instructions per segment of", G, "blocks =", len(body) / G, "per block", file=sys.stderr)
    pclob = ", ".join(f'"v{r}"' for r in range(XBUF, PT + 4))
    f.write("// the helper waves' recurrence, two units of four blocks at a time\n")
    f.write("#define STITO_COMP_STAGE_BLOCKFN2(b_a, b_b, c2, sa, sr, b_init, x_lds) \\\n    asm volatile( \\\n")
    body = stage_blockfn2()
    for l in body:
        f.write(f'        "{l}\\n\\t" \\\n')
    f.write(f'        : "=&v"(b_a), "=&v"(b_b) : "v"(c2), "v"(sa), "v"(sr), "v"(b_init), "v"(x_lds) : "memory", {pclob})\n')
    print(len(body), "instructions per two units of the block functions", file=sys.stderr)
    sys.exit(0)

clob = ", ".join(f'"v{r}"' for r in range(BUF, BUF + NREG))
f = sys.stdout
f.write("// GENERATED by tools/gen/gen_comp_scan_asm.py -- do not edit.  k_comp_blockscan's serial wave: register ring of\n")
f.write(f"// {D} block functions (v{BUF}-v{BUF + 4 * D - 1}), 9 instructions per block, one s_waitcnt vmcnt({WAIT}) per four blocks.\n")
f.write(f"#define STITO_COMP_SCAN_DEPTH {D}\n")
f.write("#define STITO_COMP_SCAN_PROLOGUE(src, pad) \\\n    asm volatile( \\\n")
for l in prologue():
    f.write(f'        "{l}\\n\\t" \\\n')
f.write(f'        : : "v"(src), "v"(pad) : "memory", {clob})\n')
f.write("#define STITO_COMP_SCAN_PASS(z, s01, s23, src, dst) \\\n    asm volatile( \\\n")
body = ring_pass()
for l in body:
    f.write(f'        "{l}\\n\\t" \\\n')
f.write(f'        : "+v"(z) : "v"(s01), "v"(s23), "v"(src), "v"(dst) : "memory", {clob})\n')
f.write("#define STITO_COMP_SCAN_DRAIN() asm volatile(\"s_waitcnt vmcnt(0)\" ::: \"memory\")\n")
print(len(body), "instructions per pass of", D, "blocks =", len(body) / D, "per block", file=sys.stderr)
