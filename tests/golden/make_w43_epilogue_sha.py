#!/usr/bin/env python
"""Records tests/golden/w43_epilogue_sha.json: per case the sha256 of the output map and of the per-stream output maxima of the
F(4x4,3x3) conv kernels that end in w43_epilogue (k_conv_wino43: algos 2 and 3, k_conv_wino43s: algo 4).  The epilogue's schedule
may change; its arithmetic may not, so the fixture is recorded with the library of the commit BEFORE such a change and the test
(tests/test_gpu_w43_epilogue_bits.py, which takes its cases and its runner from this file) holds the library after it to the same bits:

    tools/build_rev_lib.sh <parent rev> parent
    STITO_LIB_PATH=st-ito_amd/st_ito/_lib/ab/libstito_hip_parent.so python tests/golden/make_w43_epilogue_sha.py

Refuses to record when a shape is not covered by its algorithm or when two launches of a case differ.

The maxima: a library that exports stito_conv3x3_bn_relu_ws_amax hands out the kernel's own buffer, and the runner requires it
to equal the per-stream maximum of the map it just wrote (that is what the buffer is defined to hold: an atomic maximum over the
stored values, which does not depend on their order).  A library from before that entry point is recorded with the maximum of the
map in its place -- by the same definition the only value the buffer can have."""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "w43_epilogue_sha.json")

# (TTW, W, H, streams): every W leaves a partial last tile column (also of the pooled map), no H is a multiple of 4 and the odd
# ones leave a pool row over, and the tile rows of a stream (ceil(H / 4)) do not divide the 32 / TTW tile rows of a workgroup, so
# that a pixel block straddles two streams
SHAPES = [(8, 30, 9, 3), (4, 14, 10, 3), (2, 6, 5, 5), (1, 3, 7, 7)]


def cases():
    """Every tile-row width x (no pool, pool) x (f32 kernel: algo 2 with one and with two channel tiles; split kernel: algo 4),
    and algo 3 (the f32 kernel behind the hoisted transform) once per pool form."""
    out = []
    for ttw, W, H, S in SHAPES:
        for pool in (0, 1):
            for algo, cin, cout in ((2, 8, 64), (2, 8, 128), (4, 64, 256)):
                c = dict(algo=algo, S=S, H=H, W=W, cin=cin, cout=cout, pool=pool, ttw=ttw, zero_stream=None, big_stream=None)
                # one case per kernel with a stream of zeros (and no positive shift: its maximum is exactly 0), one with a stream
                # scaled by 1e3 (the split kernel: another power-of-two operand scale for that stream)
                if ttw == 8 and pool == 0 and cout != 128:
                    c["zero_stream"] = 1
                if ttw == 4 and pool == 1 and cout != 128:
                    c["big_stream"] = 2
                out.append(c)
    out.append(dict(algo=3, S=3, H=9, W=30, cin=64, cout=256, pool=0, ttw=8, zero_stream=None, big_stream=None))
    out.append(dict(algo=3, S=3, H=10, W=14, cin=64, cout=256, pool=1, ttw=4, zero_stream=None, big_stream=None))
    return out


def case_id(c):
    return f"algo{c['algo']}-ttw{c['ttw']}-{c['H']}x{c['W']}x{c['S']}-{c['cin']}to{c['cout']}-{'pool' if c['pool'] else 'nopool'}"


def inputs(c):
    """Seeded CPU generators: signed input, weights scaled to unit output variance, BN scale in [0.5, 1.5), shift of both signs."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(1000 * c["algo"] + 100 * c["ttw"] + 10 * c["pool"] + c["cout"] // 64)
    x = torch.randn((c["S"], c["cin"] // 8, c["H"], c["W"], 8), generator=g)
    w = torch.randn((c["cout"], c["cin"], 3, 3), generator=g) / (9 * c["cin"]) ** 0.5
    sc = 0.5 + torch.rand(c["cout"], generator=g)
    sh = 0.5 * torch.randn(c["cout"], generator=g)
    if c["zero_stream"] is not None:
        x[c["zero_stream"]] = 0.0
        sh = -sh.abs()
    if c["big_stream"] is not None:
        x[c["big_stream"]] *= 1e3
    return x, w, sc, sh


def amax_entry(L):
    try:
        fn = L.stito_conv3x3_bn_relu_ws_amax
    except AttributeError:
        return None
    c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
    fn.restype = c_int
    fn.argtypes = [c_void_p] * 5 + [c_int] * 7 + [c_void_p, ctypes.c_size_t, c_void_p, c_void_p]
    return fn


def run_case(c, launches=2):
    """-> (sha256 of the map, sha256 of the maxima, the maxima as int64 bit patterns); every launch must give the same bytes."""
    import numpy as np
    import torch
    from st_ito import _hip
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    st = _hip.stream_ptr()
    S, H, W, cin, cout, pool, algo = (c[k] for k in ("S", "H", "W", "cin", "cout", "pool", "algo"))
    assert L.stito_conv3x3_supported(S, H, W, cin, cout, pool, algo) == 1, f"{case_id(c)}: the shape is not covered by algorithm {algo}"
    x, w, sc, sh = (t.to(dev) for t in inputs(c))
    packed = torch.empty(L.stito_cnn14_packed_conv_floats(cout, cin, algo), device=dev)
    _hip.check(L.stito_cnn14_pack_conv(_hip.ptr(w), cout, cin, algo, _hip.ptr(packed), st))
    wsb = L.stito_conv3x3_workspace_bytes(S, H, W, cin, cout, pool, algo)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    with_amax = amax_entry(L)
    seen = []
    for _ in range(launches):
        ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device=dev)
        out = torch.full((S, cout // 8, Ho, Wo, 8), float("nan"), device=dev)   # a pixel the kernel leaves out stays NaN
        amax = torch.zeros(S, dtype=torch.int32, device=dev)
        args = (_hip.ptr(x), _hip.ptr(packed), _hip.ptr(sc), _hip.ptr(sh), _hip.ptr(out), S, H, W, cin, cout, pool, algo, _hip.ptr(ws), wsb, st)
        if with_amax is not None:
            _hip.check(with_amax(*args, _hip.ptr(amax)))
        else:
            _hip.check(L.stito_conv3x3_bn_relu_ws(*args))
        torch.cuda.synchronize()
        o = out.cpu()
        assert not torch.isnan(o).any(), f"{case_id(c)}: the kernel left output pixels unwritten"
        of_map = o.reshape(S, -1).max(dim=1).values.view(torch.int32)   # >= 0 after ReLU: bit patterns order like the values
        if with_amax is not None:
            assert torch.equal(amax.cpu(), of_map), f"{case_id(c)}: reported maxima {amax.cpu().tolist()} != maxima of the map {of_map.tolist()}"
        seen.append((o.numpy().tobytes(), of_map.numpy().astype(np.uint32).tobytes(), of_map.tolist()))
    for other in seen[1:]:
        assert other[0] == seen[0][0] and other[1] == seen[0][1], f"{case_id(c)}: two launches differ"
    return hashlib.sha256(seen[0][0]).hexdigest(), hashlib.sha256(seen[0][1]).hexdigest(), seen[0][2]


def main():
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd"))
    from st_ito import _hip
    fixture = {"library": os.path.basename(_hip.LIB_PATH), "cases": {}}
    for c in cases():
        sha_map, sha_amax, amax = run_case(c)
        if c["zero_stream"] is not None:
            assert amax[c["zero_stream"]] == 0, f"{case_id(c)}: the all-zero stream's maximum is {amax[c['zero_stream']]:#x}"
        fixture["cases"][case_id(c)] = {"out": sha_map, "amax": sha_amax}
    assert len(fixture["cases"]) == len(cases()), "two cases share an id"
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(fixture['cases'])} cases with {_hip.LIB_PATH} -> {FIXTURE}")


if __name__ == "__main__":
    main()
