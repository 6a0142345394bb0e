#!/usr/bin/env python
"""Records tests/golden/w43s3_epilogue_sha.json: per case the sha256 of the output map and of the per-stream output maxima of the
six-sweep F(4x4,3x3) conv kernel (k_conv_wino43s3, algorithm 9).  How its row epilogues are scheduled -- which vmcnt(0) a slab's
landing waits behind, where the addresses come from, how many of row 5's stored values are in flight -- may change; its arithmetic may not, so the
fixture is recorded with the library of the commit BEFORE such a change and the test (tests/test_gpu_w43s3_epilogue_bits.py, which
takes its cases and its runner from this file) holds the library after it to the same bits:

    tools/build_rev_lib.sh <parent rev> parent
    STITO_LIB_PATH=st-ito_amd/st_ito/_lib/ab/libstito_hip_parent.so python tests/golden/make_w43s3_epilogue_sha.py

Refuses to record when a shape is not covered by the algorithm or when two launches of a case differ.  The maxima come from the
kernel's own buffer (stito_conv3x3_bn_relu_ws_amax) and must equal the per-stream maximum of the map just written."""
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURE = os.path.join(ROOT, "tests", "golden", "w43s3_epilogue_sha.json")
ALGO = 9       # the six-sweep kernel
COUT = 512     # four 128-channel tiles
SWSPLIT_ENV = "STITO_W43S3_SWSPLIT"

_spec = importlib.util.spec_from_file_location("make_w43_epilogue_sha", os.path.join(ROOT, "tests", "golden", "make_w43_epilogue_sha.py"))
_w43 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_w43)
amax_entry = _w43.amax_entry

# (TTW, W, H): a workgroup item is a QUAD of pixel blocks of 32 tiles (32 / TTW tile rows of TTW tiles).  Every H is odd with H % 4 == 1:
# the last tile row holds one map row and the pooled map leaves a row over; ceil(H / 4) tile rows per stream make 2 pixel blocks with
# one stream and 5 with three -- a partial quad either way, and a second item with three streams.
SHAPES = [(8, 32, 21), (4, 16, 45), (2, 8, 93), (1, 4, 173)]
REPEAT_CASE = dict(S=3, H=21, W=32, cin=64, pool=1, ttw=8, swsplit=0)   # launched ten times into the same buffers


def cases():
    """Every tile-row width x (no pool, pool) x (64 input channels = eight periods per sweep, the shortest; 128) x (1, 3 streams)
    x (one workgroup per item, one per sweep)."""
    return [dict(S=S, H=H, W=W, cin=cin, pool=pool, ttw=ttw, swsplit=sw)
            for ttw, W, H in SHAPES for pool in (0, 1) for cin in (64, 128) for S in (1, 3) for sw in (0, 1)]


def case_id(c):
    return f"ttw{c['ttw']}-{c['H']}x{c['W']}x{c['S']}-{c['cin']}to{COUT}-{'pool' if c['pool'] else 'nopool'}-swsplit{c['swsplit']}"


def pixel_blocks(c):
    tth = 32 // c["ttw"]
    tile_rows = c["S"] * ((c["H"] + 3) // 4)
    return (tile_rows + tth - 1) // tth * ((c["W"] // 4 + c["ttw"] - 1) // c["ttw"])


def inputs(c):
    """Seeded CPU generators (the seed leaves the sweep split out: both forms get the same data): signed input, one stream scaled by
    300 where there are three, weights scaled to unit output variance, BN scale in [0.5, 1.5), shift of both signs."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(9000 + 100 * c["ttw"] + 10 * c["pool"] + c["cin"] // 64 + 1000 * c["S"])
    x = torch.randn((c["S"], c["cin"] // 8, c["H"], c["W"], 8), generator=g)
    w = torch.randn((COUT, c["cin"], 3, 3), generator=g) / (9 * c["cin"]) ** 0.5
    sc = 0.5 + torch.rand(COUT, generator=g)
    sh = 0.5 * torch.randn(COUT, generator=g)
    if c["S"] > 1:
        x[1] *= 300.0
    return x, w, sc, sh


def run_case(c, launches=2, same_buffers=False):
    """-> (sha256 of the map, sha256 of the maxima); every launch must give the same bytes.  same_buffers: all launches write
    one output map, one workspace and one maxima buffer (zeroed between launches, as the trunk does)."""
    import numpy as np
    import torch
    from st_ito import _hip
    L = _hip.lib()
    dev = torch.device("cuda", 0)
    st = _hip.stream_ptr()
    S, H, W, cin, pool = (c[k] for k in ("S", "H", "W", "cin", "pool"))
    assert L.stito_conv3x3_supported(S, H, W, cin, COUT, pool, ALGO) == 1, f"{case_id(c)}: the shape is not covered by algorithm {ALGO}"
    with_amax = amax_entry(L)
    assert with_amax is not None, "stito_conv3x3_bn_relu_ws_amax is not exported: the kernel's own maxima cannot be read"
    x, w, sc, sh = (t.to(dev) for t in inputs(c))
    packed = torch.empty(L.stito_cnn14_packed_conv_floats(COUT, cin, ALGO), device=dev)
    _hip.check(L.stito_cnn14_pack_conv(_hip.ptr(w), COUT, cin, ALGO, _hip.ptr(packed), st))
    wsb = L.stito_conv3x3_workspace_bytes(S, H, W, cin, COUT, pool, ALGO)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    seen = []
    before = os.environ.get(SWSPLIT_ENV)
    os.environ[SWSPLIT_ENV] = str(c["swsplit"])   # (the library reads it per launch)
    try:
        ws = out = amax = None
        for i in range(launches):
            if i == 0 or not same_buffers:
                ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device=dev)
                out = torch.full((S, COUT // 8, Ho, Wo, 8), float("nan"), device=dev)   # a pixel the kernel leaves out stays NaN
                amax = torch.zeros(S, dtype=torch.int32, device=dev)
            else:
                amax.zero_()
            _hip.check(with_amax(_hip.ptr(x), _hip.ptr(packed), _hip.ptr(sc), _hip.ptr(sh), _hip.ptr(out), S, H, W, cin, COUT, pool, ALGO,
                                 _hip.ptr(ws), wsb, st, _hip.ptr(amax)))
            torch.cuda.synchronize()
            o = out.cpu()
            assert not torch.isnan(o).any(), f"{case_id(c)}: the kernel left output pixels unwritten"
            of_map = o.reshape(S, -1).max(dim=1).values.view(torch.int32)   # >= 0 after ReLU: bit patterns order like the values
            assert torch.equal(amax.cpu(), of_map), f"{case_id(c)}: reported maxima {amax.cpu().tolist()} != maxima of the map {of_map.tolist()}"
            seen.append((hashlib.sha256(o.numpy().tobytes()).hexdigest(), hashlib.sha256(of_map.numpy().astype(np.uint32).tobytes()).hexdigest()))
    finally:
        if before is None:
            del os.environ[SWSPLIT_ENV]
        else:
            os.environ[SWSPLIT_ENV] = before
    for i, other in enumerate(seen[1:]):
        assert other == seen[0], f"{case_id(c)}: launch {i + 2} differs from the first"
    return seen[0]


def main():
    sys.path.insert(0, os.path.join(ROOT, "st-ito_amd"))
    from st_ito import _hip
    fixture = {"library": os.path.basename(_hip.LIB_PATH), "cases": {}}
    for c in cases():
        sha_map, sha_amax = run_case(c)
        fixture["cases"][case_id(c)] = {"out": sha_map, "amax": sha_amax}
    assert len(fixture["cases"]) == len(cases()), "two cases share an id"
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(fixture['cases'])} cases with {_hip.LIB_PATH} -> {FIXTURE}")


if __name__ == "__main__":
    main()
