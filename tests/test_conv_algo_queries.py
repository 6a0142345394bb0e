"""Pins the 3x3-conv query surface per algorithm id: stito_conv3x3_supported / _workspace_bytes / _issued_flops and
stito_cnn14_packed_conv_floats for ids -1 .. 10 (retired and unknown ids included) on the parity-test and Cnn14 shapes, and the
status code and error text of every call that is refused before anything is enqueued.  The register-resident F(2x2,3x3) kernel
(id 8) asks the device whether its LDS fits, so there is one fixture recorded without a GPU and one on the MI355X.

Record (on the commit whose answers are the reference): python tests/test_conv_algo_queries.py [--gpu]"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = list(range(-1, 11))
WS_IDS = (3, 4, 5, 8, 9)
CALLS = ("stito_conv3x3_bn_relu", "stito_conv3x3_bn_relu_ws", "stito_cnn14_pack_conv")   # fixture: index into this
FAKE_PTR = 0x100000   # never dereferenced: every call below is refused before it touches memory or enqueues work


def _fixture(gpu):
    return os.path.join(HERE, "conv_algo_queries_gpu.json" if gpu else "conv_algo_queries_cpu.json")


def _shapes():
    sys.path.insert(0, HERE)
    from test_gpu_parity import CONV_CASES, RACE_CASES
    shapes = {(H, W, cin, cout, pool): {n} for n, H, W, cin, cout, pool in CONV_CASES}
    for H, W, cin, cout, pool, _ in RACE_CASES:
        shapes.setdefault((H, W, cin, cout, pool), set())
    chans = [1, 64, 128, 256, 512, 1024, 2048]
    for T in (469, 94):   # the bench input (48 kHz, 10 s, hop 1024) and 2 s
        H, W = T, 128
        for b in range(6):
            for j in range(2):
                shapes.setdefault((H, W, chans[b] if j == 0 else chans[b + 1], chans[b + 1], int(j == 1 and b < 5)), set())
            if b < 5:
                H, W = H // 2, W // 2
    return [(n,) + s for s, ns in sorted(shapes.items()) for n in sorted(ns | {1, 64, 512})]


def _num(x):
    return int(x) if float(x).is_integer() else x


def _status_calls(rows, lib):
    """(function, args) of the calls the library refuses up front: the non-workspace entry with a workspace algorithm, the
    retired ids, a workspace one byte short (or none for an unsupported shape), packings of channel counts the kernel lacks."""
    calls = []
    for n, H, W, cin, cout, pool in rows:
        if n != 64:   # the batch only changes the numbers in the texts
            continue
        for a in WS_IDS:
            calls.append(("stito_conv3x3_bn_relu", (n, H, W, cin, cout, pool, a)))
            need = lib.stito_conv3x3_workspace_bytes(n, H, W, cin, cout, pool, a)
            calls.append(("stito_conv3x3_bn_relu_ws", (n, H, W, cin, cout, pool, a, max(int(need) - 1, 0))))
        for a in (6, 7):
            calls.append(("stito_conv3x3_bn_relu_ws", (n, H, W, cin, cout, pool, a, 1 << 30)))
    calls.append(("stito_conv3x3_bn_relu", (0, 8, 8, 64, 64, 0, 0)))
    packs = set()
    for _, _, _, cin, cout, _ in rows:
        for a in (1, 2, 3, 4, 5, 6, 7, 8, 9):
            refused = {1: cin % 8 or cout % 64, 2: cin % 8 or cout % 64, 3: cin % 8 or cout % 64, 4: cin % 64 or cout % 64,
                       5: cin % 64 or cout % 64, 6: True, 7: True, 8: cin != 64 or cout % 64, 9: cin % 64 or cout % 128}[a]
            if refused:
                packs.add((cout, cin, a))
    calls += [("stito_cnn14_pack_conv", p) for p in sorted(packs)]
    return calls


def _call(lib, fn, args):
    P = FAKE_PTR
    fn = CALLS[fn] if isinstance(fn, int) else fn
    if fn == "stito_conv3x3_bn_relu":
        rc = lib.stito_conv3x3_bn_relu(P, P, P, P, P, *args, None)
    elif fn == "stito_conv3x3_bn_relu_ws":
        rc = lib.stito_conv3x3_bn_relu_ws(P, P, P, P, P, *args[:7], P, args[7], None)
    else:
        cout, cin, a = args
        rc = lib.stito_cnn14_pack_conv(P, cout, cin, a, P, None)
    return rc, lib.stito_last_error().decode()


def _record(lib):
    rows = _shapes()
    out = {"ids": IDS, "rows": [], "packed": [], "status": [], "messages": []}
    for r in rows:
        sup = [lib.stito_conv3x3_supported(*r, a) for a in IDS]
        ws = [int(lib.stito_conv3x3_workspace_bytes(*r, a)) for a in IDS]
        fl = [_num(lib.stito_conv3x3_issued_flops(*r, a)) for a in IDS]
        out["rows"].append([list(r), sup, ws, fl])
    for cout, cin in sorted({(r[4], r[3]) for r in rows}):
        out["packed"].append([cout, cin, [int(lib.stito_cnn14_packed_conv_floats(cout, cin, a)) for a in IDS]])
    for fn, args in _status_calls(rows, lib):
        rc, msg = _call(lib, fn, args)
        assert rc < 0 and rc != -4, (fn, args, rc, msg)   # refused by the library itself, not after a HIP call
        if msg not in out["messages"]:
            out["messages"].append(msg)
        out["status"].append([CALLS.index(fn), list(args), rc, out["messages"].index(msg)])
    return out


def _check(gpu):
    from st_ito import _hip
    lib = _hip.lib()
    with open(_fixture(gpu)) as f:
        ref = json.load(f)
    assert ref["ids"] == IDS
    for r, sup, ws, fl in ref["rows"]:
        assert [lib.stito_conv3x3_supported(*r, a) for a in IDS] == sup, r
        assert [int(lib.stito_conv3x3_workspace_bytes(*r, a)) for a in IDS] == ws, r
        assert [_num(lib.stito_conv3x3_issued_flops(*r, a)) for a in IDS] == fl, r
    for cout, cin, v in ref["packed"]:
        assert [int(lib.stito_cnn14_packed_conv_floats(cout, cin, a)) for a in IDS] == v, (cout, cin)
    for fn, args, rc, msg in ref["status"]:
        assert list(_call(lib, fn, tuple(args))) == [rc, ref["messages"][msg]], (CALLS[fn], args)


def test_conv_algo_queries():
    import torch
    _check(torch.cuda.is_available())   # id 8 answers as the host's device (or its absence) lets it


@pytest.mark.gpu
def test_conv_algo_queries_mi355x():
    _check(True)


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), d) for d in ("st-ito_amd", "oracle")]
    from st_ito import _hip
    gpu = "--gpu" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else _fixture(gpu)
    with open(path, "w") as f:
        json.dump(_record(_hip.lib()), f, separators=(",", ":"))
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")
