"""GPU: the F(4x4,3x3) conv kernels that end in w43_epilogue (csrc/conv_wino43.hip: k_conv_wino43 = algos 2 and 3, k_conv_wino43s =
algo 4) give, bit for bit, the output maps and per-stream output maxima recorded in tests/golden/w43_epilogue_sha.json with the
library of the commit before the epilogue's exchange was rescheduled (three positions of every wave pair per pass, stored with
ds_write_addtid_b32, instead of the position rows {1,2}, {3,4}, {0,5}).  The schedule decides which positions travel through LDS in
which pass and where they lie there; every add, subtract and fma of Y = A^T M A, BN, ReLU, the pool and the maxima keeps its operands
and its order, so nothing may move by an ulp.

Cases and runner: tests/golden/make_w43_epilogue_sha.py (every tile-row width x pool form x kernel, partial tile columns, pool rows
left over, pixel blocks that straddle streams, a second channel tile, an all-zero stream, a stream scaled by 1e3).  No case is
skipped: a shape its algorithm does not cover fails."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_w43_epilogue_sha", os.path.join(ROOT, "tests", "golden", "make_w43_epilogue_sha.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = gen.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(gen.FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_covers_the_matrix(recorded):
    """(no GPU) the recorded file is the case table's: every id once, and the table is the coverage matrix the kernels need"""
    assert sorted(recorded) == sorted(gen.case_id(c) for c in CASES)
    cells = {(c["ttw"], c["pool"], c["algo"]) for c in CASES}
    assert {(t, p, a) for t in (8, 4, 2, 1) for p in (0, 1) for a in (2, 4)} <= cells
    assert {(c["pool"]) for c in CASES if c["algo"] == 3} == {0, 1}
    assert any(c["algo"] == 2 and c["cout"] == 128 for c in CASES)
    for algo in (2, 4):
        assert any(c["algo"] == algo and c["zero_stream"] is not None for c in CASES)
        assert any(c["algo"] == algo and c["big_stream"] is not None for c in CASES)
    for c in CASES:
        assert c["W"] % 4 != 0 and (c["W"] // 2) % 2 == 1 and c["H"] % 4 != 0, c   # partial tile column, pooled or not; partial tile row


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[gen.case_id(c) for c in CASES])
def test_bits_are_the_recorded_ones(c, recorded):
    import torch
    assert torch.cuda.is_available()
    from st_ito import _hip
    assert gen.amax_entry(_hip.lib()) is not None, "stito_conv3x3_bn_relu_ws_amax is not exported: the kernel's own maxima cannot be read"
    sha_map, sha_amax, amax = gen.run_case(c)
    want = recorded[gen.case_id(c)]
    print(f"{gen.case_id(c)}: map {sha_map[:16]} (recorded {want['out'][:16]})  maxima {sha_amax[:16]} (recorded {want['amax'][:16]})")
    if c["zero_stream"] is not None:
        assert amax[c["zero_stream"]] == 0, "the all-zero stream's maximum"
    assert sha_map == want["out"], "the output map differs from the recorded bits"
    assert sha_amax == want["amax"], "the per-stream maxima differ from the recorded bits"
