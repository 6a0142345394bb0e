"""GPU: the six-sweep F(4x4,3x3) conv kernel (csrc/conv_wino43.hip: k_conv_wino43s3 = algorithm 9) gives, bit for bit, the output
maps and per-stream output maxima recorded in tests/golden/w43s3_epilogue_sha.json with the library of the commit before its row
epilogues were rewritten (scratch-area and output addresses formed in the epilogue instead of ahead of the first sweep; row 5 reads
its stored values back by half output groups, the next one issued ahead; the stream maxima reported once per tile panel).  That
decides where an address comes from, how many loads are in flight and what a wait covers; every product, every add of
Y = A^T M A, BN, ReLU, the pool and the maxima keeps its operands and its order, so nothing may move by an ulp -- and a slab read
before it has landed, a partial read before it was stored or from the wrong slot, would move a lot.

Cases and runner: tests/golden/make_w43s3_epilogue_sha.py (64 and 128 input channels = 8 and 16 periods per sweep, every tile-row
width, pooled and not, one and three streams with partial pixel-block quads and an odd last row, one workgroup per item and one per
sweep).  No case is skipped: a shape the algorithm does not cover fails."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_w43s3_epilogue_sha", os.path.join(ROOT, "tests", "golden", "make_w43s3_epilogue_sha.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = gen.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(gen.FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_covers_the_matrix(recorded):
    """(no GPU) the recorded file is the case table's: every id once, and the table is the matrix the sweep boundaries need"""
    assert sorted(recorded) == sorted(gen.case_id(c) for c in CASES)
    cells = {(c["ttw"], c["W"], c["pool"], c["cin"], c["S"], c["swsplit"]) for c in CASES}
    assert cells == {(t, 4 * t, p, ci, s, sw) for t in (1, 2, 4, 8) for p in (0, 1) for ci in (64, 128) for s in (1, 3) for sw in (0, 1)}
    for c in CASES:
        assert c["H"] % 2 == 1 and c["H"] % 4 == 1, c                                      # an odd last row, pooled or not
        assert gen.pixel_blocks(c) % 4 != 0 and (c["S"] == 1 or gen.pixel_blocks(c) > 4), c   # a partial quad; a second item with three streams
    assert gen.case_id(gen.REPEAT_CASE) in recorded


def test_split_and_whole_items_were_recorded_with_the_same_bits(recorded):
    """(no GPU) one workgroup per item and one per sweep do the same arithmetic: the parent's library gave both the same hashes"""
    for c in CASES:
        if c["swsplit"] == 0:
            assert recorded[gen.case_id(c)] == recorded[gen.case_id(dict(c, swsplit=1))], c


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[gen.case_id(c) for c in CASES])
def test_bits_are_the_recorded_ones(c, recorded):
    import torch
    assert torch.cuda.is_available()
    sha_map, sha_amax = gen.run_case(c)
    want = recorded[gen.case_id(c)]
    print(f"{gen.case_id(c)}: map {sha_map[:16]} (recorded {want['out'][:16]})  maxima {sha_amax[:16]} (recorded {want['amax'][:16]})")
    assert sha_map == want["out"], "the output map differs from the recorded bits"
    assert sha_amax == want["amax"], "the per-stream maxima differ from the recorded bits"


@pytest.mark.gpu
def test_ten_launches_into_the_same_buffers_give_the_recorded_bits(recorded):
    """A repeat-launch check of a fixed result: the partial outputs of launch n are overwritten by launch n + 1 in the same scratch
    area, so a row-5 read that ran ahead of its row's stores would return the previous launch's -- equal -- values here and is
    caught by the cases above on fresh buffers; what this catches is state that survives a launch (the workspace, the maxima)."""
    import torch
    assert torch.cuda.is_available()
    c = gen.REPEAT_CASE
    sha_map, sha_amax = gen.run_case(c, launches=10, same_buffers=True)
    want = recorded[gen.case_id(c)]
    print(f"{gen.case_id(c)} x 10: map {sha_map[:16]} (recorded {want['out'][:16]})  maxima {sha_amax[:16]} (recorded {want['amax'][:16]})")
    assert sha_map == want["out"] and sha_amax == want["amax"]
