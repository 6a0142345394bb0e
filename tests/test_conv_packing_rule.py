"""The packing rule of the Cnn14 trunk (st_ito.models.panns.conv_packing) as literal tables: which Winograd
packing, and which alternative one, Cnn14.prepare() makes for a cin -> cout layer under the knobs -- on the host, without a
GPU, a model or (but for the last test) the library.  conv_block1_fused is the condition for conv_block1 in one launch.

Ids: 1 F(2x2) float32, 2 F(4x4), 3 F(4x4) hoisted transform, 4 split, 5 two sweeps, 8 register-resident F(2x2), 9 six sweeps;
"-": the direct kernel's packing only; "9/5": id 9 with the alternative 5."""
import pytest

from st_ito import _hip
from st_ito.models.panns import conv_block1_fused, conv_knobs, conv_packing

CHANS = (1, 64, 128, 256, 512, 1024, 2048)
PAIRS = [(CHANS[i // 2 + i % 2], CHANS[i // 2 + 1]) for i in range(12)]   # conv 0 .. 11: 1->64, 64->64, 64->128, 128->128, ...

TABLE = [   # (knobs changed from the defaults, convs 0 .. 11)
    ({}, "- 8 8 2 4 4 4 9/5 9/5 9/5 9/5 9/5"),
    (dict(conv_algo=_hip.CONV_DIRECT), "- - - - - - - - - - - -"),
    (dict(conv_algo=_hip.CONV_WINOGRAD), "- 1 1 1 1 1 1 1 1 1 1 1"),
    (dict(conv_split=False), "- 2 2 2 2 2 3 3 3 3 3 3"),
    (dict(conv_split=False, conv_pre_min_cout=0), "- 2 2 2 2 2 2 2 2 2 2 2"),
    (dict(conv_f2reg=False), "- 2 2 2 4 4 4 9/5 9/5 9/5 9/5 9/5"),
    (dict(conv_split3_min_cin=0), "- 8 8 2 4 4 4 5 5 5 5 5"),
    (dict(conv_split3_min_cin=0, conv_split2_min_cin=0), "- 8 8 2 4 4 4 4 4 4 4 4"),
    (dict(conv_split_min_cout=512), "- 8 8 2 2 2 4 9/5 9/5 9/5 9/5 9/5"),
    (dict(conv_split_min_cout=0), "- 8 8 2 2 2 3 3 3 3 3 3"),
    # the remaining schedules of tests/test_gpu_trunk_edges.py: neither knob is part of the packing rule
    (dict(conv_fuse1=False), "- 8 8 2 4 4 4 9/5 9/5 9/5 9/5 9/5"),
]
OUTSIDE = [   # pairs that are not the model's, under the defaults
    (12, 64, "-"), (64, 96, "-"), (96, 256, "2"), (64, 256, "8"),
    (512, 768, "5"),      # cout % 512 != 0: two sweeps, and nothing to be the alternative of
    (512, 1280, "3"),     # cout >= 1024 and not a multiple of 512: no split kernel covers it
]


def _knobs(**changed):
    k = conv_knobs({})   # the defaults, whatever STITO_* the environment holds
    for name, v in changed.items():
        assert hasattr(k, name), name
        setattr(k, name, v)
    return k


def _show(packing):
    algo, alt = packing
    return "-" if algo is None else str(algo) + ("" if alt is None else f"/{alt}")


def test_ids():
    assert (_hip.CONV_DIRECT, _hip.CONV_WINOGRAD, _hip.CONV_WINOGRAD_F4, _hip.CONV_WINOGRAD_F4_PRE, _hip.CONV_WINOGRAD_F4_SPLIT,
            _hip.CONV_WINOGRAD_F4_SPLIT2, _hip.CONV_WINOGRAD_F2_REG, _hip.CONV_WINOGRAD_F4_SPLIT3) == (0, 1, 2, 3, 4, 5, 8, 9)
    assert len(PAIRS) == 12 and PAIRS[:4] == [(1, 64), (64, 64), (64, 128), (128, 128)] and PAIRS[10:] == [(1024, 2048), (2048, 2048)]


@pytest.mark.parametrize("changed,row", TABLE, ids=[",".join(f"{k}={int(v)}" for k, v in c.items()) or "defaults" for c, _ in TABLE])
def test_model_layers(changed, row):
    k = _knobs(**changed)
    assert " ".join(_show(conv_packing(cin, cout, k)) for cin, cout in PAIRS) == row


@pytest.mark.parametrize("cin,cout,want", OUTSIDE)
def test_pairs_outside_the_model(cin, cout, want):
    assert _show(conv_packing(cin, cout, _knobs())) == want


def test_an_alternative_rides_only_with_six_sweeps():
    """Over every knob row and a grid of channel pairs: the alternative is the two-sweep packing, and only id 9 has one."""
    for changed, _ in TABLE:
        k = _knobs(**changed)
        for cin in (1, 8, 12, 64, 96, 128, 256, 512, 1024, 2048):
            for cout in (64, 96, 128, 256, 512, 768, 1024, 1280, 1536, 2048):
                algo, alt = conv_packing(cin, cout, k)
                assert (alt is not None) == (algo == _hip.CONV_WINOGRAD_F4_SPLIT3), (changed, cin, cout)
                assert alt in (None, _hip.CONV_WINOGRAD_F4_SPLIT2)


def _fused(k, conv1_shape=(64, 1, 3, 3)):
    return conv_block1_fused(k, conv1_shape, conv_packing(64, 64, k)[0])   # as prepare() asks: conv_block1.conv2 is 64 -> 64


def test_conv_block1_in_one_launch():
    assert _fused(_knobs()) is True
    assert _fused(_knobs(conv_fuse1=False)) is False
    assert _fused(_knobs(conv_f2reg=False)) is False
    for changed in (dict(conv_algo=_hip.CONV_DIRECT), dict(conv_algo=_hip.CONV_WINOGRAD), dict(conv_split=False)):
        assert _fused(_knobs(**changed)) is False, changed   # conv_block1.conv2 is then not on the register-resident kernel
    assert _fused(_knobs(), (128, 1, 3, 3)) is False and _fused(_knobs(), (64, 8, 3, 3)) is False   # the kernel's first conv is 1 -> 64
    assert conv_block1_fused(_knobs(), (64, 1, 3, 3), None) is False   # nothing packed for conv_block1.conv2


def test_the_environment_sets_the_knobs():
    """The variable names and what they parse to; an empty environment gives the defaults the tables above are stated under."""
    assert vars(conv_knobs({})) == dict(conv_algo=_hip.CONV_WINOGRAD_F4, conv_pre_min_cout=512, conv_split=True, conv_split_min_cout=256,
                                        conv_split2_min_cin=512, conv_split3_min_cin=512, conv_f2reg=True, conv_fuse1=True)
    env = dict(STITO_CONV_ALGO="winograd", STITO_CONV_PRE_MIN_COUT="0", STITO_CONV_SPLIT="0", STITO_CONV_SPLIT_MIN_COUT="512",
               STITO_CONV_SPLIT2_MIN_CIN="1024", STITO_CONV_SPLIT3_MIN_CIN="0", STITO_CONV_F2REG="0", STITO_CONV_FUSE1="0")
    assert vars(conv_knobs(env)) == dict(conv_algo=_hip.CONV_WINOGRAD, conv_pre_min_cout=0, conv_split=False, conv_split_min_cout=512,
                                         conv_split2_min_cin=1024, conv_split3_min_cin=0, conv_f2reg=False, conv_fuse1=False)


def test_six_sweeps_cover_what_two_sweeps_cover_on_the_model_layers():
    """The launch rule (cnn14_choice in csrc/cnn14.hip) hands a layer its input's per-stream maxima exactly when the kernel it picks
    reads them.  Reading the raw id instead, as the trunk did before, differs only where id 9 does not cover a shape that its
    alternative id 5 covers; for the channel pairs prepare() gives 9 / 5 there is no such shape (this one needs the library, on
    the host): convs 7 .. 11, with and without pooling, 1 to 64 streams, maps from 64 x 64 down to 1 x 1 (every height; the
    widths a mel count halves to, and odd ones).  With every width 1 .. 64 and every stream count 1 .. 64 the same loop makes
    2 621 440 calls in 16 s and finds none either (profiles/trunk_choice_refactor_ab.txt)."""
    supported = _hip.lib().stito_conv3x3_supported
    for cin, cout in PAIRS[7:]:
        for pool in (0, 1):
            for n in (1, 2, 18, 64):
                for H in range(1, 65):
                    for W in (1, 2, 3, 4, 5, 8, 16, 33, 64):
                        assert supported(n, H, W, cin, cout, pool, 9) == supported(n, H, W, cin, cout, pool, 5), (n, H, W, cin, cout, pool)
