"""Pins the answers of the workspace size queries whose layout the launchers share -- stito_render_workspace_bytes,
stito_lufs_workspace_bytes, stito_lufs_raw_workspace_bytes, stito_climb_workspace_bytes, stito_cnn14_workspace_bytes -- on the
host, without a GPU.  A region that moved or changed its size shows here; where the launchers' pointers land is pinned by the
guard tests of tests/test_gpu_parity.py.

The render cases are recorded with STITO_REVERB_SPLIT forced to 0 and to 1 (unset, the answer depends on the device's CU count);
the trunk cases use the algorithm ids that do not ask the device anything (direct, 3, 4, 5, 9; conv_block1 in two launches).

Record (on the commit whose answers are the reference): python tests/test_workspace_sizes.py"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "workspace_sizes.json")
FAKE_PTR = 0x100000   # never dereferenced: the queries read the descriptors, not what they point at

# ---- stito_render_workspace_bytes: chains as lists of (kind, aux_len) ----
NOISE_REVERB = 6
SINGLE = [[(k, 0)] for k in range(11) if k != NOISE_REVERB] + [[(NOISE_REVERB, taps)] for taps in (0, 2, 4100)]
BENCH = [(0, 0), (1, 0), (4, 0), (0, 0), (5, 0)]                 # ParametricEQ, Compressor, Reverb, ParametricEQ, Gain
ALL_REGIONS = [(1, 0), (4, 0), (NOISE_REVERB, 4100), (9, 0)]     # Compressor + Reverb + NoiseShapedReverb + dasp compressor
CHAINS = [[]] + SINGLE + [BENCH, ALL_REGIONS]
RENDER_SHAPES = [(1, 1), (3, 4099), (32, 262144), (256, 480000)]   # (pop, n_samples)

# ---- the loudness meter and the hill-climb: (n_items, channels, n_samples, n_blocks); the last rows must answer 0 ----
METER_SHAPES = [(n, c, L, nb) for n, L, nb in ((1, 19200, 1), (3, 4099, 2), (32, 480000, 97), (256, 480000, 97)) for c in (1, 2)]
METER_EMPTY = [(0, 2, 4099, 2), (3, 0, 4099, 2), (3, 2, 0, 2), (3, 2, 4099, 0), (-1, 2, 4099, 2), (3, 2, -5, 2)]

# ---- stito_cnn14_workspace_bytes ----
CHANNELS = [1, 64, 128, 256, 512, 1024, 2048]
TRUNK_ALGOS = {   # name -> per conv (algo, alt algo or None); None: no transformed weights (the direct kernel)
    "direct": [None] * 12,
    "3": [None] + [(3, None)] * 11,
    "4": [None] + [(4, None)] * 11,
    "5": [None] + [(5, None)] * 11,
    "9": [None] + [(9, None)] * 11,
    "mixed": [None, (3, None), (3, None), (4, None), (4, None), (5, None), (5, None), (9, 5), (9, 5), (9, 5), (9, 5), (9, None)],
}
TRUNK_SHAPES = [(2, 32), (3, 63), (64, 257), (512, 469)]   # (streams, n_frames)
TRUNK_CHUNKS = [(0, 0, 0), (2, 2, 5), (2, 4, 4)]           # (chunk_streams, first conv, last conv): none, a run of layers, one layer


def _chain(lib_mod, chain):
    descs = (lib_mod.FxDesc * max(1, len(chain)))()
    for d, (kind, aux_len) in zip(descs, chain):
        d.kind, d.num_channels, d.aux_len = kind, 2, aux_len
        d.aux_dev = FAKE_PTR if aux_len else None
    return descs


def _weights(lib_mod, algos, chunk):
    W = lib_mod.Cnn14Weights()
    W.embed_dim, W.n_mels = 512, 128
    for i, c in enumerate(CHANNELS):
        W.channels[i] = c
    for i, a in enumerate(algos):
        W.conv_w_dev[i] = W.bn_scale_dev[i] = W.bn_shift_dev[i] = FAKE_PTR
        if a is not None:
            W.conv_wino_dev[i], W.conv_wino_algo[i] = FAKE_PTR, a[0]
            if a[1] is not None:
                W.conv_alt_dev[i], W.conv_alt_algo[i] = FAKE_PTR, a[1]
    W.fc_mid_wt_dev = W.fc_mid_b_dev = W.fc_side_wt_dev = W.fc_side_b_dev = FAKE_PTR
    W.conv1_f2reg_w_dev = None   # conv_block1 in one launch asks the device for its LDS size
    W.chunk_streams, W.chunk_first_conv, W.chunk_last_conv = chunk
    return W


def _answers():
    """Every case as [query, arguments, bytes], in a fixed order."""
    from st_ito import _hip
    lib = _hip.lib()
    rows = []
    saved = os.environ.get("STITO_REVERB_SPLIT")
    try:
        for split in ("0", "1"):
            os.environ["STITO_REVERB_SPLIT"] = split
            for chain in CHAINS:
                descs = _chain(_hip, chain)
                for pop, n in RENDER_SHAPES:
                    rows.append(["render", [[list(fx) for fx in chain], pop, n, split],
                                 int(lib.stito_render_workspace_bytes(descs, len(chain), 1, n, pop))])
    finally:
        if saved is None:
            del os.environ["STITO_REVERB_SPLIT"]
        else:
            os.environ["STITO_REVERB_SPLIT"] = saved
    for n, c, L, nb in METER_SHAPES + METER_EMPTY:
        rows.append(["lufs", [n, L, nb], int(lib.stito_lufs_workspace_bytes(n, L, nb))])
        rows.append(["lufs_raw", [n, c, L, nb], int(lib.stito_lufs_raw_workspace_bytes(n, c, L, nb))])
        rows.append(["climb", [n, c, L, nb], int(lib.stito_climb_workspace_bytes(n, c, L, nb))])
    for name, algos in TRUNK_ALGOS.items():
        for chunk in TRUNK_CHUNKS:
            W = _weights(_hip, algos, chunk)
            for S, T in TRUNK_SHAPES:
                rows.append(["cnn14", [name, list(chunk), S, T], int(lib.stito_cnn14_workspace_bytes(ctypes.byref(W), S, T))])
    return rows


def test_workspace_sizes_are_the_recorded_ones():
    with open(FIXTURE) as f:
        ref = json.load(f)
    got = _answers()
    assert [r[:2] for r in got] == [r[:2] for r in ref], "the fixture does not hold the cases of this file: record it again"
    for g, r in zip(got, ref):
        assert g[2] == r[2], (g[0], g[1], g[2], r[2])
    for q, args, nbytes in ref:   # an empty argument of a meter query answers 0; everything else is whole 256-byte regions
        if q in ("lufs", "lufs_raw", "climb") and min(args) <= 0:
            assert nbytes == 0, (q, args)
        else:
            assert nbytes > 0 and nbytes % 256 == 0, (q, args, nbytes)


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), d) for d in ("st-ito_amd", "oracle")]
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in _answers()) + "\n]\n")
    print(path, os.path.getsize(path), "bytes")
