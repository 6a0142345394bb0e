"""CPU tests of the FX-Encoder's host side: the float64 restatement against the reference's recorded output, the state-dict key
map, the batch-norm fold, the weight packing rule, the length rule and the constructor's contract."""
import math
import os

import numpy as np
import pytest
import torch

import fx_encoder_ref64 as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fx_encoder_toy.npz")


def load_golden():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd:")}
    return z, sd


def test_ref64_reproduces_the_reference_output():
    z, sd = load_golden()
    blocks = R.blocks_from_state_dict(sd, z["strides"])
    y = R.stack(torch.from_numpy(z["x"]), blocks)
    assert y.shape == (3, 64) and z["x"].shape == (3, 2, 211)
    assert float((y - torch.from_numpy(z["y"])).abs().max()) < 1e-12


def test_load_state_dict_maps_every_golden_key():
    from st_ito.models.fx_encoder import FXencoder
    z, sd = load_golden()
    m = FXencoder(channels=list(z["channels"]), kernels=list(z["kernels"]), strides=list(z["strides"]))
    own = m.state_dict()
    assert set(sd) == set(own), set(sd) ^ set(own)
    m.load_state_dict({"module." + k: v for k, v in sd.items()})   # a DistributedDataParallel checkpoint
    for k, v in m.state_dict().items():
        if not k.endswith("num_batches_tracked"):
            assert torch.equal(v.double(), sd[k].float().double()), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if "encoder.1.conv2.conv1d.conv1d.bias" != k})
    assert m.embed_dim == 64 and next(m.parameters()).dtype == torch.float32 and not m.training


def test_fold_equals_bias_then_batch_norm():
    from st_ito.models.fx_encoder import fold_batch_norm
    g = torch.Generator().manual_seed(3)
    p = R.random_layer(g, 7, 19, 10, dtype=torch.float64)
    assert (p["gamma"] < 0).any() and (p["gamma"] > 0).any()
    x = torch.randn(2, 7, 40, generator=g, dtype=torch.float64)
    want = R.batch_norm(R.conv_bias(x, p, 2), p)
    scale, shift = fold_batch_norm(p["bias"], p["gamma"], p["beta"], p["mean"], p["var"])
    assert scale.dtype == torch.float64
    nobias = dict(p, bias=torch.zeros_like(p["bias"]))
    got = R.conv_bias(x, nobias, 2) * scale[None, :, None] + shift[None, :, None]
    assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("cout,cin,k,stride", [(1, 5, 25, 4), (33, 33, 10, 1), (65, 64, 15, 2), (128, 5, 5, 1), (16, 2, 25, 4), (3, 2, 7, 3)])
def test_weight_packing_round_trips(cout, cin, k, stride):
    from st_ito import _hip
    from st_ito.models.fx_encoder import layer_tiles, pack_conv1d_weights, unpack_conv1d_weights
    bm, bk = layer_tiles(cout, cin, k, stride)
    w = torch.randn(cout, cin, k, generator=torch.Generator().manual_seed(cout))
    packed = pack_conv1d_weights(w, bm, bk)
    assert packed.numel() == _hip.lib().stito_fxenc_packed_floats(cout, cin, k, stride)
    assert torch.equal(unpack_conv1d_weights(packed, cout, cin, k, bm, bk), w)
    if bm:   # element (mt, r, mi) = w[mt * bm + mi][r // k][r % k]; the padding is zero
        rpad = -(-cin * k // bk) * bk
        p3 = packed.reshape(-1, rpad, bm)
        co, ci, t = cout - 1, cin - 1, k - 1
        assert p3[co // bm, ci * k + t, co % bm] == w[co, ci, t]
        assert int((packed != 0).sum()) == int((w != 0).sum())
    else:
        assert cin <= 2 and torch.equal(packed.reshape(w.shape), w)


def test_length_rule_and_too_short_inputs():
    from st_ito import _hip
    from st_ito.models.fx_encoder import FXencoder, out_len, reflect_pads
    assert reflect_pads(10) == (4, 5) and reflect_pads(25) == (12, 12) and reflect_pads(5) == (2, 2)
    lib = _hip.lib()
    for n, s in [(240845, 4), (60212, 4), (15053, 2), (941, 2), (59, 1), (1, 4), (8, 4), (9, 4)]:
        assert out_len(n, s) == math.ceil(n / s) == lib.stito_fxenc_out_len(n, s)
    m = FXencoder()
    lens = m.layer_lengths(240845)
    assert len(lens) == 24 and [o for _, _, o in lens][1::2] == [60212, 15053, 7527, 3764, 1882, 941, 471, 236, 118, 59, 59, 59]
    assert all(o == i for _, i, o in lens[0::2])   # a block's first layer keeps the length
    shortest = m.min_input_length()
    m.layer_lengths(shortest)
    with pytest.raises(ValueError, match=r"encoder\.\d+\.conv[12]"):
        m.layer_lengths(shortest - 1)
    # a net whose binding layer is in the middle: the K = 10 block needs 6 samples behind a stride-4 block
    t = FXencoder(channels=[5, 33, 64], kernels=[25, 10, 5], strides=[4, 2, 1])
    assert t.min_input_length() == 21 and out_len(21, 4) == 6
    t.layer_lengths(21)
    with pytest.raises(ValueError, match=r"encoder\.1\.conv1 "):
        t.layer_lengths(20)
    with pytest.raises(ValueError, match=r"encoder\.0\.conv1 "):
        t.layer_lengths(12)


def test_symbols_constructor_contract_and_defaults():
    from st_ito import _hip
    from st_ito.models import fx_encoder as FX
    for name in ("stito_fxenc_out_len", "stito_fxenc_tile_m", "stito_fxenc_tile_k", "stito_fxenc_packed_floats", "stito_fxenc_conv1d",
                 "stito_fxenc_pool", "stito_fxenc_workspace_bytes", "stito_fxenc_forward"):
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
    assert _hip.lib().stito_version() == 10 and _hip.lib().stito_version_minor() >= 11
    for kw in (dict(conv_block="conv"), dict(norm="instance"), dict(norm=None), dict(activation="lrelu"), dict(dilation=[1] * 11 + [2])):
        with pytest.raises(NotImplementedError):
            FX.FXencoder(**kw)
    with pytest.raises(NotImplementedError):
        FX.FXencoder().train()
    a, b = FX.FXencoder(), FX.FXencoder()
    assert a.channels == b.channels == [2, 16, 32, 64, 128, 256, 256, 512, 512, 1024, 1024, 2048, 2048]
    assert FX.DEFAULT_CHANNELS == (16, 32, 64, 128, 256, 256, 512, 512, 1024, 1024, 2048, 2048)
    assert a.embed_dim == 2048 and sum(p.numel() for p in a.parameters()) > 81e6
    mine = [16, 32]
    FX.FXencoder(channels=mine, kernels=[25, 25], strides=[4, 4])
    assert mine == [16, 32]   # the caller's list is copied, not extended
    a.eval()
    assert not a.training


def test_loader_and_synthetic_model(tmp_path):
    from st_ito.utils import load_fx_encoder_model, make_synthetic_fx_encoder
    missing = str(tmp_path / "FXencoder_ps.pt")
    with pytest.raises(FileNotFoundError, match="FXencoder_ps.pt"):
        load_fx_encoder_model(ckpt_path=missing)
    m = make_synthetic_fx_encoder(1, channels=[16, 32], kernels=[25, 15], strides=[4, 2])
    sd = m.state_dict()
    assert (sd["encoder.1.conv2.conv1d.batch_norm.weight"] < 0).any() and float(sd["encoder.0.conv1.conv1d.batch_norm.running_var"].min()) >= 0.25
    m2 = make_synthetic_fx_encoder(1, channels=[16, 32], kernels=[25, 15], strides=[4, 2])
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    if not torch.cuda.is_available():   # no CPU fallback: the forward fails loudly without a device
        from st_ito import _hip
        with pytest.raises(_hip.StitoError):
            m(torch.zeros(1, 2, 4096))
