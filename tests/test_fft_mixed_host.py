"""Host side of the mixed-radix bark spectrum (csrc/fft_mixed.hip): the float64 yardstick itself, the factorisation the
launch uses, the twiddle tables and the argument checks.  Nothing here needs a GPU.

1. tests/feature_ref64.barkspectrum -- the reference of tests/test_gpu_fft_mixed.py -- is pinned against torch.stft in
   float64 at lengths that are not powers of two, with the reference's own sequence (features.py:166-232) restated here.
2. stito_fft_mixed_plan on every even 7-smooth length in [128, 96000], and its refusals.
3. get_mir_feature_embeds refuses an unknown binding before it needs a GPU; the tables for 48 000 are float64 roots of
   unity rounded once to float32.
"""
import ctypes

import numpy as np
import pytest
import torch

import feature_ref64 as R

pytestmark = pytest.mark.filterwarnings("ignore:At least one bark filterbank", "ignore:A window was not provided")


def _fb_44100(n_freqs):
    from st_ito.features import barkscale_fbanks
    return barkscale_fbanks(n_freqs, 20.0, 20000.0, 24, 44100)


def _torch_barkspectrum(x, fb, fft, mode):
    """features.py:166-232 on float64: torch.stft without a window, |X|, mean over frames, filterbank, log, the signals
    concatenated on the last axis, rows normalised."""
    x = x.double()
    if mode == "mono":
        sigs = [x.mean(dim=1)]
    else:
        sigs = [x[:, 0] + x[:, 1], x[:, 0] - x[:, 1]]
    outs = []
    for s in sigs:
        X = torch.stft(s, n_fft=fft, hop_length=fft // 4, return_complex=True)      # (bs, n_freqs, T)
        m = X.abs().mean(dim=-1)                                                      # (bs, n_freqs)
        outs.append(torch.log(m @ fb.double() + 1e-8).unsqueeze(-1))                  # (bs, n_bands, 1)
    e = torch.cat(outs, dim=-1).reshape(x.shape[0], -1)
    return torch.nn.functional.normalize(e, p=2, dim=-1).numpy()


@pytest.mark.parametrize("fft", [250, 686, 44100, 48000])
def test_reference_pin_against_torch_stft(fft):
    """The yardstick, not the feature: passes with or without the mixed-radix kernel."""
    fb = _fb_44100(fft // 2 + 1)
    for i, n in enumerate((fft // 2 + 1, 3 * fft // 2 + 7)):
        rng = np.random.default_rng(fft + i)
        t = np.arange(n) / 48000.0
        x = 0.1 * rng.standard_normal((2, 2, n)) + 0.3 * np.sin(2 * np.pi * 440.0 * t + rng.uniform(0, 6.3, (2, 2, 1)))
        x = torch.from_numpy(x)
        for mode in ("mono", "mid-side"):
            got = R.barkspectrum(x, fb, fft, mode)
            ref = _torch_barkspectrum(x, fb, fft, mode)
            assert got.shape == ref.shape == (2, 24 * (1 if mode == "mono" else 2))
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9, err_msg=f"fft {fft} n {n} {mode}")


def _smooth_lengths():
    out = []
    for fft in range(128, 96001, 2):
        m = fft
        for p in (2, 3, 5, 7):
            while m % p == 0:
                m //= p
        if m == 1:
            out.append(fft)
    return out


def _plan(lib, fft, cap=32):
    na, nb, rad = ctypes.c_int(-1), ctypes.c_int(-1), (ctypes.c_int * cap)()
    n = lib.stito_fft_mixed_plan(fft, ctypes.byref(na), ctypes.byref(nb), rad, cap)
    return n, na.value, nb.value, list(rad[:max(n, 0)])


def test_plan_every_even_7_smooth_length():
    """Fails without the feature: the symbol does not exist."""
    from st_ito import _hip
    lib = _hip.lib()
    lengths = _smooth_lengths()
    assert len(lengths) > 300 and {44100, 48000, 22050, 32000, 88200, 96000, 128, 32768, 65536} <= set(lengths)
    for fft in lengths:
        n, na, nb, rad = _plan(lib, fft)
        assert n > 0, (fft, n, lib.stito_last_error())
        assert na * nb == fft // 2, (fft, na, nb)
        assert set(rad) <= {2, 3, 4, 5, 7}, (fft, rad)
        prods = np.cumprod(rad)
        split = int(np.searchsorted(prods, na)) + 1                 # the radices of na come first
        assert int(np.prod(rad[:split])) == na and int(np.prod(rad[split:])) == nb, (fft, na, nb, rad)
    for bad in (154, 11025, 126, 96002, 98304):
        n, _, _, _ = _plan(lib, bad)
        assert n == _hip.E_UNSUPPORTED, (bad, n)
        assert str(bad) in lib.stito_last_error().decode()
    assert _plan(lib, 48000, cap=2)[0] == _hip.E_INVALID             # eight radices do not fit two slots
    assert lib.stito_barkspectrum_mixed_workspace_bytes(3, 1, 48000) >= 3 * (24000 * 8 + 24001 * 4)
    assert lib.stito_barkspectrum_mixed_workspace_bytes(3, 1, 11025) == 0


def test_python_plan_and_refusals():
    from st_ito import features as F
    assert F.fft_mixed_plan(48000)[:2] == (160, 150) and F.fft_mixed_plan(44100)[:2] == (150, 147)
    na, nb, ra, rb = F.fft_mixed_plan(30870)
    assert int(np.prod(ra)) == na and int(np.prod(rb)) == nb and na * nb == 15435
    for bad in (154, 11025, 96002, 98304):
        with pytest.raises(NotImplementedError, match=str(bad)):
            F.fft_mixed_plan(bad)


def test_unknown_binding_is_refused_before_the_gpu():
    from st_ito.utils import get_mir_feature_embeds, load_mir_feature_extractor
    with pytest.raises(ValueError, match="binding"):
        get_mir_feature_embeds(torch.zeros(1, 2, 30000), load_mir_feature_extractor(), 48000, binding="x")


def test_tables_48000_are_rounded_float64_roots():
    from st_ito import features as F
    fft = 48000
    na, nb, _, _ = F.fft_mixed_plan(fft)
    N2 = na * nb
    tab = F.mixed_tables_host(fft)
    assert tab.dtype == np.float32 and tab.shape == (na + nb + 2 * N2, 2)

    def roots(k, n):
        w = np.exp(-2j * np.pi * (np.asarray(k, dtype=np.int64) % n) / n)
        return np.stack([w.real, w.imag], 1)

    n2, k1 = np.divmod(np.arange(N2, dtype=np.int64), na)            # the slab's order: n2 * na + k1
    want = np.concatenate([roots(np.arange(na), na), roots(np.arange(nb), nb), roots(n2 * k1, N2), roots(np.arange(N2), fft)])
    # one rounding of a value of magnitude <= 1: at most half a unit in the last place of [0.5, 1) = 2^-25 (the 0.1 % on top
    # covers a last-bit difference between the two float64 evaluations next to a rounding tie)
    assert np.abs(tab.astype(np.float64) - want).max() <= 2.0 ** -25 * 1.001
    assert np.array_equal(tab[0], [1.0, 0.0]) and np.array_equal(tab[na], [1.0, 0.0])
