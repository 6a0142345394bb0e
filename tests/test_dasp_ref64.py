"""CPU pins of tests/dasp_ref64.py -- the float64 reference that tests/test_gpu_dasp_chain.py trusts -- and of the formulation the
kernels use instead of a large FFT (the causal recursion started from the periodic state), plus the host-side counts of the
"autodiff" chain.  A wrong reference or a wrong formulation fails here, not on the GPU machine."""
import numpy as np
import scipy.signal
import torch

import dasp_ref64 as R

SR = 48000


def _raw(v, lo, hi):
    return (v - lo) / (hi - lo)


def _eq_params(sections):
    """[(gain_db, freq, q)] * 6 -> (1, 18) raw parameters"""
    return torch.tensor([[_raw(v, *R.EQ_RANGES[k]) for sec in sections for k, v in enumerate(sec)]], dtype=torch.float64)


# the corner the issue measured: two sections at 20 Hz / Q 10 / +18 dB, the others spread over the ranges' other ends
CORNER = [(18.0, 20.0, 10.0), (18.0, 20.0, 10.0), (-18.0, 1000.0, 0.1), (6.0, 3000.0, 1.0), (18.0, 20000.0, 10.0), (-18.0, 20000.0, 0.1)]


def test_ref64_eq_is_the_causal_filter_when_the_impulse_response_is_short():
    """Cutoffs >= 1 kHz and Q <= 1: the impulse response has died out long before N - L >= L samples, so circular == causal and
    the FFT form must reproduce scipy.signal.sosfilt to float64 rounding (1e-9 of peak)."""
    rng = np.random.default_rng(11)
    n = 65536
    x = torch.from_numpy((0.3 * rng.standard_normal((1, 2, n))).astype(np.float32))
    for _ in range(4):
        secs = [(rng.uniform(-18, 18), rng.uniform(1000, 20000), rng.uniform(0.1, 1.0)) for _ in range(6)]
        p = _eq_params(secs)
        got = R.parametric_eq(x, p, SR)[0].numpy()
        ref = scipy.signal.sosfilt(R.eq_sos(p, SR)[0].numpy(), x[0].double().numpy(), axis=-1)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"ref64 EQ vs sosfilt: {err:.2e}")
        assert err < 1e-9, err


def test_periodic_start_recursion_is_the_frequency_sampled_eq():
    """20 Hz / Q 10 / +18 dB, L = 4096: the frequency-sampled filter is circular over N = 8192 and far from the causal one; the
    recursion started from s* = (I - A^N)^-1 A^(N - L) s_L is it."""
    rng = np.random.default_rng(0)
    n = 4096
    x = (0.3 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 20 * np.arange(n) / SR)).astype(np.float32)
    p = _eq_params(CORNER)
    ref = R.parametric_eq(torch.from_numpy(x)[None, None], p, SR)[0, 0].numpy()
    sos = R.eq_sos(p, SR)[0].numpy()
    peak = np.abs(ref).max()
    e_proto = np.abs(R.eq_periodic_start(sos, x) - ref).max() / peak
    e_causal = np.abs(scipy.signal.sosfilt(sos, x.astype(np.float64)) - ref).max() / peak
    print(f"periodic-start vs ref64: {e_proto:.2e}; sosfilt vs ref64: {e_causal:.2e}")
    assert e_proto < 1e-6, e_proto
    assert e_causal > 0.1, e_causal
    # L == 1: N == 1 and rfft(b, 1) keeps b0 alone
    one = R.parametric_eq(torch.ones(1, 1, 1), p, SR).item()
    assert abs(one - float(np.prod(sos[:, 0]))) < 1e-12 * abs(one) and abs(R.eq_periodic_start(sos, [1.0])[0] - one) < 1e-12 * abs(one)


def test_periodic_start_recursion_is_the_frequency_sampled_one_pole():
    """The compressor's smoother at attack 250 ms (alpha^8192 = 0.22), L = 4096, on a gain-computer-like step signal."""
    rng = np.random.default_rng(1)
    n = 4096
    g_c = -20.0 * (rng.random(n) < 0.5) * rng.random(n)
    alpha = float(R.compressor_alpha(torch.tensor([250.0]), SR)[0])
    assert alpha == float(np.float32(alpha)) and abs(alpha - np.exp(-np.log(9.0) / 12000.0)) < 6e-8
    b, a = torch.tensor([[1 - alpha, 0.0]], dtype=torch.float64), torch.tensor([[1.0, -alpha]], dtype=torch.float64)
    N = R.fft_len(n)
    ref = torch.fft.irfft(torch.fft.rfft(torch.from_numpy(g_c)[None], N) * (torch.fft.rfft(b, N) / torch.fft.rfft(a, N)), N)[0, :n].numpy()
    peak = np.abs(ref).max()
    e_proto = np.abs(R.onepole_periodic_start(alpha, g_c) - ref).max() / peak
    e_causal = np.abs(scipy.signal.lfilter([1 - alpha], [1.0, -alpha], g_c) - ref).max() / peak
    print(f"one-pole periodic-start vs FFT: {e_proto:.2e}; lfilter vs FFT: {e_causal:.2e}")
    assert e_proto < 1e-6, e_proto
    assert e_causal > 0.1, e_causal


def test_ref64_compressor_lookahead_and_short_inputs():
    """The signal path is delayed by 512 samples, the gain is not; up to 512 samples nothing comes out."""
    rng = np.random.default_rng(2)
    x = torch.from_numpy((0.5 * rng.standard_normal((1, 2, 2048))).astype(np.float32))
    p = torch.tensor([[1.0, 0.0, 0.5, 0.5, 0.5, 0.0]], dtype=torch.float64)   # threshold 0 dB, ratio 1: unit gain
    y = R.compressor(x, p, SR)
    assert torch.all(y[..., :512] == 0) and torch.allclose(y[..., 512:], x[..., :-512].double(), atol=1e-12)
    for n in (1, 511, 512):
        assert torch.all(R.compressor(x[..., :n], p, SR) == 0)


def test_autodiff_chain_host_counts():
    from st_ito import _hip, effects as E
    from st_ito.engine import compile_chain
    lib = _hip.lib()
    assert lib.stito_version() == 10 and lib.stito_version_minor() >= 2
    assert [lib.stito_fx_num_params(k) for k in (8, 9, 10)] == [18, 6, 1]
    assert lib.stito_fx_num_params(11) < 0
    pl = E.make_plugins("autodiff")
    d, n = compile_chain({k: v for k, v in pl.items() if k != "Reverb"})   # (the reverb's noise bank lives on the GPU)
    assert n == 26 and [x.kind for x in list(d)[:4]] == [8, 9, 10, 5]
    sizes = [v["num_params"] for v in pl.values()]
    assert sizes == [18, 6, 1, 25, 1] and sum(sizes) == 51
    assert list(np.cumsum([0] + sizes[:-1])) == [0, 18, 24, 25, 50]
    assert [E.DaspParametricEQ.KIND, E.DaspCompressor.KIND, E.DaspDistortion.KIND] == [8, 9, 10]
    eq = E.DaspParametricEQ()
    assert len(eq.parameters) == 18 and all((p.min_value, p.max_value) == R.EQ_RANGES[i] for i, p in enumerate(eq.parameters.values()))
    assert [(p.min_value, p.max_value) for p in E.DaspCompressor().parameters.values()] == R.COMP_RANGES
    assert [(p.min_value, p.max_value) for p in E.DaspDistortion().parameters.values()] == [(0.0, 48.0)]
    # the dasp compressor never up-mixes: a chain of it alone keeps one channel whatever num_channels says
    one = E.make_plugins([("Compressor", E.DaspCompressor, 2)])
    assert lib.stito_chain_out_channels(compile_chain(one)[0], 1, 1) == 1
    # its out-of-place copy is in the workspace
    with_c = lib.stito_render_workspace_bytes(compile_chain(one)[0], 1, 2, 48000, 4)
    without = lib.stito_render_workspace_bytes(compile_chain(E.make_plugins([("Distortion", E.DaspDistortion, 1)]))[0], 1, 2, 48000, 4)
    assert with_c - without >= 4 * 2 * 48000 * 4
    # the reference's assertions on the apply_* surface fire before anything touches a GPU
    import pytest
    with pytest.raises(AssertionError):
        E.apply_parametric_eq(torch.zeros(1, 1, 64), torch.zeros(1, 15), SR)
    with pytest.raises(AssertionError):
        E.apply_parametric_eq(torch.zeros(1, 1, 64), torch.zeros(1, 18), 22050)
    with pytest.raises(AssertionError):
        E.apply_complex_autodiff_processor(torch.zeros(1, 1, 64), torch.full((1, 51), 1.5), SR)
    with pytest.raises(AssertionError):
        E.apply_compressor(torch.zeros(1, 1, 64), torch.zeros(1, 4), SR)
    assert not hasattr(E, "apply_simple_autodiff_processor")
    from st_ito.utils import get_param_embeds
    with pytest.raises(NotImplementedError):
        get_param_embeds(torch.zeros(1, 2, 64), None, SR, requires_grad=True)
