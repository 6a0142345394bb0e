"""Generate tests/golden/rule_based_eq.npz: the matched-EQ half of the reference's run_rule_based on seeded short inputs.

The average spectra and their smoothing come from the reference's own get_average_spectrum and smooth_spectrum (imported
through _ref_import.install_stubs(); both are pure torch / scipy, so no stand-in supplies arithmetic); the firwin2 design
and the lfilter call are scipy's, called directly.  Cases: tests/rule_based_ref.py GOLDEN_CASES (1 s stereo and 0.5 s mono
at 48 kHz, 0.5 s stereo at 44.1 kHz), each at -12 dBFS like the reference's first step.  Run from the repository root:

    python tests/golden/make_golden_rule_based.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import scipy.signal
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import _ref_import  # noqa: E402
import rule_based_ref as R  # noqa: E402  (the seeded signals and the -12 dBFS step only)

_ref_import.install_stubs()
import st_ito.style_transfer as RS  # noqa: E402  (reference)


def main():
    arrs = {}
    for i, (seed, chs, n, sr) in enumerate(R.GOLDEN_CASES):
        x, t = R.case_signals(seed, chs, n, sr)
        x, t = R.peak_normalize(x), R.peak_normalize(t)
        with contextlib.redirect_stdout(io.StringIO()):
            spec_in = RS.get_average_spectrum(torch.from_numpy(x), n_fft=16384).numpy()
            spec_ref = RS.get_average_spectrum(torch.from_numpy(t), n_fft=16384).numpy()
        sm_in, sm_ref = RS.smooth_spectrum(spec_in), RS.smooth_spectrum(spec_ref)
        response = sm_ref / sm_in
        response[-1] = 0.0
        freqs = np.linspace(0, 1.0, num=len(response))
        taps = scipy.signal.firwin2(2048, freqs * (sr / 2), response, fs=sr)
        filtered = scipy.signal.lfilter(taps, [1.0], x).astype(np.float32)
        arrs.update({f"c{i}_spec_in": spec_in, f"c{i}_spec_ref": spec_ref, f"c{i}_sm_in": sm_in, f"c{i}_sm_ref": sm_ref,
                     f"c{i}_taps": taps, f"c{i}_filtered": filtered[:, ::R.GOLDEN_STRIDE]})
    path = os.path.join(HERE, "rule_based_eq.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
