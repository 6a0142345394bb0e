"""Writes tests/golden/device_es_n128.npz: the state the host CMAEvolutionStrategy reaches at N = 128, popsize 64 on the
1e6-conditioned ellipsoid when its axis ratio first exceeds 1e2 (2814 iterations, 8 s of host time -- too long for a test, so the
test of the device eigendecomposition imports the recorded state; N = 5 and 37 are stepped live).  Run from the repository root:
python tests/golden/make_device_es_states.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "st-ito_amd")]

import device_es_ref as R  # noqa: E402

if __name__ == "__main__":
    es = R.step_to_axis_ratio(128, 64)
    print(es.countiter, es.D.max() / es.D.min())
    R.save_state(es, os.path.join(HERE, "device_es_n128.npz"))
