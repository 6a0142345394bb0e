"""The generated kernel sources under st-ito_amd/csrc are committed (the build needs no Python) and hold register contracts
that nothing else states: fixed VGPRs declared only as clobbers, operand registers shared between asm statements.  Each must
be, byte for byte, what its generator under tools/gen prints -- a hand edit of an .inc, or a generator change without
regenerating, fails here.  No GPU, no hipcc; nothing is written inside the repository."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENERATED = [
    ("conv_wino23r_body.inc", "gen_w23_body.py", []),
    ("conv_wino23r_body_f1.inc", "gen_w23_body.py", ["fuse1"]),
    ("conv_wino23r_pro.inc", "gen_w23_body.py", ["prologue"]),
    ("comp_scan.inc", "gen_comp_scan_asm.py", []),
]


@pytest.mark.parametrize("inc,gen,args", GENERATED, ids=[g[0] for g in GENERATED])
def test_committed_file_is_its_generators_output(inc, gen, args, tmp_path):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen", gen)] + args, cwd=tmp_path, capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    committed = open(os.path.join(ROOT, "st-ito_amd", "csrc", inc), "rb").read()
    regen = "python tools/gen/" + " ".join([gen] + args) + " > st-ito_amd/csrc/" + inc
    assert run.stdout == committed, f"st-ito_amd/csrc/{inc} is not what its generator prints; regenerate it: {regen}"
    assert not list(tmp_path.iterdir()), "the generator wrote a file: it is meant to print to stdout only"
