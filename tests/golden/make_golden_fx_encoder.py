"""Records tests/golden/fx_encoder_toy.npz from the reference's own FXencoder (st_ito/models/fx_encoder.py there), run once where
the reference is checked out; the fixture is data only: a seeded state dict, a (3, 2, 211) input and the float64 output.

    python tests/golden/make_golden_fx_encoder.py

The reference file imports torchaudio, which only its alias-free mode uses: the stand-in modules of _ref_import suffice.  Its
constructor inserts the stereo 2 into the list it is given (and into its own default), so every call gets a fresh list."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

CHANNELS, KERNELS, STRIDES = [5, 33, 64], [25, 10, 5], [4, 2, 1]


def main():
    _ref_import.install_stubs()
    spec = importlib.util.spec_from_file_location("ref_fx_encoder", os.path.join(_ref_import.REF, "st_ito", "models", "fx_encoder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    model = mod.FXencoder(channels=list(CHANNELS), kernels=list(KERNELS), strides=list(STRIDES), dilation=[1, 1, 1])
    g = torch.Generator().manual_seed(20261021)
    sd = model.state_dict()
    for k, v in sd.items():
        if k.endswith("num_batches_tracked"):
            continue
        if k.endswith("conv1d.weight"):
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / (v.shape[1] * v.shape[2])) ** 0.5)
        elif k.endswith("running_var"):
            v.copy_(0.25 + 1.5 * torch.rand(v.shape, generator=g))
        elif k.endswith("batch_norm.weight"):
            gamma = 0.75 + 0.5 * torch.rand(v.shape, generator=g)
            v.copy_(torch.where(torch.rand(v.shape, generator=g) < 0.3, -gamma, gamma))
        elif k.endswith("batch_norm.bias"):
            v.copy_(0.2 + 0.1 * torch.randn(v.shape, generator=g))
        else:   # conv bias, running mean
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
    model.load_state_dict(sd)
    model.double().eval()
    x = torch.randn(3, 2, 211, generator=g, dtype=torch.float64)
    with torch.no_grad():
        y = model(x)
    out = {"sd:" + k: v.double().numpy() for k, v in model.state_dict().items()}
    out.update(x=x.numpy(), y=y.numpy(), channels=np.array(CHANNELS), kernels=np.array(KERNELS), strides=np.array(STRIDES))
    path = os.path.join(HERE, "fx_encoder_toy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; output", y.shape, "max |e|", float(y.abs().max()))


if __name__ == "__main__":
    main()
