#!/usr/bin/env python
"""FX-Encoder forward on the GPU: the product's HIP stack (stito_fxenc_forward) against the same network written in torch
(F.pad(mode="reflect") + F.conv1d + the folded affine, float32), default configuration, synthetic weights, at the ES's own shape:
(P, 2, 240 845) -- a 262 144-sample crop at 48 kHz resampled to 44.1 kHz.

The two sides alternate call by call in one process; each call is bracketed by device events and the medians of --reps calls
after --warmup are reported.  One extra pass launches the product's layers one by one (stito_fxenc_conv1d) with an event pair per
launch: time and achieved TFLOP/s per layer, FLOPs = 2 cout cin K Lout P as the algorithm needs them (tile padding not counted),
next to the f32 matrix pipe's 157.3 TFLOP/s peak.  Needs a GPU; writes --out (default profiles/fx_encoder.txt).

    python tools/fx_encoder_bench.py --pops 32 128 256
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "st-ito_amd"))

F32_MFMA_PEAK_TFLOPS = 157.3
N_SAMPLES = 240845


def torch_forward(x, layers):
    for w, scale, shift, k, stride, residual in layers:
        y = F.conv1d(F.pad(x, ((k - 1) // 2, (k - 1) - (k - 1) // 2), mode="reflect"), w, None, stride=stride)
        y = torch.relu(y * scale[None, :, None] + shift[None, :, None])
        x = y + x if residual else y
    return x.mean(dim=-1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pops", type=int, nargs="+", default=[32, 128, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=N_SAMPLES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fx_encoder.txt"))
    a = ap.parse_args(argv)

    from st_ito import _hip
    from st_ito.models.fx_encoder import fold_batch_norm
    from st_ito.utils import make_synthetic_fx_encoder

    _hip.require_gpu()
    dev = torch.device("cuda", 0)
    model = make_synthetic_fx_encoder(0)
    _, M, _ = model.prepare()
    tl = []
    for _, ly in model.layers():
        conv, bn = ly.conv1d.conv1d, ly.conv1d.batch_norm
        scale, shift = fold_batch_norm(conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        tl.append((conv.weight.detach(), scale.float().to(dev), shift.float().to(dev), ly.kernel, ly.stride, ly.residual))
    L = _hip.lib()
    lines = [f"FX-Encoder forward, default configuration (24 conv1d layers, {sum(p.numel() for p in model.parameters()) / 1e6:.1f} M parameters), "
             f"synthetic weights, input (P, 2, {a.samples}) float32",
             f"device: {torch.cuda.get_device_name(0)}; medians of {a.reps} calls after {a.warmup} warm-up calls, product and torch "
             "alternating call by call, device events around each call", ""]
    per_layer = {}
    for P in a.pops:
        x = torch.randn(P, 2, a.samples, device=dev, generator=torch.Generator(device=dev).manual_seed(P))
        x /= x.abs().max()
        t_hip, t_torch, diff = [], [], None
        with torch.no_grad():
            for i in range(a.warmup + a.reps):
                th, yh = timed(lambda: model(x))
                tt, yt = timed(lambda: torch_forward(x, tl))
                if i >= a.warmup:
                    t_hip.append(th); t_torch.append(tt)
                diff = float((yh - yt).abs().max()), float(yt.abs().max())
        flops = sum(2.0 * ly.cout * ly.cin * ly.kernel * o * P for (_, ly), (_, _, o) in zip(model.layers(), model.layer_lengths(a.samples)))
        mh, mt = statistics.median(t_hip), statistics.median(t_torch)
        lines.append(f"P = {P:3d}: product {mh:9.2f} ms (min {min(t_hip):.2f}, max {max(t_hip):.2f}; {flops / mh / 1e9:6.1f} TFLOP/s end to end)   "
                     f"torch {mt:9.2f} ms (min {min(t_torch):.2f}, max {max(t_torch):.2f})   torch / product {mt / mh:5.2f}   "
                     f"max |product - torch| {diff[0]:.2e} at max |e| {diff[1]:.3g}")
        print(lines[-1], flush=True)
        # per layer: the product's launches one by one, an event pair each
        bufs = [torch.empty(P * 16 * (-(-a.samples // 4)) + 16, device=dev), torch.empty(P * 16 * (-(-a.samples // 4)) + 16, device=dev)]
        need = max(P * ly.cout * o for (_, ly), (_, _, o) in zip(model.layers(), model.layer_lengths(a.samples)))
        assert need <= bufs[0].numel()
        cur, rows, evs = x, [], []
        for i, ((name, ly), (_, n_in, n_out)) in enumerate(zip(model.layers(), model.layer_lengths(a.samples))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            dst = bufs[i & 1]
            e0.record()
            _hip.check(L.stito_fxenc_conv1d(M.layers[i], _hip.ptr(cur), P, n_in, _hip.ptr(dst), _hip.stream_ptr()))
            e1.record()
            evs.append((name, ly, n_in, n_out, e0, e1))
            cur = dst
        torch.cuda.synchronize()
        for name, ly, n_in, n_out, e0, e1 in evs:
            ms = e0.elapsed_time(e1)
            gf = 2.0 * ly.cout * ly.cin * ly.kernel * n_out * P / 1e9
            rows.append((name, ly.cin, ly.cout, ly.kernel, ly.stride, n_in, n_out, ms, gf, gf / ms))
        per_layer[P] = rows
        del x, bufs
        torch.cuda.empty_cache()
    for P, rows in per_layer.items():
        lines += ["", f"per layer at P = {P} (one pass, one event pair per launch; TFLOP/s of the algorithm's FLOPs; peak of the f32 matrix pipe "
                      f"{F32_MFMA_PEAK_TFLOPS})", f"{'layer':18s} {'cin':>5s} {'cout':>5s} {'K':>3s} {'s':>2s} {'L in':>7s} {'L out':>7s} {'ms':>9s} {'GFLOP':>9s} {'TFLOP/s':>8s} {'of peak':>8s}"]
        for name, cin, cout, k, s, n_in, n_out, ms, gf, tf in rows:
            lines.append(f"{name:18s} {cin:5d} {cout:5d} {k:3d} {s:2d} {n_in:7d} {n_out:7d} {ms:9.3f} {gf:9.1f} {tf:8.1f} {100 * tf / F32_MFMA_PEAK_TFLOPS:7.1f}%")
        lines.append(f"{'sum':18s} {'':35s} {sum(r[7] for r in rows):9.3f} {sum(r[8] for r in rows):9.1f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[3 + len(a.pops):]))
    print("->", a.out)


if __name__ == "__main__":
    main()
