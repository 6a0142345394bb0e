"""The FX-Encoder restated in torch, operation by operation as the published network applies them (reflection padding, conv1d with
bias, eval-mode batch norm, ReLU, the residual after the ReLU, the mean over positions), in the dtype it is called with:
float64 is the reference of the GPU tests, the same code in float32 on the CPU gives each case family's d32 (the distance a
plain float32 evaluation sits from float64), of which the bar is 4 x.

A network is a list of blocks; a block is {"conv1": layer, "conv2": layer, "kernel": K, "stride": S}; a layer is a dict of
the tensors weight (cout, cin, K), bias, gamma, beta, mean, var."""
import torch
import torch.nn.functional as F

EPS = 1e-5


def pads(k):
    return (k - 1) // 2, (k - 1) - (k - 1) // 2


def conv_bias(x, p, stride, dtype=torch.float64):
    """reflection padding + conv1d + bias"""
    k = p["weight"].shape[-1]
    return F.conv1d(F.pad(x.to(dtype), pads(k), mode="reflect"), p["weight"].to(dtype), p["bias"].to(dtype), stride=stride)


def batch_norm(z, p, dtype=torch.float64):
    c = lambda t: t.to(dtype)[None, :, None]  # noqa: E731
    return (z - c(p["mean"])) / torch.sqrt(c(p["var"]) + EPS) * c(p["gamma"]) + c(p["beta"])


def layer(x, p, stride, residual=False, dtype=torch.float64):
    y = torch.relu(batch_norm(conv_bias(x, p, stride, dtype), p, dtype))
    return y + x.to(dtype) if residual else y


def block(x, blk, dtype=torch.float64):
    c1 = layer(x, blk["conv1"], 1, True, dtype)
    return layer(c1, blk["conv2"], blk["stride"], False, dtype)


def stack(x, blocks, dtype=torch.float64):
    for blk in blocks:
        x = block(x, blk, dtype)
    return x.mean(dim=-1)


def embeds(x_resampled, blocks, peak="batch", dtype=torch.float64):
    """get_fx_encoder_embeds behind the resampler (taken as given): x_resampled (B, C, L) at 44.1 kHz."""
    x = x_resampled.to(dtype)
    d = x.abs().max().clamp(1e-8) if peak == "batch" else x.abs().amax(dim=(1, 2), keepdim=True).clamp(1e-8)
    x = x / d
    if x.shape[1] == 1:
        x = x.repeat(1, 2, 1)
    return stack(x, blocks, dtype)


def blocks_from_state_dict(sd, strides):
    """The reference checkpoint's keys -> blocks."""
    def lay(prefix):
        return {"weight": sd[prefix + "conv1d.weight"], "bias": sd[prefix + "conv1d.bias"], "gamma": sd[prefix + "batch_norm.weight"],
                "beta": sd[prefix + "batch_norm.bias"], "mean": sd[prefix + "batch_norm.running_mean"],
                "var": sd[prefix + "batch_norm.running_var"]}
    out = []
    for i, s in enumerate(strides):
        c1, c2 = lay(f"encoder.{i}.conv1.conv1d."), lay(f"encoder.{i}.conv2.conv1d.")
        out.append({"conv1": c1, "conv2": c2, "kernel": c1["weight"].shape[-1], "stride": int(s)})
    return out


def blocks_from_model(model):
    """An st_ito.models.fx_encoder.FXencoder's parameters (on the CPU) -> blocks."""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return blocks_from_state_dict(sd, model.strides)


def random_layer(g, cin, cout, k, dtype=torch.float32):
    """Seeded layer parameters with negative gamma in places and a running variance away from 1."""
    gamma = 0.75 + 0.5 * torch.rand(cout, generator=g)
    return {"weight": (torch.randn(cout, cin, k, generator=g) * (2.0 / (cin * k)) ** 0.5).to(dtype), "bias": (0.1 * torch.randn(cout, generator=g)).to(dtype),
            "gamma": torch.where(torch.rand(cout, generator=g) < 0.3, -gamma, gamma).to(dtype), "beta": (0.2 + 0.1 * torch.randn(cout, generator=g)).to(dtype),
            "mean": (0.1 * torch.randn(cout, generator=g)).to(dtype), "var": (0.25 + 1.5 * torch.rand(cout, generator=g)).to(dtype)}
