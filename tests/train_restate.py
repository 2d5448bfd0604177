"""Test-side helpers of the training-step tests (test_train_cpu.py, test_gpu_train.py): the reference side of
``training_loss`` as autograd through the CPU oracle (oracle/diffwave_oracle.py: plain differentiable torch ops) in a chosen
dtype, and the per-tensor acceptance rule.  Not product code."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from audiopure_amd import synth  # noqa: E402
from oracle import diffwave_oracle as O  # noqa: E402


def leaves_of(sd, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in sd.items()}


def fold(leaves):
    """O.fold_state_dict without its casts to fp32 (so that a float64 oracle stays float64)."""
    w = {}
    for k, t in leaves.items():
        if k.endswith(".weight_v"):
            w[k[:-2]] = O.fold_weight_norm(leaves[k[:-2] + "_g"], t)
        elif not k.endswith(".weight_g"):
            w[k] = t
    return w


def oracle_loss(leaves, cfg, x, z, steps, dtype):
    """util.py:176-185 with nn.MSELoss(), the network being the oracle's; the schedule is the fp32 table every caller holds."""
    ab = O.diffusion_hyperparams(**synth.DIFFUSION_CONFIG)["Alpha_bar"]
    t = torch.as_tensor(steps).long().view(-1, 1, 1)
    x, z = x.to(dtype), z.to(dtype)
    x_t = torch.sqrt(ab[t].to(dtype)) * x + torch.sqrt(1 - ab[t].to(dtype)) * z
    eps = O.eps_net(fold(leaves), cfg, x_t, t.view(-1, 1).to(dtype))
    return torch.nn.functional.mse_loss(eps, z)


def oracle_grads(sd, cfg, x, z, steps, dtype=torch.float64):
    """(loss, {parameter name: gradient or None}) of one training step through the oracle."""
    leaves = leaves_of(sd, dtype)
    loss = oracle_loss(leaves, cfg, x, z, steps, dtype)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return loss.item(), {k: (None if g is None else g.detach()) for k, g in zip(names, grads)}


def largest(grads):
    return max(float(g.abs().max()) for g in grads.values() if g is not None)


def check_tensor(name, g, g_ref, G, rel=1e-4, report=None):
    """max|g - g_ref| <= rel * max(max|g_ref|, 1e-3 G), G the largest max|g_ref| over all tensors (the floor: init_conv's weight_v
    has gradient 0 analytically)."""
    g = torch.as_tensor(np.asarray(g)).double().reshape(-1)
    g_ref = torch.as_tensor(np.asarray(g_ref)).double().reshape(-1)
    assert g.shape == g_ref.shape, (name, g.shape, g_ref.shape)
    assert torch.isfinite(g).all(), name
    err, bound = float((g - g_ref).abs().max()), rel * max(float(g_ref.abs().max()), 1e-3 * G)
    if report is not None:
        report.append((name, err, bound))
    print(f"{name}: err {err:.3e} bound {bound:.3e} max|ref| {float(g_ref.abs().max()):.3e}")
    assert err <= bound, f"{name}: max|g - g_ref| = {err:.3e} > {bound:.3e}"
