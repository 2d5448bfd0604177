"""The training loss of the spectrogram epsilon-network: ``GaussianDiffusion.training_losses`` (gaussian_diffusion.py:709-746) for the
recipe the reference trains it with (spect_train_mpi_run.sh:1-8, script_util.py:15-35,231-269): LossType.MSE, epsilon prediction,
fixed variance, T = 200 linear betas, no timestep rescaling.

    losses = training_losses(model, x_start, t)          # {"loss": [B], "mse": [B]}
    losses["loss"].mean().backward()                      # .grad on every parameter, from HIP kernels
    optimizer.step()

x_t is ``ap_qsample_rows`` (q_sample with one step per sample, :188-206), eps is ``UNetModel.forward_train``; the per-sample mean
(``mean_flat``), the loss weights, the final ``.mean()``, the step sampler, AdamW, EMA, DDP and the loop stay the caller's torch
(train_util.py:191-229), as for the other native training steps.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native as N
from .improved_diffusion_ddpm import GaussianTables
from .improved_diffusion_unet import UNetModel


def training_losses(model: UNetModel, x_start, t, noise=None, dropout=None, tables: GaussianTables = None):
    """x_start [B, 1, H, W] on the model's device, t [B] integer steps in [0, T); noise: the epsilon to predict (default
    ``torch.randn_like``); dropout: as ``UNetModel.forward_train``."""
    if model.out_channels != model.in_channels:
        raise NotImplementedError("audiopure_amd training_losses: learn_sigma=True (a variance head, the KL term of "
                                  "gaussian_diffusion.py:719-741) is not built")
    tb = tables if tables is not None else GaussianTables()
    dev = next(model.parameters()).device
    x0 = x_start.detach().to(dev).float().contiguous()
    B = x0.shape[0]
    tl = torch.as_tensor(t).detach().reshape(-1).long().cpu()
    if tl.numel() != B or int(tl.min()) < 0 or int(tl.max()) >= tb.T:
        raise ValueError(f"t: one step in [0, {tb.T}) per sample")
    z = torch.randn_like(x0) if noise is None else noise.detach().to(dev).float().contiguous()
    if z.shape != x0.shape:
        raise ValueError("noise must have x_start's shape")
    idx = tl.numpy()
    # _extract_into_tensor (:749-763): the float64 tables, indexed per sample and rounded to float32
    a = torch.from_numpy(tb.sqrt_ac[idx].astype(np.float32)).to(dev)
    b = torch.from_numpy(tb.sqrt_1m_ac[idx].astype(np.float32)).to(dev)
    x_t = torch.empty_like(x0)
    with torch.cuda.device(dev):
        N.check(N.lib().ap_qsample_rows(N.ptr(x0), N.ptr(z), N.ptr(a), N.ptr(b), N.ptr(x_t), B, x0[0].numel(), N.stream()),
                "ap_qsample_rows")
    eps = model.forward_train(x_t, tl.to(dev).float(), dropout=dropout)
    mse = ((z - eps) ** 2).flatten(1).mean(1)                             # mean_flat, nn.py:91-95
    return {"loss": mse, "mse": mse}
