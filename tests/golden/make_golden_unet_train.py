#!/usr/bin/env python3
"""Golden numbers of the REFERENCE's own train step of the spectrogram epsilon-network: its ``UNetModel(...).train()``, its
``create_gaussian_diffusion(...).training_losses`` and torch autograd (imported from the reference checkout; build container only) on
cases a and b of tests/unet_train_restate.py, float32 on the CPU.  ``nn.Dropout.forward`` is patched to apply the restatement's
counter-based mask (the reference draws from torch's global generator), one ``draw`` per call in execution order.

Per case: the loss terms, eps, dx (with respect to x_t), one gradient tensor in full per parameter kind
(``unet_train_restate.GOLDEN_FULL``) and, for every other parameter, its float64 inner product with a seeded probe vector.

    python tests/golden/make_golden_unet_train.py
"""
import os
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AUDIOPURE_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))    # the reference checkout
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
for m in ["torchvision", "torchvision.utils", "torchvision.datasets", "torchvision.transforms", "torchaudio", "torchsde",
          "librosa", "mpi4py", "blobfile", "torchaudio.transforms"]:
    sys.modules[m] = MagicMock()

from diffusion_models.Improved_Diffusion_Unconditional.improved_diffusion.unet import UNetModel as RefUNet   # noqa: E402
from diffusion_models.Improved_Diffusion_Unconditional.improved_diffusion import script_util as su            # noqa: E402
import unet_train_restate as R                                                                                 # noqa: E402
sys.path.insert(1, os.path.join(ROOT, "tools"))
from synth_convnets import synth_init                                                                          # noqa: E402

dd = su.model_and_diffusion_defaults()
diff = su.create_gaussian_diffusion(steps=dd["diffusion_steps"], learn_sigma=dd["learn_sigma"], sigma_small=dd["sigma_small"],
                                    noise_schedule=dd["noise_schedule"], use_kl=dd["use_kl"], predict_xstart=dd["predict_xstart"],
                                    rescale_timesteps=dd["rescale_timesteps"], rescale_learned_sigmas=dd["rescale_learned_sigmas"],
                                    timestep_respacing=dd["timestep_respacing"])
assert dd["diffusion_steps"] == R.T_STEPS

out = {}
for name in ("a", "b"):
    kw, p, B, steps, seed, side = R.CASES[name]
    ref = synth_init(RefUNet(dropout=p, **kw), seed).train()
    assert list(ref.state_dict().keys()) == list(R.build(name).state_dict().keys())
    x0, t, z = R.inputs(name)
    dseed, offset, _ = R.drop_of(name)
    state = {"draw": 0}

    def dropout_forward(self, h):
        assert self.training and abs(self.p - p) < 1e-12
        draw, state["draw"] = state["draw"], state["draw"] + 1
        if p == 0.0:
            return h
        return h * torch.from_numpy(R.dropout_mask(dseed, draw, offset, h.shape[0], h[0].numel(), p)).reshape(h.shape)

    leaves = []

    def model(x, ts, **kwargs):
        leaves.append(x.detach().requires_grad_(True))
        model.eps = ref(leaves[-1], ts, **kwargs)
        return model.eps

    keep = torch.nn.Dropout.forward
    torch.nn.Dropout.forward = dropout_forward
    try:
        terms = diff.training_losses(model, x0, t, noise=z)
        terms["loss"].mean().backward()
    finally:
        torch.nn.Dropout.forward = keep
    assert state["draw"] == sum(1 for m in ref.modules() if type(m).__name__ == "ResBlock")
    pre = name + "/"
    out[pre + "mse"] = terms["mse"].detach().numpy().copy()
    out[pre + "loss"] = terms["loss"].detach().numpy().copy()
    out[pre + "eps"] = model.eps.detach().numpy().copy()
    out[pre + "dx"] = leaves[0].grad.numpy().copy()
    for k, q in ref.named_parameters():
        if k in R.GOLDEN_FULL:
            out[pre + "grad/" + k] = q.grad.numpy().copy()
        else:
            out[pre + "dot/" + k] = np.float64((q.grad.double() * R.golden_probe(k, q.shape)).sum())

path = os.path.join(HERE, "golden_unet_train_v1.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes;", len(out), "entries")
