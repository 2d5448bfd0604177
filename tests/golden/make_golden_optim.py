"""Golden vectors of the EMA update from the REFERENCE's own function (improved_diffusion/nn.py:55-65 update_ema, loaded by file path
as in make_golden_unet_train.py), run in float64 on tests/optim_restate.py's golden_ema_inputs(): three calls at the default rate 0.99 and
three at train_util.py's 0.9999, the source moving between calls as it does between optimizer steps.  Only what the
reference's function produced is stored (the targets after each call); the inputs are regenerated from optim_restate.
Run in the build container only; commits tests/golden/golden_optim_v1.npz."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import optim_restate as R  # noqa: E402

spec = importlib.util.spec_from_file_location(
    "improved_diffusion_nn_ref", "/root/reference/diffusion_models/Improved_Diffusion_Unconditional/improved_diffusion/nn.py")
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)

out = {}
for rate in R.GOLDEN_EMA_RATES:
    targets, sources = R.golden_ema_inputs()
    targ = [torch.from_numpy(t.copy()) for t in targets]
    for call, src in enumerate(sources):
        if rate is None:
            mod.update_ema(targ, [torch.from_numpy(s) for s in src])         # the default rate
        else:
            mod.update_ema(targ, [torch.from_numpy(s) for s in src], rate=rate)
        for i, t in enumerate(targ):
            out[f"rate_{rate}/call{call}/t{i}"] = t.numpy().copy()
path = os.path.join(ROOT, "tests", "golden", "golden_optim_v1.npz")
np.savez_compressed(path, **out)
print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")
