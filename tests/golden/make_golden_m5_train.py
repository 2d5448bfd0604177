#!/usr/bin/env python
"""Golden vectors of M5 in train mode, produced by running the REFERENCE's own ``M5Net.M5`` (audio_models/M5/M5Net.py) in
``.train()`` with ``F.nll_loss`` and autograd on the CPU, float32 (build container only), as audio_models/M5/train.py:86-103 does.
Nothing of the reference is stored: weights, clips and labels are the recipes of tests/m5_train_restate.py (``synth`` weights with
every fifth gamma negated), and the file holds the reference's outputs.

golden_m5_train_v1.npz, for each case c = 0, 1 (m5_train_restate.SHAPES[1] and [2]):
  c/shape                (B, L, n_channel, n_output)
  c/logp, c/loss         log-probabilities [B,n_output] and the nll loss of the first train-mode forward
  c/grad/<parameter>     every parameter gradient of that loss;  c/dx [B,1,L]
  c/run1/<buffer>, c/run2/<buffer>   bn{i}.running_mean / running_var / num_batches_tracked after one and after two forwards
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (sets up sys.path and the third-party mocks; imports the reference's M5)

import m5_train_restate as T  # noqa: E402

CASES = (T.SHAPES[1], T.SHAPES[2])


def main():
    out = {}
    for c, shape in enumerate(CASES):
        B, L, nc, no = shape
        sd, x, y = T.case_inputs(shape)
        m = G.M5(n_input=1, n_output=no, n_channel=nc)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        m.train()
        xr = x.clone().requires_grad_(True)
        with torch.enable_grad():
            logp = m(xr)
            loss = F.nll_loss(logp, y)
            loss.backward()
        out[f"{c}/shape"] = np.asarray(shape, np.int64)
        out[f"{c}/logp"], out[f"{c}/loss"] = logp.detach().numpy().copy(), np.float64(loss.item())
        for name, p in m.named_parameters():
            out[f"{c}/grad/{name}"] = p.grad.detach().numpy().copy()
        out[f"{c}/dx"] = xr.grad.detach().numpy().copy()
        for k, v in m.named_buffers():
            out[f"{c}/run1/{k}"] = v.detach().numpy().copy()
        with torch.no_grad():
            m(x)
        for k, v in m.named_buffers():
            out[f"{c}/run2/{k}"] = v.detach().numpy().copy()
    path = os.path.join(HERE, "golden_m5_train_v1.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
