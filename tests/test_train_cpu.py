"""The training step's CPU side: the C-ABI symbols, the golden of the reference's own ``training_loss`` + autograd
(tests/golden/make_golden_train.py) against the oracle's autograd, and the sub-batch planner."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import synth  # noqa: E402
import train_restate as T  # noqa: E402


def test_library_exports_the_weight_gradient_symbols():
    from audiopure_amd import _native as N
    lib = ctypes.CDLL(N.LIB_PATH)
    for name in ("ap_wgrad_corr", "ap_wgrad_workspace_bytes", "ap_rowsum", "ap_rowsum_f64", "ap_embed_bwd", "ap_embed_bwd_scratch_elems",
                 "ap_weight_norm_bwd"):
        assert hasattr(lib, name), name
        assert name in N.SIGNATURES, name
    N.lib()                                                       # binds every declared symbol or raises


def test_workspace_bytes_is_host_only_and_covers_the_slices():
    from audiopure_amd import _native as N
    lib = N.lib()
    assert lib.ap_wgrad_workspace_bytes(2, 512, 256, 640, 3) % (512 * 256 * 3 * 4) == 0
    assert lib.ap_wgrad_workspace_bytes(1, 64, 32, 37, 3) >= 64 * 32 * 3 * 4
    assert lib.ap_wgrad_workspace_bytes(1, 64, 32, 37, 2) == 0    # taps in {1, 3}


@pytest.fixture(scope="module")
def golden_train():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_train_v1.npz"))


def check_against_golden(gt, loss, grads, rel=1e-4):
    """``grads``: {name: tensor or None}.  Whole tensors by the per-tensor rule; sampled ones by the rule on the sample, and their
    sum / sum of squares within what that per-element bound tau allows: |sum - sum_ref| <= n tau,
    |sumsq - sumsq_ref| <= tau (2 sqrt(n sumsq_ref) + n tau)."""
    assert abs(loss - float(gt["loss"])) <= 2e-5 * abs(float(gt["loss"]))
    whole = {k[5:]: gt[k] for k in gt.files if k.startswith("grad/")}
    sampled = {k[7:]: gt[k] for k in gt.files if k.startswith("sample/")}
    G = max(float(np.abs(v).max()) for v in list(whole.values()) + list(sampled.values()))
    assert set(gt["none"].tolist()) == {k for k, g in grads.items() if g is None}
    for name, ref in whole.items():
        T.check_tensor(name, grads[name].detach().cpu(), ref, G, rel)
    for name, ref in sampled.items():
        g = grads[name].detach().cpu().double().reshape(-1)
        stride, n = int(gt["stride/" + name]), g.numel()
        T.check_tensor(name + " (sample)", g[::stride][:ref.size], ref, G, rel)
        tau = rel * max(float(np.abs(ref).max()), 1e-3 * G)
        s_ref, q_ref = float(gt["sum/" + name]), float(gt["sumsq/" + name])
        assert abs(float(g.sum()) - s_ref) <= n * tau, name
        assert abs(float((g * g).sum()) - q_ref) <= tau * (2 * (n * q_ref) ** 0.5 + n * tau), name


def test_oracle_autograd_matches_the_reference_training_step(golden_train):
    """The oracle (O.eps_net over O.fold_weight_norm of leaf tensors) differentiates to what the reference's own network,
    training_loss, nn.MSELoss() and autograd gave for the mini net, steps [3, 3, 150]: fp32 against fp32."""
    gt = golden_train
    cfg = synth.mini_wavenet_config(32, 3, 12)
    sd = synth.wavenet_state_dict(cfg, 0)
    loss, grads = T.oracle_grads(sd, cfg, torch.from_numpy(gt["x"]), torch.from_numpy(gt["z"]), gt["steps"].tolist(), torch.float32)
    check_against_golden(gt, loss, grads)


def test_float64_oracle_agrees_with_the_golden(golden_train):
    """... and the float64 oracle, the GPU tests' reference, too."""
    gt = golden_train
    cfg = synth.mini_wavenet_config(32, 3, 12)
    sd = synth.wavenet_state_dict(cfg, 0)
    loss, grads = T.oracle_grads(sd, cfg, torch.from_numpy(gt["x"]), torch.from_numpy(gt["z"]), gt["steps"].tolist(), torch.float64)
    check_against_golden(gt, loss, grads)


@pytest.mark.parametrize("steps", [[3, 3, 150], [7], [5, 9, 5, 5, 9, 5, 1], [0] * 9])
def test_sub_batch_planner_covers_every_clip_once_in_order(steps):
    from audiopure_amd.diffusion_models._grad import plan_sub_batches, step_groups
    per_clip, fixed = 1000, 24
    bytes_of = lambda k: fixed + per_clip * k
    groups = step_groups(steps)
    assert sorted(i for _, idx in groups for i in idx) == list(range(len(steps)))
    assert [idx[0] for _, idx in groups] == sorted(idx[0] for _, idx in groups)       # groups in the order of their first clip
    for budget in (10 ** 9, bytes_of(4), bytes_of(3) - 1, bytes_of(2), bytes_of(1), 1, 0):
        plan = plan_sub_batches(steps, bytes_of, budget)
        assert sorted(i for _, idx in plan for i in idx) == list(range(len(steps)))   # every clip exactly once
        fit = max(1, min(len(steps), (budget - fixed) // per_clip)) if budget >= bytes_of(1) else 1
        for t, idx in plan:
            assert idx == sorted(idx) and all(steps[i] == t for i in idx)
            assert 1 <= len(idx) <= fit
        # the sub-batches of a group follow each other in ascending clip order, and the groups keep step_groups' order
        assert [i for _, idx in plan for i in idx] == [i for _, idx in groups for i in idx]
        if budget >= bytes_of(len(steps)):
            assert plan == [(t, idx) for t, idx in groups]
        if budget < bytes_of(2):
            assert all(len(idx) == 1 for _, idx in plan)


def test_dropin_util_exports_training_loss():
    import importlib.util
    path = os.path.join(ROOT, "dropin", "diffusion_models", "DiffWave_Unconditional", "util.py")
    spec = importlib.util.spec_from_file_location("_dropin_dw_util", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from audiopure_amd.diffusion_models.DiffWave_Unconditional import util
    assert mod.training_loss is util.training_loss and mod.calc_diffusion_hyperparams is util.calc_diffusion_hyperparams


def test_narrow_net_is_a_corner_of_the_native_width():
    """A 32-channel net runs in the 64-channel kernels zero-padded (WaveNet._native_tensors): the padded state dict is a valid
    64-channel one and the oracle computes the same eps from it, bit for bit."""
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    from oracle import diffwave_oracle as O
    cfg = synth.mini_wavenet_config(32, 3, 12)
    sd = synth.wavenet_state_dict(cfg, 0)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    assert net.native_width() == 64
    name_of = {id(p): n for n, p in net.named_parameters()}
    ts = net._blob_tensors()
    cfg64 = dict(cfg, res_channels=64, skip_channels=64)
    sd64 = {name_of[id(t)]: p for t, p in zip(ts, net._native_tensors(ts))}
    assert {k: tuple(v.shape) for k, v in sd64.items()} == {k: v.shape for k, v in synth.wavenet_state_dict(cfg64, 0).items()}
    x, st = torch.from_numpy(synth.waveforms(2, 300, seed=3)), torch.tensor([[3.0], [150.0]])
    with torch.no_grad():
        assert torch.equal(O.eps_net(O.fold_state_dict(sd), cfg, x, st), O.eps_net(O.fold_state_dict(sd64), cfg64, x, st))
    wide = WaveNet_Speech_Commands(**cfg64)
    tw = wide._blob_tensors()
    assert wide.native_width() == 64 and all(a.shape == b.shape for a, b in zip(tw, wide._native_tensors(tw)))
