"""The float64 restatement of the UNet train step (unet_train_restate.py), on the CPU: pinned to the reference's own classes
(tests/golden/golden_unet_train_v1.npz), the conditions the GPU bounds rest on hold for every case, and the recorded bounds are what
this machine measures.  The GPU tests (test_gpu_unet_train.py) hold the kernels to this restatement."""
import math
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_train_restate as R  # noqa: E402

NAMES = list(R.CASES)


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_matches_the_references_own_train_step(name):
    """The golden holds the reference's float32 numbers; the float64 restatement lies within float32 torch's own error of them, and so
    do the golden's own float32 gradients within the bound of the restatement (the same statement read the other way)."""
    ref = R.reference(name)[0]
    fwd, grad = R.compare_golden(ref, name, ref)
    print(f"{name}: restatement against the reference's float32 numbers: forward {fwd:.2e}, gradients {grad:.2e}")
    assert fwd <= R.FWD_BOUND and grad <= R.GRAD_BOUND
    G = R.golden()
    assert np.array_equal(G[name + "/loss"], G[name + "/mse"])                   # LossType.MSE without a variance head


def test_the_walk_without_dropout_is_the_oracles_forward():
    from oracle import unet_oracle as U
    m = R.build("b")
    x0, t, z = R.inputs("b")
    x_t = R.q_sample(x0, t, z, torch.float32)
    with torch.no_grad():
        got = R.Walk(m, (0, 0, 0.0))(x_t, t)
    assert torch.equal(got, U.unet_forward(m, x_t, t.float()))


@pytest.mark.parametrize("name", NAMES)
def test_conditions_the_gpu_bounds_rest_on(name):
    ref, info = R.reference(name)
    m = R.build(name)
    zeros = R.structural_zeros(m)
    _, p, B, steps, seed, side = R.CASES[name]
    assert seed == 1                                                              # the first seed tried meets every condition
    for k, g in ref["grads"].items():
        if k in zeros:                                                            # 0 in exact arithmetic: noise, far below its layer's dW
            assert float(g.abs().max()) < 1e-9 * float(ref["grads"][zeros[k]].abs().max()), k
        else:
            assert float(g.abs().max()) > 0.0, k
    assert float(ref["dx"].abs().max()) > 0.0
    assert info["min_var_over_eps"] >= R.MIN_VAR_OVER_EPS
    n_blocks = sum(1 for mod in m.modules() if type(mod).__name__ == "ResBlock")
    if p > 0:
        assert len(info["kept"]) == n_blocks
        for frac, n in info["kept"]:
            assert abs(frac - (1 - p)) <= 6 * math.sqrt(p * (1 - p) / n), (frac, n)
    else:
        assert "kept" not in info


def test_recorded_bounds_are_what_float32_torch_measures():
    """FWD_BOUND / GRAD_BOUND = 4 x the float32-torch error against the float64 restatement, maximised over the cases: re-measured
    here; the bounds must hold for the measurement, and the recorded figures must not exceed it by more than the same factor."""
    wf = wg = 0.0
    for name in NAMES:
        f, g, k = R.measure_f32(name)
        print(f"{name}: float32 torch against float64: forward {f:.2e}, gradients {g:.2e} ({k})")
        wf, wg = max(wf, f), max(wg, g)
    assert wf <= R.FWD_BOUND and R.FWD_F32_ERR <= 4 * wf            # (another CPU's float32 sums round differently: the recorded
    assert wg <= R.GRAD_BOUND and R.GRAD_F32_ERR <= 4 * wg          # figure is held to a factor of 4 either way)
    assert R.FWD_BOUND == 4 * R.FWD_F32_ERR and R.GRAD_BOUND == 4 * R.GRAD_F32_ERR


def test_dropout_mask_restatement():
    """The mask is a pure function of (seed, draw, global sample index, element): rows of a batch are the rows of its sub-batches,
    another draw or seed is another mask, and p = 0 keeps everything at scale 1."""
    full = R.dropout_mask(5, 2, 0, 4, 37, 0.3)
    assert np.array_equal(full[2:], R.dropout_mask(5, 2, 2, 2, 37, 0.3))
    assert not np.array_equal(full, R.dropout_mask(5, 3, 0, 4, 37, 0.3)) and not np.array_equal(full, R.dropout_mask(6, 2, 0, 4, 37, 0.3))
    assert set(np.unique(full)) <= {np.float32(0.0), np.float32(1.0 / 0.7)}
    assert np.array_equal(R.dropout_mask(5, 2, 0, 2, 9, 0.0), np.ones((2, 9), np.float32))
    assert np.array_equal(full[:, :5], R.dropout_mask(5, 2, 0, 4, 5, 0.3))        # n is no part of the counter


def test_constructor_keeps_dropout_and_old_pickles_load():
    from audiopure_amd.diffusion_models.improved_diffusion_unet import UNetModel
    m = R.build("a")
    assert m.dropout_p == 0.3 and R.build("b").dropout_p == 0.0 and UNetModel.dropout_p == 0.0
    assert all(mod.p == 0.0 for mod in m.modules() if isinstance(mod, torch.nn.Dropout))    # the holders' nn.Dropout stays inert
    old = pickle.loads(pickle.dumps(m))
    del old.__dict__["dropout_p"]                                                 # a module pickled before the attribute existed
    old = pickle.loads(pickle.dumps(old))
    assert old.dropout_p == 0.0 and list(old.state_dict()) == list(m.state_dict())


def test_training_losses_refuses_a_variance_head_and_bad_steps():
    from audiopure_amd.diffusion_models.improved_diffusion_train import training_losses
    from audiopure_amd.diffusion_models.improved_diffusion_unet import UNetModel
    m = UNetModel(in_channels=1, model_channels=32, out_channels=2, num_res_blocks=1, attention_resolutions=(), channel_mult=(1,))
    with pytest.raises(NotImplementedError, match="learn_sigma"):
        training_losses(m, torch.zeros(1, 1, 8, 8), torch.tensor([3]))
    with pytest.raises(ValueError):
        R.build("b")._dropout_config(("philox", 1, 0, 1.0))
    with pytest.raises(ValueError):
        R.build("b")._dropout_config(("mt", 1, 0))
    torch.manual_seed(3)
    c1 = R.build("a")._dropout_config(None)
    torch.manual_seed(3)
    c2 = R.build("a")._dropout_config(None)
    assert c1 == c2 and c1["p"] == 0.3 and c1["seed"] != R.build("a")._dropout_config(None)["seed"]


def test_recorded_piece_bounds_are_what_float32_torch_measures():
    """test_gpu_unet_train_pieces.GN_F32_ERR / SILU_BWD_F32_ERR, re-measured: every recorded figure is within a factor of 4 of what
    float32 torch gives here, either way."""
    import test_gpu_unet_train_pieces as T
    assert set(T.GN_F32_ERR) == set(T.GN_CASES)
    for name in T.GN_CASES:
        e = T.gn_measure_f32(name)
        print(f"{name}: float32 torch against float64: {e:.2e} (recorded {T.GN_F32_ERR[name]:.2e})")
        assert e <= 4 * T.GN_F32_ERR[name] <= 16 * e
    e = R.rel(T.silu_bwd_autograd(torch.float32), T.silu_bwd_autograd(torch.float64))
    print(f"silu backward: {e:.2e} (recorded {T.SILU_BWD_F32_ERR:.2e})")
    assert e <= 4 * T.SILU_BWD_F32_ERR <= 16 * e
