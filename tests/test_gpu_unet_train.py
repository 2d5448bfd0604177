"""The native train step of the Improved-Diffusion UNet (UNetModel.forward_train, improved_diffusion_train.training_losses) on the GPU
against the float64 restatement (unet_train_restate.py) under the recorded bounds, and against the reference's own numbers
(tests/golden/golden_unet_train_v1.npz): loss terms, every parameter gradient, dx; determinism, accumulation, frozen parameters, the
optimizer hand-over, and that forward() is untouched by a train step."""
import copy
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_train_restate as R  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402
from audiopure_amd.diffusion_models.improved_diffusion_train import training_losses  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(R.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def drop_arg(name):
    seed, offset, p = R.drop_of(name)
    return ("philox", seed, offset)                       # p is the constructor's


def loss_step(m, name, dev):
    """zero_grad + training_losses + .mean().backward() -> (mse [B] on the CPU, {name: .grad clone})"""
    x0, t, z = R.inputs(name)
    for q in m.parameters():
        q.grad = None
    terms = training_losses(m, x0.to(dev), t, noise=z.to(dev), dropout=drop_arg(name))
    assert set(terms) == {"loss", "mse"} and terms["loss"].shape == (x0.shape[0],)
    terms["loss"].mean().backward()
    torch.cuda.synchronize()
    return terms["mse"].detach().cpu(), {k: q.grad.detach().clone() for k, q in m.named_parameters() if q.grad is not None}


@functools.lru_cache(maxsize=None)
def gpu_step(name):
    """One step of the case on cuda:0 -> (module, step dict like the restatement's).  The parameter gradients come from
    training_losses; eps and dx from forward_train on the float32 x_t of the restatement as a leaf.  Shared: do not modify."""
    dev = torch.device("cuda:0")
    m = R.build(name).to(dev)
    mse, grads = loss_step(m, name, dev)
    x0, t, z = R.inputs(name)
    x_t = R.q_sample(x0, t, z, torch.float32).to(dev).requires_grad_(True)
    eps = m.forward_train(x_t, t.to(dev).float(), dropout=drop_arg(name))
    before = {k: q.grad.detach().clone() for k, q in m.named_parameters()}
    ((z.to(dev) - eps) ** 2).flatten(1).mean(1).mean().backward()
    torch.cuda.synchronize()
    twice = {k: q.grad.detach().clone() for k, q in m.named_parameters()}
    return m, dict(eps=eps.detach().cpu(), mse=mse, grads={k: g.cpu() for k, g in grads.items()}, dx=x_t.grad.detach().cpu()), before, twice


@pytest.mark.parametrize("name", NAMES)
def test_train_step_against_the_float64_restatement(name):
    m, got, _, _ = gpu_step(name)
    ref = R.reference(name)[0]
    fwd, grad, worst = R.compare(got, ref, R.structural_zeros(m))
    print(f"{name}: forward {fwd:.2e} (bound {R.FWD_BOUND:.2e}), gradients {grad:.2e} at {worst} (bound {R.GRAD_BOUND:.2e})")
    assert all(bool(torch.isfinite(g).all()) for g in got["grads"].values()) and set(got["grads"]) == set(ref["grads"])
    assert fwd <= R.FWD_BOUND
    assert grad <= R.GRAD_BOUND


@pytest.mark.parametrize("name", ["a", "b"])
def test_train_step_against_the_references_own_numbers(name):
    _, got, _, _ = gpu_step(name)
    fwd, grad = R.compare_golden(got, name, R.reference(name)[0])
    print(f"{name}: against the golden: forward {fwd:.2e}, gradients {grad:.2e}")
    assert fwd <= R.FWD_BOUND + R.FWD_F32_ERR and grad <= R.GRAD_BOUND + R.GRAD_F32_ERR     # the golden is itself float32 torch


def test_two_runs_give_equal_bits_and_two_backwards_accumulate(dev):
    m, got, before, twice = gpu_step("a")
    mse2, grads2 = loss_step(copy.deepcopy(m), "a", dev)
    assert torch.equal(mse2, got["mse"])
    for k, g in grads2.items():
        assert torch.equal(g.cpu(), got["grads"][k]), k
    # the second backward (forward_train on the restatement's x_t: the same step up to the rounding of x_t) added to .grad
    ref = R.reference("a")[0]
    zeros = R.structural_zeros(m)
    for k, g in got["grads"].items():
        assert torch.equal(before[k].cpu(), g), k
        scale = float(ref["grads"][zeros.get(k, k)].abs().max())
        assert float((twice[k].cpu().double() - 2 * ref["grads"][k]).abs().max()) <= 2 * R.GRAD_BOUND * scale, k
        if k not in zeros:
            assert not torch.equal(twice[k].cpu(), g), k


def test_a_frozen_parameter_gets_none_and_the_rest_their_bits(dev):
    m, got, _, _ = gpu_step("c")
    m2 = copy.deepcopy(m)
    frozen = ["input_blocks.1.0.in_layers.2.weight", "input_blocks.1.0.out_layers.0.weight", "input_blocks.1.0.emb_layers.1.bias",
              "time_embed.0.weight", "out.0.bias"]
    ps = dict(m2.named_parameters())
    for k in frozen:
        ps[k].requires_grad_(False)
    _, grads = loss_step(m2, "c", dev)
    for k, q in m2.named_parameters():
        if k in frozen:
            assert q.grad is None, k
        else:
            assert torch.equal(grads[k].cpu(), got["grads"][k]), k


def test_default_dropout_seeds_from_torchs_cpu_generator(dev):
    m = copy.deepcopy(gpu_step("a")[0])
    x0, t, z = R.inputs("a")
    outs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        with torch.no_grad():
            outs.append(m.forward_train(x0.to(dev), t.to(dev).float()))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    with torch.no_grad():
        off = m.forward_train(x0.to(dev), t.to(dev).float(), dropout=("philox", 1, 0, 0.0))
    m.eval()
    with torch.no_grad():                                                   # p = 0: the inference network, no dropout launch
        assert torch.equal(off, m.forward_save(x0.to(dev), t.to(dev).float())[0])
        assert R.rel(off, m(x0.to(dev), t.to(dev).float())) <= R.FWD_BOUND


def test_adamw_step_is_seen_by_forward_and_forward_is_untouched_by_training(dev):
    m = copy.deepcopy(gpu_step("b")[0])
    x0, t, z = R.inputs("b")
    x, ts = x0.to(dev), t.to(dev).float()
    fresh = m(x, ts).clone()                                                # train mode, grad enabled, as existing callers
    saved = copy.deepcopy(m.state_dict())
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    opt.zero_grad()
    training_losses(m, x, t, noise=z.to(dev), dropout=drop_arg("b"))["loss"].mean().backward()
    opt.step()
    m.eval()
    moved = m(x, ts)
    assert float((moved - fresh).abs().max()) > 1e-4 * float(fresh.abs().max())          # the updated weights were re-packed
    # the same eps as a module that never trained, built from the updated state dict
    m3 = R.build("b").to(dev).eval()
    m3.load_state_dict(m.state_dict())
    assert torch.equal(m3(x, ts), moved)
    m.load_state_dict(saved)
    m.train()
    assert torch.equal(m(x, ts), fresh)                                     # restored weights: identical bits


def test_refusals(dev):
    from audiopure_amd.diffusion_models.improved_diffusion_unet import UNetModel
    m = copy.deepcopy(gpu_step("b")[0])
    x0, t, z = R.inputs("b")
    x, ts = x0.to(dev), t.to(dev).float()
    m.set_precision("f32s")
    with pytest.raises(N.NativeError, match="fp32"):
        m.forward_train(x, ts)
    m.set_precision("f32")
    xg = x.clone().requires_grad_(True)
    eps = m.forward_train(xg, ts, dropout=("philox", 1, 0))
    (g,) = torch.autograd.grad(eps.sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):                                       # once differentiable: a double backward raises
        g.sum().backward()
    sig = UNetModel(in_channels=1, model_channels=32, out_channels=2, num_res_blocks=1, attention_resolutions=(), channel_mult=(1,)).to(dev)
    with pytest.raises(NotImplementedError, match="learn_sigma"):
        training_losses(sig, x, t)
    out = m.forward_train(x, ts)                                            # x without grad: no dx, parameters still get theirs
    out.sum().backward()
    assert xg.grad is None and m.out[2].weight.grad is not None
