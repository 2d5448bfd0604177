"""NativeConvNet in train() mode on the device, under AUDIOPURE_STRICT=1 as the suite sets it: the five small networks of
convnet_train_restate.py at B = 4, 1 x 32 x 32.  Logits, loss, running statistics and num_batches_tracked after one and two steps, every
parameter gradient and dx against the float64 restatement AT THIS RUN'S ReLU DECISIONS (convnet_train_restate.reference_at: only inputs
within the forward bound of 0 may be decided otherwise) and against the reference's own numbers (the golden) within FWD_BOUND / GRAD_BOUND; frozen stages, the no_grad forward, the re-lowered eval forward after an SGD step, equal bits of two runs, live dropout.
On the parent commit train() mode under strict is a NativeError."""
import copy
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import _native as N  # noqa: E402
from audiopure_amd import convnet  # noqa: E402
from audiopure_amd.convnet import NativeConvNet  # noqa: E402
import convnet_train_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(R.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available() and convnet.strict()
    return torch.device("cuda:0")


def native(name, dev):
    """a fresh device copy of the case's module, wrapped, in train() mode"""
    m, _, x, y = R.case(name)
    net = NativeConvNet(copy.deepcopy(m).to(dev), R.CHW).train()
    return net, x.to(dev), y.to(dev)


def step(net, x, y):
    """zero_grad + forward + CrossEntropyLoss + backward -> the dict of convnet_train_restate.train_step"""
    for q in net.module.parameters():
        q.grad = None
    xs = x.clone().requires_grad_(True)
    logits = net(xs)
    assert type(logits.grad_fn).__name__ == "_ConvNetTrainFnBackward"   # the HIP route, not the caller's module
    masks = R.masks_from_bufs(net._train_plan, logits.grad_fn.saved[0])
    loss = F.cross_entropy(logits, y)
    loss.backward()
    sd = net.module.state_dict()
    return dict(logits=logits.detach(), loss=loss.detach(), masks=masks,
                running={k: sd[k].detach().clone() for k in sd if "running_" in k or k.endswith("num_batches_tracked")},
                grads={k: (q.grad.detach().clone() if q.grad is not None else None) for k, q in net.module.named_parameters()}, dx=xs.grad.detach())


@pytest.mark.parametrize("name", NAMES)
def test_two_train_steps_match_float64_and_the_reference(dev, name):
    net, x, y = native(name, dev)
    plan = R.case(name)[1]
    g1, g2, _ = R.reference_at(name, R.golden_flips(name))
    for n_step in (1, 2):
        got = step(net, x, y)
        assert all(g is not None and torch.isfinite(g).all() for g in got["grads"].values())
        flips = R.flips_of(name, got["masks"])                   # undecided ReLU inputs this run decided the other way than float64
        r1, r2, decided = R.reference_at(name, flips)
        print(f"{name} step {n_step}: ReLU decisions other than float64's: {flips}")
        assert decided == 0, "a ReLU input that is not within the forward bound of 0 was decided the other way"
        ref = (r1, r2)[n_step - 1]
        fwd, grad = R.compare(got, ref, plan)
        gf, gg = R.compare_golden(got, name, n_step, plan, ref, (g1, g2)[n_step - 1])
        print(f"{name} step {n_step}: against float64: forward {fwd:.2e} (bound {R.FWD_BOUND:.2e}), gradients {grad:.2e} (bound "
              f"{R.GRAD_BOUND:.2e}); against the reference's float32 numbers: forward {gf:.2e}, gradients {gg:.2e}")
        assert fwd <= R.FWD_BOUND and grad <= R.GRAD_BOUND
        assert gf <= R.FWD_BOUND and gg <= R.GRAD_BOUND
        for k, v in ref["running"].items():
            if k.endswith("num_batches_tracked"):
                assert int(got["running"][k]) == int(v) == 100 + n_step


def test_frozen_stage_costs_nothing_and_changes_nothing_else(dev):
    """requires_grad=False on a stage: its .grad stays None, every other gradient and dx are the same bits."""
    net, x, y = native("resnext", dev)
    full = step(net, x, y)
    net2, _, _ = native("resnext", dev)
    frozen = [k for k, _ in net2.module.named_parameters() if k.startswith("stage_2.")]
    assert frozen
    for k, q in net2.module.named_parameters():
        q.requires_grad_(k not in frozen)
    part = step(net2, x, y)
    for k, g in full["grads"].items():
        if k in frozen:
            assert part["grads"][k] is None
        else:
            assert torch.equal(part["grads"][k], g), k
    assert torch.equal(part["dx"], full["dx"]) and torch.equal(part["logits"], full["logits"])


def test_no_grad_forward_is_the_same_bits_and_moves_the_statistics(dev):
    net, x, y = native("densenet", dev)
    net2, _, _ = native("densenet", dev)
    a = step(net, x, y)
    with torch.no_grad():
        out = net2(x)
    assert not out.requires_grad and torch.equal(out, a["logits"])
    sd = net2.module.state_dict()
    moved = 0
    for k, v in a["running"].items():
        assert torch.equal(sd[k], v), k
        moved += int(not torch.equal(v.cpu(), R.case("densenet")[0].state_dict()[k]))
    assert moved == len(a["running"])


def test_eval_after_an_sgd_step_relowers_from_the_trained_parameters(dev):
    name = "wideresnet"
    net, x, y = native(name, dev)
    opt = torch.optim.SGD(net.module.parameters(), lr=0.05)
    with torch.no_grad():
        before = net.eval()(x).clone()
    net.train()
    opt.zero_grad()
    F.cross_entropy(net(x), y).backward()
    opt.step()
    with torch.no_grad():
        after = net.eval()(x)
    assert net.plan is not None and not net.plan.train
    m64 = copy.deepcopy(net.module).cpu().double().eval()
    with torch.no_grad():
        ref = m64(x.cpu().double())
    err = R.rel(after, ref)
    print(f"eval after one SGD step against the float64 module on the updated parameters and statistics: {err:.2e}; the step moved the "
          f"scores by {R.rel(after, before.double()):.2e}")
    assert err <= R.FWD_BOUND and R.rel(after, before.double()) > 100 * R.FWD_BOUND


def test_momentum_none_is_the_cumulative_average(dev):
    """BatchNorm2d(momentum=None): the step uses 1 / num_batches_tracked (after the increment), as torch does; a conv with a bias in
    front of it, and a module that was lowered on sight (input shape unknown until the first call)."""
    import torch.nn as nn
    from audiopure_amd.lowering import lower_classifier
    torch.manual_seed(0)
    m = nn.Sequential(nn.Conv2d(1, 6, 3, padding=1), nn.BatchNorm2d(6, momentum=None), nn.ReLU(), nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                      nn.Linear(6, 3))
    m[1].num_batches_tracked.fill_(3)
    m64 = copy.deepcopy(m).double().train()
    net = lower_classifier(m.to(dev).train())
    assert isinstance(net, NativeConvNet) and net.training
    x = torch.randn(5, 1, 8, 8)
    y = torch.arange(5) % 3
    F.cross_entropy(net(x.to(dev)), y.to(dev)).backward()
    F.cross_entropy(m64(x.double()), y).backward()
    assert int(m[1].num_batches_tracked) == 4
    for k, q in m64.named_parameters():
        g = dict(m.named_parameters())[k].grad
        scale = float(m64[0].weight.grad.abs().max()) if k == "0.bias" else None      # (an exact zero: the BatchNorm removes the mean)
        assert R.rel(g, q.grad, scale) <= R.GRAD_BOUND, k
    assert R.rel(m[1].running_mean, m64[1].running_mean) <= R.FWD_BOUND and R.rel(m[1].running_var, m64[1].running_var) <= R.FWD_BOUND


def test_two_identical_steps_give_equal_bits(dev):
    a_net, x, y = native("dpn", dev)
    b_net, _, _ = native("dpn", dev)
    a, b = step(a_net, x, y), step(b_net, x, y)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["dx"], b["dx"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    for k in a["running"]:
        assert torch.equal(a["running"][k], b["running"][k]), k


def test_live_dropout_and_other_precisions_raise_under_strict(dev):
    import synth_convnets as S
    vgg = NativeConvNet(S.vgg19_bn(10, 1, width_div=8).to(dev), R.CHW).train()
    x = R.case("resnext")[2].to(dev)
    with pytest.raises(N.NativeError, match="dropout"):
        vgg(x)
    net, x, _ = native("wideresnet", dev)
    net.set_precision("f32s")
    with pytest.raises(N.NativeError, match="f32"):
        net(x)
    net.set_precision("f32")
    with pytest.raises(NotImplementedError, match="double backward"):
        xs = x.clone().requires_grad_(True)
        g, = torch.autograd.grad(net(xs).sum(), xs, create_graph=True)
