"""NativeConvNet in train() mode with live dropout on the device, under AUDIOPURE_STRICT=1 as the suite sets it: the eighth-width
VGG19-BN (nn.Dropout() twice, p = 0.5) and the depth-10 WideResNet with F.dropout(p = 0.3) in each block, B = 4, 1 x 32 x 32, under
``set_dropout(("philox", seed, 7))``.  Logits, loss, running statistics after one and two steps, every parameter gradient and dx against
the float64 restatement of convnet_dropout_restate.py AT THIS RUN'S ReLU DECISIONS and against the reference's own numbers (the golden)
within FWD_BOUND / GRAD_BOUND; equal bits of two runs; the seed matters; "philox" under torch.manual_seed; the no_grad forward; the
eval forward; set_dropout(None).  On the parent commit NativeConvNet has no set_dropout."""
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
import convnet_dropout_restate as D  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(D.CASES)
STREAM = ("philox", D.DROP_SEED, D.SAMPLE_OFFSET)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available() and convnet.strict()
    return torch.device("cuda:0")


def native(name, dev, spec=STREAM):
    m, _, x, y = D.case(name)
    net = NativeConvNet(copy.deepcopy(m).to(dev), D.CHW).train().set_dropout(spec)
    return net, x.to(dev), y.to(dev)


def step(net, x, y):
    """zero_grad + forward + CrossEntropyLoss + backward -> the dict of convnet_train_restate.train_step"""
    for q in net.module.parameters():
        q.grad = None
    xs = x.clone().requires_grad_(True)
    logits = net(xs)
    assert type(logits.grad_fn).__name__ == "_ConvNetTrainFnBackward"   # the HIP route, not the caller's module
    assert any(s.kind == "drop" for s in net._train_plan.steps)
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
    plan = D.case(name)[1]
    g1, g2, _ = D.reference_at(name, D.golden_flips(name))
    for n_step in (1, 2):
        got = step(net, x, y)
        assert all(g is not None and torch.isfinite(g).all() for g in got["grads"].values())
        flips = D.flips_of(name, got["masks"])
        r1, r2, decided = D.reference_at(name, flips)
        print(f"{name} step {n_step}: ReLU decisions other than float64's: {flips}")
        assert decided == 0, "a ReLU input that is not within the forward bound of 0 was decided the other way"
        ref = (r1, r2)[n_step - 1]
        fwd, grad = D.compare(got, ref, plan)
        gf, gg = D.compare_golden(got, name, n_step, plan, ref, (g1, g2)[n_step - 1])
        print(f"{name} step {n_step}: against float64: forward {fwd:.2e} (bound {D.FWD_BOUND:.2e}), gradients {grad:.2e} (bound "
              f"{D.GRAD_BOUND:.2e}); against the reference's float32 numbers: forward {gf:.2e}, gradients {gg:.2e}")
        assert fwd <= D.FWD_BOUND and grad <= D.GRAD_BOUND
        assert gf <= D.FWD_BOUND and gg <= D.GRAD_BOUND
        for k, v in ref["running"].items():
            if k.endswith("num_batches_tracked"):
                assert int(got["running"][k]) == int(v) == 100 + n_step


@pytest.mark.parametrize("name", NAMES)
def test_equal_bits_and_what_changes_them(dev, name):
    a_net, x, y = native(name, dev)
    b_net, _, _ = native(name, dev)
    a, b = step(a_net, x, y), step(b_net, x, y)
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["dx"], b["dx"])
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
    for k in a["running"]:
        assert torch.equal(a["running"][k], b["running"][k]), k
    # the no_grad train forward applies the same masks: the grad forward's bits, and the statistics move alike
    c_net, _, _ = native(name, dev)
    with torch.no_grad():
        out = c_net(x)
    assert not out.requires_grad and torch.equal(out, a["logits"])
    for k, v in a["running"].items():
        assert torch.equal(c_net.module.state_dict()[k], v), k
    # another seed, another offset: other logits
    for spec in (("philox", D.DROP_SEED + 1, D.SAMPLE_OFFSET), ("philox", D.DROP_SEED, 0)):
        d_net, _, _ = native(name, dev, spec)
        with torch.no_grad():
            assert R.rel(d_net(x), a["logits"].double()) > 100 * D.FWD_BOUND


def test_philox_reproduces_under_manual_seed(dev):
    outs = []
    for seed in (3, 3, 4):
        net, x, y = native("wideresnetD", dev, "philox")
        torch.manual_seed(seed)
        with torch.no_grad():
            outs.append(net(x).clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    net, x, y = native("wideresnetD", dev, "philox")
    torch.manual_seed(3)
    with torch.no_grad():
        first, second = net(x).clone(), net(x).clone()           # every forward draws anew
    assert not torch.equal(first, second)


@pytest.mark.parametrize("name", NAMES)
def test_eval_is_unaffected_and_none_restores_the_raise(dev, name):
    net, x, y = native(name, dev, None)
    with torch.no_grad():
        plain = net.eval()(x).clone()
        with_spec = net.set_dropout(STREAM).eval()(x).clone()
    assert torch.equal(plain, with_spec)
    net.train()
    out = net(x.clone().requires_grad_(True))
    assert type(out.grad_fn).__name__ == "_ConvNetTrainFnBackward"
    net.set_dropout(None)
    with pytest.raises(N.NativeError, match="dropout"):
        net(x)
    net.set_dropout(STREAM)
    assert type(net(x.clone().requires_grad_(True)).grad_fn).__name__ == "_ConvNetTrainFnBackward"
