"""The train plan with live dropout on the CPU: what ``lower(..., train=True, dropout=True)`` yields for the VGG (nn.Dropout) and the
WideResNet (F.dropout), what it still refuses, and the float64 restatement of tests/convnet_dropout_restate.py pinned to each module's
own float32 step and to the reference's own classes (the golden), both with F.dropout patched to ap_dropout's masks; the conditions
and recorded bounds test_gpu_convnet_dropout.py rests on."""
import copy
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnet_train_restate as R  # noqa: E402
import convnet_dropout_restate as D  # noqa: E402
import synth_convnets as S  # noqa: E402
from audiopure_amd.convnet import NativeConvNet, lower  # noqa: E402

NAMES = list(D.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_lowering_yields_the_drop_steps(name):
    m, plan, _, _ = D.case(name)
    drops = [s for s in plan.steps if s.kind == "drop"]
    assert [s.p["p"] for s in drops] == D.DROPS[name] and [s.p["draw"] for s in drops] == list(range(len(drops)))
    # one per nn.Dropout of the VGG (2), one per block of the WideResNet (depth 10: (10 - 4) / 6 = 1 block in each of the 3 stacks)
    n_mod = sum(isinstance(q, nn.Dropout) for q in m.modules()) if name == "vgg" else sum(isinstance(q, S._WideBlock) for q in m.modules())
    assert len(drops) == n_mod == {"vgg": 2, "wideresnetD": 3}[name]
    assert all(s.out.full and s.ins[0].full for s in drops)
    with pytest.raises(NotImplementedError):
        lower(m, D.CHW, train=True)                              # without the keyword: today's refusal
    if name == "vgg":
        with pytest.raises(NotImplementedError, match=r"live dropout \(nn.Dropout\(p > 0\) in train\(\) mode\) has no kernel"):
            lower(m, D.CHW, train=True)
    assert not any(s.kind == "drop" for s in lower(m, D.CHW).steps)                       # eval: inert, with or without the keyword
    assert not any(s.kind == "drop" for s in lower(m, D.CHW, dropout=True).steps)
    assert F.dropout is torch.nn.functional.dropout and F.dropout.__module__ == "torch.nn.functional"   # the trace's patch is gone


def test_what_the_drop_step_refuses():
    class Sliced(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(1, 8, 3, padding=1)
            self.fc = nn.Linear(4, 3)

        def forward(self, x):
            y = F.dropout(self.conv(x)[:, 2:6], 0.25, self.training)                      # a channel slice of a wider buffer
            return self.fc(y.mean((2, 3)))
    with pytest.raises(NotImplementedError, match="channel slice"):
        lower(Sliced(), (1, 8, 8), train=True, dropout=True)
    for mod in (nn.Dropout2d(0.2), nn.AlphaDropout(0.2)):
        net = nn.Sequential(nn.Conv2d(1, 4, 3), mod, nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(4, 3))
        with pytest.raises(NotImplementedError, match=type(mod).__name__):
            lower(net, (1, 8, 8), train=True, dropout=True)
        with pytest.raises(NotImplementedError, match="live dropout"):
            lower(net, (1, 8, 8), train=True)
    inert = nn.Sequential(nn.Conv2d(1, 4, 3), nn.Dropout(0.0), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(4, 3))
    assert not any(s.kind == "drop" for s in lower(inert, (1, 8, 8), train=True, dropout=True).steps)


def test_set_dropout_validates_and_keys_the_train_plan():
    net = NativeConvNet(D.CASES["vgg"](), D.CHW)
    assert net._dropout is None and net._dropout_stream() is None
    for bad in ("mt", ("philox", 1), ("mt", 1, 0), ("philox", 1, -1)):
        with pytest.raises(ValueError):
            net.set_dropout(bad)
    assert net.set_dropout(("philox", 5, 7)) is net and net._dropout_stream() == dict(seed=5, offset=7)
    net.set_dropout("philox")
    torch.manual_seed(3)
    a = net._dropout_stream()
    torch.manual_seed(3)
    b = net._dropout_stream()
    assert a == b and a["offset"] == 0 and a != net._dropout_stream()
    x = torch.zeros((2,) + D.CHW)
    assert any(s.kind == "drop" for s in net.train()._train_plan_for(x).steps)
    net.set_dropout(None)
    with pytest.raises(NotImplementedError, match="dropout"):
        net._train_plan_for(x)                                   # toggling re-lowers: the refusal is back
    assert net._train_plan is None


@pytest.mark.parametrize("name", NAMES)
def test_conditions_the_gpu_bounds_rest_on(name):
    info = D.reference(name)[2]
    print(name, {k: v for k, v in info.items() if k != "masks"})
    assert D.find_seed(name) == D.SEED[name]                     # the first seed at which the restatement alone meets them
    assert info["undecided"] <= D.MAX_UNDECIDED * info["relu_inputs"]
    assert info["min_pool_gap"] >= D.FWD_BOUND
    assert info["min_var_over_eps"] > 1.0


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_modules_own_patched_float32_step(name):
    f, g = D.measure_f32(name)
    print(f"{name}: patched float32 torch against float64: forward {f:.2e}, gradients {g:.2e}")
    assert f <= D.FWD_BOUND and g <= D.GRAD_BOUND                # (another CPU's float32 sums round differently: within the bound itself)
    # in float64 the module's own patched step IS the restatement
    m, plan, x, y = D.case(name)
    m64 = copy.deepcopy(m).double()
    got = D.module_step(m64, x.double(), y)
    f64, g64 = D.compare(got, D.reference(name)[0], plan)
    assert f64 <= 1e-12 and g64 <= 1e-10


def test_recorded_bounds_are_what_was_measured():
    worst = [max(v) for v in zip(*(D.measure_f32(n) for n in NAMES))]
    assert worst[0] <= D.FWD_BOUND and D.FWD_F32_ERR <= 4 * worst[0]          # (another CPU's float32 sums round differently: the recorded
    assert worst[1] <= D.GRAD_BOUND and D.GRAD_F32_ERR <= 4 * worst[1]        # figure is held to a factor of 4 either way, as in 3.12)
    assert D.FWD_BOUND == 4 * D.FWD_F32_ERR and D.GRAD_BOUND == 4 * D.GRAD_F32_ERR


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_references_own_classes(name):
    _, plan, _, _ = D.case(name)
    r1, r2, decided = D.reference_at(name, D.golden_flips(name))
    assert decided == 0
    G = D.golden()
    for step, ref in ((1, r1), (2, r2)):
        got = dict(ref)
        f, g = D.compare_golden(got, name, step, plan, ref)
        print(f"{name} step {step}: float64 restatement against the reference's float32 numbers: forward {f:.2e}, gradients {g:.2e}")
        assert f <= D.FWD_F32_ERR * 1.05 and g <= D.GRAD_F32_ERR * 1.05
        for k, v in ref["running"].items():
            if k.endswith("num_batches_tracked"):
                assert int(G[f"{name}/{step}/running/{k}"]) == int(v)


def test_the_masks_matter():
    """another stream gives other logits, and the restatement without the drop steps is not the restatement"""
    m, plan, x, y = D.case("wideresnetD")
    st = R.state(m, torch.float64)
    with torch.no_grad():
        a, _ = D.run_plan(plan, st, x.double())
        b, _ = D.run_plan(plan, st, x.double(), seed=D.DROP_SEED + 1)
        c, _ = D.run_plan(plan, st, x.double(), offset=0)
    assert R.rel(b, a) > 1e-3 and R.rel(c, a) > 1e-3
