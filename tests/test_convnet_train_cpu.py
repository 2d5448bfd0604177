"""The train plan of audiopure_amd.convnet (``lower(module, chw, train=True)``) and its float64 restatement
(convnet_train_restate.py), on the CPU: the plan reproduces the module's own ``.train()`` step, the restatement is pinned to the
reference's own classes (tests/golden/golden_convnet_train_v1.npz), the conditions the GPU bounds rest on hold for every case, and the
recorded bounds are what this machine measures.  The GPU tests (test_gpu_convnet_train.py) hold the kernels to this restatement."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convnet_train_restate as R  # noqa: E402
from audiopure_amd.convnet import lower  # noqa: E402

NAMES = list(R.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_train_plan_reproduces_the_modules_own_train_step_in_float64(name):
    """Forward, loss, running statistics (one and two steps) and the float64 autograd gradients of the module itself, in float64:
    only the order of a few sums differs between the plan's functionals and nn.Module's, so the two agree to 1e-9."""
    m, plan, x, y = R.case(name)
    assert plan.train and any(s.kind == "bn" for s in plan.steps) and not plan.weights          # nothing folded, nothing cloned
    m64 = copy.deepcopy(m).double()
    r1, r2, _ = R.reference(name)
    assert R.flips_of(name, R.module_masks(m64, x.double())) == ()        # the module's ReLUs, in the order they run, are the plan's
    for ref in (r1, r2):
        got = R.module_step(m64, x.double(), y)
        fwd, grad = R.compare(got, ref, plan)
        print(f"{name}: module(float64) against the restatement: forward {fwd:.2e}, gradients {grad:.2e}")
        assert fwd < 1e-9 and grad < 1e-9
        for k, v in ref["running"].items():
            if k.endswith("num_batches_tracked"):
                assert int(got["running"][k]) == int(v)


def test_train_plan_keeps_batchnorm_and_names_live_parameters():
    """BN -> ReLU sets the bn step's flag, add -> ReLU stays fused, a conv is never given a ReLU or a folded scale; every conv and bn
    step names state-dict keys of the module; the eval plan of the same module is unchanged by the flag's existence."""
    m, plan, _, _ = R.case("resnext")
    keys = set(m.state_dict())
    for s in plan.steps:
        if s.kind == "conv":
            assert not s.p["relu"] and "sk" not in s.p and s.p["wname"] in keys
        if s.kind == "bn":
            assert {s.p["wname"], s.p["bname"], s.p["rmname"], s.p["rvname"], s.p["nbtname"]} <= keys and s.p["momentum"] == 0.1
    assert any(s.kind == "bn" and s.p["relu"] for s in plan.steps) and any(s.kind == "add" and s.p["relu"] for s in plan.steps)
    ev = lower(copy.deepcopy(m).eval(), R.CHW)
    assert not ev.train and all(s.kind != "bn" for s in ev.steps) and ev.weights
    # wideresnet: the projection conv and the second 3 x 3 meet in an add with no BatchNorm between them -> the conv's epilogue adds
    _, wplan, _, _ = R.case("wideresnet")
    assert any(s.kind == "conv" and s.p["res"] is not None for s in wplan.steps)


def test_train_lowering_refuses_what_it_has_no_kernel_for():
    import torch.nn as nn
    import synth_convnets as S
    with pytest.raises(NotImplementedError, match="dropout"):
        lower(S.vgg19_bn(10, 1, width_div=8), R.CHW, train=True)
    for bn in (nn.BatchNorm2d(4, affine=False), nn.BatchNorm2d(4, track_running_stats=False)):
        net = nn.Sequential(nn.Conv2d(1, 4, 3, padding=1), bn, nn.ReLU(), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(4, 3))
        with pytest.raises(NotImplementedError):
            lower(net, (1, 8, 8), train=True)
    # momentum=None is the cumulative average: the plan says so, the restatement applies 1 / (num_batches_tracked + 1)
    net = nn.Sequential(nn.Conv2d(1, 4, 3, padding=1), nn.BatchNorm2d(4, momentum=None), nn.ReLU(), nn.AdaptiveAvgPool2d(1), nn.Flatten(),
                        nn.Linear(4, 3)).train()
    plan = lower(net, (1, 8, 8), train=True)
    assert [s.p["momentum"] for s in plan.steps if s.kind == "bn"] == [None]
    x = torch.randn(3, 1, 8, 8, dtype=torch.float64)
    net64 = copy.deepcopy(net).double()
    net64[1].num_batches_tracked.fill_(3)
    st = R.state(net64, torch.float64)
    _, running = R.run_plan(plan, st, x)
    net64(x)
    assert torch.allclose(running["1.running_var"], net64[1].running_var, rtol=1e-12, atol=0)
    assert torch.allclose(running["1.running_mean"], net64[1].running_mean, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_references_own_classes(name):
    """The golden holds float32 results of the reference's classes, and which undecided ReLU inputs that run decided the other way
    than float64; the float64 restatement at those decisions is within the float32 figures of them."""
    _, plan, _, _ = R.case(name)
    r1, r2, decided = R.reference_at(name, R.golden_flips(name))
    assert decided == 0 and len(R.golden_flips(name)) <= 2
    for step, ref in ((1, r1), (2, r2)):
        fwd, grad = R.compare_golden(ref, name, step, plan, ref)
        print(f"{name} step {step}: restatement against the reference's float32 numbers: forward {fwd:.2e}, gradients {grad:.2e}")
        assert fwd <= R.FWD_F32_ERR and grad <= R.GRAD_F32_ERR
        assert int(R.golden()[f"{name}/{step}/running/" + next(s.p["nbtname"] for s in plan.steps if s.kind == "bn")]) == 100 + step


@pytest.mark.parametrize("name", NAMES)
def test_conditions_the_gpu_bounds_rest_on(name):
    info = R.reference(name)[2]
    print(name, info)
    assert info["undecided"] <= R.MAX_UNDECIDED * info["relu_inputs"]
    assert info["min_pool_gap"] >= R.FWD_BOUND                                # no max-pool tie within the float32 error
    assert info["min_var_over_eps"] > 1.0                                      # every channel's batch variance above eps


def test_a_flipped_decision_is_what_the_decision_aware_reference_absorbs_and_nothing_else():
    """Flip one UNDECIDED input: the reference moves by percents of a tensor (what a fixed-decision comparison would have to
    tolerate) and `reference_at` follows it; flip one DECIDED input: it is counted, and the callers fail."""
    name = "resnext"
    own = R.reference(name)[2]["masks"]
    m, plan, x, y = R.case(name)
    info = {}
    R.run_plan(plan, R.state(m, torch.float64), x.double(), info)
    big = int(torch.nonzero(own[4].reshape(-1))[0])                          # a ReLU input that is clearly on
    r1, _, decided = R.reference_at(name, ((4, (big,)),))
    assert decided == 1
    _, grad = R.compare(r1, R.reference(name)[0], plan)
    assert grad > 100 * R.GRAD_BOUND


def test_recorded_bounds_are_what_float32_torch_measures():
    """FWD_BOUND / GRAD_BOUND = 4 x the float32-torch error against the float64 restatement, maximised over the cases: re-measured
    here; the bounds must hold for the measurement, and the recorded figures must not exceed it by more than the same factor."""
    worst_f = worst_g = 0.0
    for name in NAMES:
        f, g = R.measure_f32(name)
        print(f"{name}: float32 torch against float64: forward {f:.2e}, gradients {g:.2e}")
        worst_f, worst_g = max(worst_f, f), max(worst_g, g)
    assert worst_f <= R.FWD_BOUND and R.FWD_F32_ERR <= 4 * worst_f        # (another CPU's float32 sums round, and decide ReLUs, differently:
    assert worst_g <= R.GRAD_BOUND and R.GRAD_F32_ERR <= 4 * worst_g      # the recorded figure is held to a factor of 4 either way)
    assert R.FWD_BOUND == 4 * R.FWD_F32_ERR and R.GRAD_BOUND == 4 * R.GRAD_F32_ERR


def test_batchnorm_unit_bounds_are_what_float32_torch_measures_on_their_own_cases():
    """test_gpu_bn2d_train.F32_ERR, re-measured: each case's bound (4 x the recorded figure) holds for float32 torch here, and no
    recorded figure exceeds the measurement by more than the same factor."""
    import test_gpu_bn2d_train as T
    assert set(T.F32_ERR) == set(T.CASES)
    for name in T.CASES:
        f, g = T.measure_f32(name)
        print(f"{name}: float32 torch against float64: forward {f:.2e}, backward {g:.2e}")
        assert f <= 4 * T.F32_ERR[name][0] <= 16 * f and g <= 4 * T.F32_ERR[name][1] <= 16 * g


def test_a_batchnorm_reached_twice_is_refused():
    import torch.nn as nn

    class Twice(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.bn, self.fc = nn.Conv2d(1, 4, 3, padding=1), nn.BatchNorm2d(4), nn.Linear(4, 3)

        def forward(self, x):
            return self.fc(torch.relu(self.bn(torch.relu(self.bn(self.conv(x))))).mean((2, 3)))

    with pytest.raises(NotImplementedError, match="twice"):
        lower(Twice(), (1, 8, 8), train=True)
    assert lower(Twice().eval(), (1, 8, 8)) is not None              # the eval plan folds both applications, as before
