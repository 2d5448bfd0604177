"""CPU checks of tests/optim_restate.py (the float64 reference the native optimizer step is held to) and of the host side of
audiopure_amd/optim.py: the restatements equal torch.optim in float64, the EMA restatement equals the reference's update_ema
(tests/golden/golden_optim_v1.npz), the recorded float32 constants re-measure, the input condition holds, and the native classes
keep torch's state_dict layout and refuse what they do not serve."""
import os

import numpy as np
import pytest
import torch

import optim_restate as R
from audiopure_amd import _native as N
from audiopure_amd import optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cs():
    return R.chunk_and_slab()


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_restatement_equals_torch_optim_in_float64(kind, cs):
    """three steps, the lr halved before the third, one parameter's grad None, an all-zero gradient, two groups: every parameter, state
    and EMA tensor within 1e-13 of its largest entry (R.plain_err), and `compare` -- which also checks `step` and the tensors that must
    not move -- sees nothing above a few float64 ulps in its own units"""
    for name in ("sizes", "S+1"):
        table = R.Table(name, *cs)
        assert table.none == 1 and table.zero == len(table.sizes) - 1
        got, ref = R.run_torch(kind, table, torch.float64, 2), R.run_restate(kind, table, 2)
        err = R.compare(kind, table, got, ref)
        plain = R.plain_err(got, ref)
        print(kind, name, plain, err)
        assert plain <= 1e-13, plain
        assert err["param"] <= 1e-11 and err["state"] <= 1e-13 and err["ema"] <= 1e-13, err
        z = table.zero
        assert np.array_equal(got["params"][z], table.p0[z]) and np.array_equal(ref["params"][z], table.p0[z])
        assert np.array_equal(ref["params"][1], table.p0[1]) and not ref["states"][1]
        if kind != "sgd0":
            assert "step" not in ref["states"][1] and ref["states"][0]
        if kind in ("adam", "adamw"):
            assert ref["states"][0]["step"] == R.STEPS


def test_ema_restatement_equals_the_references_update_ema():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_optim_v1.npz"))
    for rate in R.GOLDEN_EMA_RATES:
        targets, sources = R.golden_ema_inputs()
        for call, src in enumerate(sources):
            R.ema_update(targets, src, 0.99 if rate is None else rate)
            for i, t in enumerate(targets):
                ref = g[f"rate_{rate}/call{call}/t{i}"]
                assert ref.dtype == np.float64 and ref.shape == t.shape
                assert np.abs(t - ref).max() <= 1e-13 * np.abs(ref).max()
    assert len(g.files) == len(R.GOLDEN_EMA_RATES) * R.STEPS * len(targets)
    # and the operator-by-operator copy the float32 measurement uses is the same function
    targets, sources = R.golden_ema_inputs()
    tt = [torch.from_numpy(t) for t in targets]
    R.reference_update_ema(tt, [torch.from_numpy(s) for s in sources[0]])
    assert all(np.array_equal(t.numpy(), g[f"rate_None/call0/t{i}"]) for i, t in enumerate(tt))


def test_recorded_constants_remeasure(cs):
    m = R.measure_f32(*cs)
    print(m)
    for key, rec in (("adam", R.ADAM_F32_ERR), ("sgd", R.SGD_F32_ERR), ("state", R.STATE_F32_ERR), ("ema", R.EMA_F32_ERR)):
        assert rec / 1.5 <= m[key] <= rec * 1.5, (key, m[key], rec)
    assert (R.ADAM_BOUND, R.SGD_BOUND, R.STATE_BOUND, R.EMA_BOUND) == (4 * R.ADAM_F32_ERR, 4 * R.SGD_F32_ERR, 4 * R.STATE_F32_ERR,
                                                                       4 * R.EMA_F32_ERR)


def test_input_condition_holds(cs):
    """every effective gradient entry is 0 or >= 1e-6 = 100 eps, in the float64 run and in torch's own float32 run"""
    zeros = 0
    for name in R.table_names():
        table = R.Table(name, *cs)
        assert sum(table.sizes) <= 1e5                        # the squared norm's bound is derived for N <= 1e5
        for kind in R.KINDS:
            run = R.run_restate(kind, table)
            R.check_condition(table, kind, run)
            R.check_condition(table, kind, R.effective_grads_f32(kind, table))
            zeros += sum(int((e == 0).sum()) for step in run["eff"] for e in step if e is not None)
    assert zeros > 0                                          # exact zeros are part of the tables
    with pytest.raises(AssertionError):
        R.check_condition(table, "adam", dict(eff=[[np.array([0.0, 1e-7])]]))


def test_sqnorm_restatement():
    g = [np.array([3.0, 4.0]), None, np.array([12.0])]
    assert R.sqnorm(g) == 169.0


# ---- host side of audiopure_amd.optim ---------------------------------------------------------------------------------------------
def _on_cpu(monkeypatch, cls, params, **kw):
    """a native optimizer over CPU tensors, for its host logic only (its step() cannot run here: there is no CPU path)"""
    monkeypatch.setattr(optim, "_check_param", lambda p, who: None)
    return cls(params, **kw)


@pytest.mark.parametrize("name,kw", [("Adam", dict(weight_decay=1e-2)), ("AdamW", {}), ("SGD", dict(lr=0.1, momentum=0.9)),
                                     ("SGD", dict(lr=0.1))])
def test_state_dict_keys_and_types_equal_torchs(monkeypatch, name, kw):
    def params():
        torch.manual_seed(0)
        return [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5))]
    pt, pn = params(), params()
    ref = getattr(torch.optim, name)(pt, **kw)
    nat = _on_cpu(monkeypatch, getattr(optim, name), pn, **kw)
    assert isinstance(nat, torch.optim.Optimizer)
    assert nat.defaults == ref.defaults
    for p in pt:
        p.grad = torch.ones_like(p)
    ref.step()
    if name != "SGD" or kw.get("momentum"):
        for p in pn:                                          # what step() does on the host before it launches
            st = nat._state_of(p)
            if "step" in st:
                st["step"] += 1
    a, b = ref.state_dict(), nat.state_dict()
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys()
        for k, v in a["state"][i].items():
            w = b["state"][i][k]
            assert type(v) is type(w) and v.dtype == w.dtype and v.device == w.device and v.shape == w.shape, (k, v, w)
        if "step" in a["state"][i]:
            assert torch.equal(a["state"][i]["step"], b["state"][i]["step"])
    # and it moves both ways
    nat.load_state_dict(a)
    ref.load_state_dict(nat.state_dict())
    for i, p in enumerate(pn):
        for k, v in ref.state[pt[i]].items():
            assert torch.equal(nat.state[p][k], v) and nat.state[p][k].device == v.device and nat.state[p][k].dtype == v.dtype


def test_lr_is_read_from_param_groups(monkeypatch):
    p = [torch.nn.Parameter(torch.ones(4))]
    nat = _on_cpu(monkeypatch, optim.Adam, p, lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(nat, step_size=1, gamma=0.5)
    nat.param_groups[0]["lr"] = 4e-3
    assert nat._hyper(nat.param_groups[0]).lr == 4e-3 and nat._hyper(nat.param_groups[0]).kind == N.AP_OPTIM_ADAM
    assert sched.optimizer is nat
    w = _on_cpu(monkeypatch, optim.AdamW, [torch.nn.Parameter(torch.ones(4))])
    assert w._hyper(w.param_groups[0]).kind == N.AP_OPTIM_ADAMW and w._hyper(w.param_groups[0]).weight_decay == 1e-2


def test_refused_arguments_raise(monkeypatch):
    def p():
        return [torch.nn.Parameter(torch.ones(4))]
    # no CPU path: a parameter that is not contiguous fp32 on a HIP device
    for cls in (optim.Adam, optim.AdamW, optim.SGD):
        with pytest.raises(N.NativeError, match="HIP device"):
            cls(p(), lr=0.1)
    monkeypatch.setattr(optim, "_check_param", lambda p, who: None)
    for cls in (optim.Adam, optim.AdamW):
        for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
            with pytest.raises(NotImplementedError, match=flag):
                cls(p(), **{flag: True})
        with pytest.raises(NotImplementedError, match="tensor lr"):
            cls(p(), lr=torch.tensor(1e-3))
        cls(p(), foreach=True, fused=True)                     # accepted and ignored
        with pytest.raises(ValueError):
            cls(p(), betas=(1.0, 0.999))
        with pytest.raises(ValueError):
            cls(p(), lr=-1.0)
    for kw, word in ((dict(nesterov=True, momentum=0.9), "nesterov"), (dict(dampening=0.1), "dampening"), (dict(maximize=True), "maximize"),
                     (dict(differentiable=True), "differentiable"), (dict(lr=torch.tensor(0.1)), "tensor lr")):
        with pytest.raises(NotImplementedError, match=word):
            optim.SGD(p(), **kw)
    optim.SGD(p(), lr=0.1, foreach=True, fused=True)
    # a flag switched on later in a param group is refused at the step, before anything runs
    o = optim.Adam(p())
    o.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError, match="amsgrad"):
        o.step()
    # at most AP_OPTIM_MAX_EMA rates
    o = optim.SGD(p(), lr=0.1)
    for r in (0.9, 0.99, 0.999, 0.9999):
        assert len(o.track_ema(r)) == 1
    with pytest.raises(N.NativeError, match="at most 4"):
        o.track_ema(0.5)
    with pytest.raises(N.NativeError, match="track_ema"):
        o.add_param_group(dict(params=p()))


def test_c_entry_points_refuse_bad_arguments_without_a_gpu():
    """every refusal comes before any launch, so it can be checked here: -22 and ap_last_error"""
    import ctypes as C
    lib = N.lib()
    assert lib.ap_optim_slab() >= 1 and lib.ap_optim_chunk() % 4 == 0
    buf = C.create_string_buffer(64)
    addr = C.addressof(buf)

    def call(hyper, **fields):
        t = N.ApOptimTensor(param=addr, grad=addr, state1=addr, state2=addr, n=4, step_size=1e-3, sqrt_bc2=1.0)
        for k in range(N.AP_OPTIM_MAX_EMA):
            t.ema[k] = addr
        for k, v in fields.items():
            setattr(t, k, v)
        h = N.ApOptimHyper(kind=N.AP_OPTIM_ADAM, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
        for k, v in hyper.items():
            setattr(h, k, v)
        return lib.ap_optim_step(C.byref(t), 1, C.byref(h), None), lib.ap_last_error()

    for hyper, fields, word in ((dict(kind=4), {}, b"kind"), (dict(kind=-1), {}, b"kind"), (dict(n_ema=5), {}, b"n_ema"),
                                (dict(beta1=1.0), {}, b"betas"), (dict(beta2=-0.1), {}, b"betas"), (dict(lr=-1e-3), {}, b"negative"),
                                (dict(eps=-1e-8), {}, b"negative"), (dict(weight_decay=-0.1), {}, b"negative"),
                                ({}, dict(param=None), b"null param"), ({}, dict(state1=None), b"null state"),
                                ({}, dict(state2=None), b"null state"), (dict(kind=N.AP_OPTIM_SGD, momentum=0.9), dict(state1=None), b"null state"),
                                (dict(kind=N.AP_OPTIM_EMA_ONLY), {}, b"n_ema")):
        rc, msg = call(hyper, **fields)
        assert rc == -22 and word in msg, (hyper, fields, rc, msg)
    t = N.ApOptimTensor(param=addr, n=4)
    h = N.ApOptimHyper(kind=N.AP_OPTIM_EMA_ONLY, n_ema=1)
    assert lib.ap_optim_step(C.byref(t), 1, C.byref(h), None) == -22 and b"null ema" in lib.ap_last_error()
    assert lib.ap_optim_step(None, 1, C.byref(h), None) == -22 and lib.ap_optim_step(C.byref(t), 1, None, None) == -22
    n = (C.c_uint64 * 2)(5, 2 * lib.ap_optim_chunk() + 1)
    assert lib.ap_optim_sqnorm_workspace_bytes(n, 2) == 8 * 4
    ptrs = (C.c_void_p * 2)(addr, None)
    assert lib.ap_optim_sqnorm(ptrs, n, 2, addr, 64, addr, None) == -22 and b"null grad" in lib.ap_last_error()
    ptrs = (C.c_void_p * 2)(addr, addr)
    assert lib.ap_optim_sqnorm(ptrs, n, 2, addr, 24, addr, None) == -22 and b"workspace" in lib.ap_last_error()
    assert lib.ap_optim_sqnorm(ptrs, n, 2, None, 64, addr, None) == -22
