"""The native optimizer step (audiopure_amd/optim.py on csrc/ap_optim.hip) where its kernel branches, against the float64 restatement
of tests/optim_restate.py within that file's bounds: tensor sizes around the chunk (c = ap_optim_chunk()), tensor counts around the
slab (S = ap_optim_slab()), 16-byte-aligned tensors (the float4 path) and views at 4-, 8- and 12-byte offsets with parameter and
gradient misaligned differently (the per-element path), every tensor between sentinel-filled guard elements."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import optim_restate as R
from audiopure_amd import _native as N
from audiopure_amd import optim

pytestmark = pytest.mark.gpu

GUARD = 8                                                     # elements on either side of every placed tensor
SENTINEL = -123456.75                                         # exactly representable; any write shows


@functools.lru_cache(maxsize=None)
def _cs():
    return R.chunk_and_slab()


@functools.lru_cache(maxsize=None)
def _table(name):
    return R.Table(name, *_cs())


@functools.lru_cache(maxsize=None)
def _reference(kind, name, n_ema):
    """computed once per case, shared and never written"""
    return R.run_restate(kind, _table(name), n_ema)


class Placer:
    """puts tensor i into its own sentinel-filled buffer: `aligned` at a 16-byte boundary, `views` at byte offset 4 k with
    k = (i + shift) % 4 for parameters and a different k for gradients"""

    def __init__(self, align, is_grad):
        self.align, self.is_grad, self.held = align, is_grad, []

    def offset(self, i):
        if self.align == "aligned":
            return 0
        kp = i % 4
        return (kp + 1 + (i // 4) % 3) % 4 if self.is_grad else kp

    def __call__(self, i, array):
        n, k = array.size, self.offset(i)
        buf = torch.full((n + 2 * GUARD + 4,), SENTINEL, dtype=torch.float32, device="cuda")
        view = buf[GUARD + k:GUARD + k + n]
        view.copy_(torch.from_numpy(array).to(torch.float32))
        assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * k
        self.held.append((buf, GUARD + k, n))
        return view

    def check_guards(self):
        for buf, lo, n in self.held:
            b = buf.cpu()
            assert bool((b[:lo] == SENTINEL).all()) and bool((b[lo + n:] == SENTINEL).all()), "a guard element was written"


def _set_lr(opt, base, step):
    for g, lr in zip(opt.param_groups, base):
        g["lr"] = lr * (0.5 if step >= 2 else 1.0)


def run_native(kind, name, n_ema, align, steps=R.STEPS):
    table = _table(name)
    cls, common, _ = R.KINDS[kind]
    pp, gp = Placer(align, False), Placer(align, True)
    params = R.make_params(table, torch.float32, place=pp)
    opt = getattr(optim, cls)(R.param_groups(kind, table, params), **common)
    emas = [opt.track_ema(R.EMA_RATES[k]) for k in range(n_ema)]
    base = [g["lr"] for g in opt.param_groups]
    for s in range(steps):
        _set_lr(opt, base, s)
        R.set_grads(table, params, s, place=gp)
        opt.step()
    torch.cuda.synchronize()
    pp.check_guards()
    gp.check_guards()
    for i, p in enumerate(params):                            # a view is what the kernel was handed
        if align == "views" and p.grad is not None:
            assert p.data_ptr() % 16 != p.grad.data_ptr() % 16
    return R.collect(opt, params, emas), opt, params


def _bits(res):
    out = [p.astype(np.float32).view(np.int32) for p in res["params"]]
    out += [e.astype(np.float32).view(np.int32) for es in res["emas"] for e in es]
    out += [v.astype(np.float32).view(np.int32) for st in res["states"] for k, v in sorted(st.items()) if k != "step"]
    return out


def _assert_within(kind, table, got, ref, what):
    err = R.compare(kind, table, got, ref)
    pb = R.SGD_BOUND if R.KINDS[kind][0] == "SGD" else R.ADAM_BOUND
    print(f"{what}: param {err['param']:.2e} (bound {pb:.2e})  state {err['state']:.2e} (bound {R.STATE_BOUND:.2e})  "
          f"ema {err['ema']:.2e} (bound {R.EMA_BOUND:.2e})")
    assert err["param"] <= pb and err["state"] <= R.STATE_BOUND and err["ema"] <= R.EMA_BOUND, err


# n_ema of the (aligned, views) run of each kind: 0, 1 and 4 tracked rates on either path
N_EMA = {"adam": (0, 1), "adamw": (4, 1), "sgd": (1, 4), "sgd0": (0, 4)}


@pytest.mark.parametrize("kind", list(R.KINDS))
@pytest.mark.parametrize("name", R.table_names())
def test_three_steps_against_the_float64_restatement(name, kind):
    table = _table(name)
    for align, n_ema in zip(("aligned", "views"), N_EMA[kind]):
        got, opt, params = run_native(kind, name, n_ema, align)
        ref = _reference(kind, name, n_ema)
        _assert_within(kind, table, got, ref, f"{name} {kind} {align} n_ema={n_ema}")
        if table.zero >= 0:
            z, none = table.zero, table.none
            p0 = [p.astype(np.float32) for p in table.p0]
            # all-zero gradients at wd = 0: the bits stay; no grad: the bits stay and there is no state; its EMA copies move
            assert np.array_equal(got["params"][z].astype(np.float32).view(np.int32), p0[z].view(np.int32))
            assert np.array_equal(got["params"][none].astype(np.float32).view(np.int32), p0[none].view(np.int32))
            assert params[none] not in opt.state
            for es, rs in zip(got["emas"], ref["emas"]):
                assert np.abs(es[none] - rs[none]).max() <= R.EMA_BOUND * np.abs(rs[none]).max()
        again, _, _ = run_native(kind, name, n_ema, align)
        assert all(np.array_equal(a, b) for a, b in zip(_bits(got), _bits(again))), "two runs differ in bits"


def run_torch_on_the_device(kind, name, n_ema):
    """the same three steps by torch.optim on the device (its default path there), the EMA copies by the reference's update_ema"""
    table = _table(name)
    cls, common, _ = R.KINDS[kind]
    params = R.make_params(table, torch.float32, device="cuda")
    opt = getattr(torch.optim, cls)(R.param_groups(kind, table, params), **common)
    emas = [[p.detach().clone() for p in params] for _ in range(n_ema)]
    base = [g["lr"] for g in opt.param_groups]
    for s in range(R.STEPS):
        _set_lr(opt, base, s)
        R.set_grads(table, params, s)
        opt.step()
        for k in range(n_ema):
            R.reference_update_ema(emas[k], params, R.EMA_RATES[k])
    return R.collect(opt, params, emas)


@pytest.mark.parametrize("kind", list(R.KINDS))
@pytest.mark.parametrize("name", ["sizes", "2S+1"])
def test_native_step_has_the_bits_of_torch_optim_on_the_device(name, kind):
    """The kernel pins the rounding sequence of torch.optim's default path on the device (one fma per add(alpha) / lerp / addcmul /
    addcdiv, a rounding after every operator, correctly rounded sqrt and divide), on the float4 path and on the per-element path:
    parameters, state and EMA copies after three steps are torch's bit for bit.  That is what lets a native loop run beside a
    torch.optim loop (tests/test_gpu_optim_models.py): where a gradient entry is rounding noise around Adam's eps, a single differing
    last bit of a parameter decides the sign of the next update."""
    ref = _bits(run_torch_on_the_device(kind, name, 2))
    for align in ("aligned", "views"):
        got = _bits(run_native(kind, name, 2, align)[0])
        assert len(got) == len(ref)
        differing = sum(int((a != b).sum()) for a, b in zip(got, ref))
        print(f"{name} {kind} {align}: {differing} of {sum(a.size for a in ref)} entries differ from torch.optim's bits")
        assert differing == 0


def test_lerp_at_a_weight_above_one_half_has_torchs_bits_too():
    """beta1 = 0.3: torch's lerp takes its other form at weights of 0.5 and above (end - (end - start)(1 - weight), one fma)"""
    table = _table("S+1")
    results = []
    for module in (torch.optim, optim):
        params = R.make_params(table, torch.float32, device="cuda")
        opt = module.Adam(params, lr=1e-3, betas=(0.3, 0.999), weight_decay=1e-2)
        for s in range(R.STEPS):
            R.set_grads(table, params, s)
            opt.step()
        results.append(_bits(R.collect(opt, params, [])))
    assert sum(int((a != b).sum()) for a, b in zip(*results)) == 0


def test_a_parameter_whose_grad_becomes_none_keeps_its_bits_and_its_step():
    table = _table("sizes")
    params = R.make_params(table, torch.float32, place=Placer("views", False))
    opt = optim.Adam(params, lr=1e-3, weight_decay=1e-2)
    ema = opt.track_ema(0.9)
    R.set_grads(table, params, 0)
    params[1].grad = torch.ones_like(params[1])
    opt.step()
    idx = 5                                                   # c elements: more than the tail path
    keep = [t.clone() for t in (params[idx], opt.state[params[idx]]["exp_avg"], opt.state[params[idx]]["exp_avg_sq"])]
    e0 = ema[idx].clone()
    versions = (params[idx]._version, opt.state[params[idx]]["exp_avg"]._version, ema[idx]._version)
    R.set_grads(table, params, 1)
    params[1].grad = torch.ones_like(params[1])
    params[idx].grad = None
    opt.step()
    st = opt.state[params[idx]]
    assert st["step"].item() == 1 and opt.state[params[0]]["step"].item() == 2
    assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
    for a, b in zip(keep, (params[idx], st["exp_avg"], st["exp_avg_sq"])):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    want = 0.9 * e0.double() + (1 - 0.9) * params[idx].detach().double()
    assert float((ema[idx].double() - want).abs().max()) <= R.EMA_BOUND * float(want.abs().max())
    assert not torch.equal(ema[idx], e0)
    # untouched tensors keep their version; the EMA copy, which was written, does not
    assert (params[idx]._version, st["exp_avg"]._version) == versions[:2] and ema[idx]._version > versions[2]


def test_version_counters_follow_every_written_tensor():
    table = _table("S+1")
    for kind in ("adamw", "sgd"):
        cls, common, _ = R.KINDS[kind]
        params = R.make_params(table, torch.float32, device="cuda")
        opt = getattr(optim, cls)(R.param_groups(kind, table, params), **common)
        ema = opt.track_ema(0.99)
        R.set_grads(table, params, 0)
        opt.step()
        v1 = [[p._version for p in params], [e._version for e in ema],
              [[t._version for k, t in sorted(opt.state[p].items()) if k != "step"] for p in params if p in opt.state]]
        R.set_grads(table, params, 1)
        opt.step()
        v2 = [[p._version for p in params], [e._version for e in ema],
              [[t._version for k, t in sorted(opt.state[p].items()) if k != "step"] for p in params if p in opt.state]]
        for i, (a, b) in enumerate(zip(v1[0], v2[0])):
            assert (b == a) if i == table.none else (b > a), (kind, i, a, b)
        assert all(b > a for a, b in zip(v1[1], v2[1]))
        assert v2[2] and all(b > a for sa, sb in zip(v1[2], v2[2]) for a, b in zip(sa, sb))


@pytest.mark.parametrize("name", ["sizes", "2S+1"])
def test_grad_sqnorm_against_numpy_float64(name):
    table = _table(name)
    for align in ("aligned", "views"):
        gp = Placer(align, True)
        params = R.make_params(table, torch.float32, device="cuda")
        opt = optim.SGD(params, lr=0.1)
        R.set_grads(table, params, 0, place=gp)
        ref = R.sqnorm(table.grads[0])
        a = opt.grad_sqnorm()
        b = opt.grad_sqnorm()
        assert a.dtype == torch.float64 and a.shape == (1,) and a.is_cuda
        rel = abs(a.item() - ref) / ref
        print(f"{name} {align}: sum g^2 = {a.item():.17g}, numpy {ref:.17g}, relative {rel:.2e} (bound {R.SQNORM_BOUND:.0e})")
        assert sum(g.size for g in table.grads[0] if g is not None) <= 1e5
        assert rel <= R.SQNORM_BOUND
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert opt.grad_norm() == math.sqrt(a.item())
        gp.check_guards()
    for p in params:
        p.grad = None
    assert opt.grad_sqnorm().item() == 0.0


def test_update_ema_function():
    """the stand-alone update_ema (the EMA-only launch kind) on views, against the restatement; the sources are not written"""
    targets, sources = R.golden_ema_inputs()
    tp, sp = Placer("views", False), Placer("views", True)
    targ = [tp(i, t) for i, t in enumerate(targets)]
    ref = [t.copy() for t in targets]
    for call, src in enumerate(sources):
        s = [sp(i, a) for i, a in enumerate(src)]
        before = [t.clone() for t in s]
        versions = [t._version for t in targ]
        if call == 0:
            optim.update_ema(targ, s)                         # the reference's default rate, 0.99
        else:
            optim.update_ema(targ, s, rate=0.9999)
        R.ema_update(ref, [a.astype(np.float32).astype(np.float64) for a in src], 0.99 if call == 0 else 0.9999)
        assert all(torch.equal(a, b) for a, b in zip(before, s))
        assert all(t._version > v for t, v in zip(targ, versions))
    worst = max(float(np.abs(t.double().cpu().numpy() - r).max() / np.abs(r).max()) for t, r in zip(targ, ref))
    print(f"update_ema: {worst:.2e} (bound {R.EMA_BOUND:.2e})")
    assert worst <= R.EMA_BOUND
    tp.check_guards()
    sp.check_guards()
    with pytest.raises(N.NativeError):
        optim.update_ema([torch.zeros(4)], [torch.zeros(4)])


@pytest.mark.parametrize("direction", ["native_to_torch", "torch_to_native"])
def test_state_dict_moves_between_native_and_torch_adam(direction):
    """two steps on one side, the state_dict loaded into the other, step 3 there: within the Adam bound of the three-step restatement"""
    name, kind = "S+1", "adam"
    table = _table(name)
    first, second = (optim.Adam, torch.optim.Adam) if direction == "native_to_torch" else (torch.optim.Adam, optim.Adam)
    params = R.make_params(table, torch.float32, device="cuda")
    a = first(R.param_groups(kind, table, params))
    base = [g["lr"] for g in a.param_groups]
    for s in range(2):
        R.set_grads(table, params, s)
        a.step()
    sd = a.state_dict()
    assert all(v["step"].device.type == "cpu" for v in sd["state"].values())
    b = second(R.param_groups(kind, table, params))
    b.load_state_dict(sd)
    _set_lr(b, base, 2)
    R.set_grads(table, params, 2)
    b.step()
    _assert_within(kind, table, R.collect(b, params, []), _reference(kind, name, 0), direction)


def test_step_refuses_sparse_and_non_contiguous_grads():
    p = torch.nn.Parameter(torch.ones(4, 6, device="cuda"))
    opt = optim.Adam([p])
    p.grad = torch.ones(6, 4, device="cuda").t()
    with pytest.raises(N.NativeError, match="contiguous"):
        opt.step()
    p.grad = torch.ones(4, 6, device="cuda").to_sparse()
    with pytest.raises(N.NativeError, match="sparse"):
        opt.step()
    assert p not in opt.state or opt.state[p]["step"].item() == 0
    assert torch.equal(p.detach(), torch.ones(4, 6, device="cuda"))
    with pytest.raises(N.NativeError, match="HIP device"):
        optim.SGD([torch.nn.Parameter(torch.ones(4, 6, device="cuda").t())], lr=0.1)
    with pytest.raises(N.NativeError, match="HIP device"):
        optim.SGD([torch.nn.Parameter(torch.ones(4, device="cuda", dtype=torch.float64))], lr=0.1)


def test_c_entry_points_refuse_bad_arguments():
    lib = N.lib()
    buf = torch.zeros(64, device="cuda")
    addr = buf.data_ptr()

    def call(hyper, **fields):
        t = N.ApOptimTensor(param=addr, grad=addr, state1=addr, state2=addr, n=4, step_size=1e-3, sqrt_bc2=1.0)
        for k in range(N.AP_OPTIM_MAX_EMA):
            t.ema[k] = addr
        for k, v in fields.items():
            setattr(t, k, v)
        h = N.ApOptimHyper(kind=N.AP_OPTIM_ADAM, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
        for k, v in hyper.items():
            setattr(h, k, v)
        return lib.ap_optim_step(C.byref(t), 1, C.byref(h), N.stream()), lib.ap_last_error()

    for hyper, fields, word in ((dict(kind=7), {}, b"kind"), (dict(n_ema=5), {}, b"n_ema"), (dict(beta1=1.0), {}, b"betas"),
                                (dict(beta2=1.5), {}, b"betas"), (dict(lr=-1e-3), {}, b"negative"), (dict(eps=-1.0), {}, b"negative"),
                                (dict(weight_decay=-1.0), {}, b"negative"), ({}, dict(param=None), b"null"),
                                ({}, dict(state2=None), b"null")):
        rc, msg = call(hyper, **fields)
        assert rc == -22 and word in msg, (hyper, fields, rc, msg)
    h = N.ApOptimHyper(kind=N.AP_OPTIM_ADAM, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    assert lib.ap_optim_step(None, 1, C.byref(h), N.stream()) == -22
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                      # nothing ran
    with pytest.raises(N.NativeError):
        N.check(lib.ap_optim_sqnorm(None, None, 1, addr, 64, addr, N.stream()), "ap_optim_sqnorm")
