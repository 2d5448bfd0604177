"""M5 in train mode on the GPU (ap_m5_train.hip through audiopure_amd.audio_models.M5.M5Net.M5 and through the C-ABI) against
the float64 restatement of m5_train_restate.py.  The case table, the clip seeds (every clip of every case is decided) and the
bounds are that module's, their conditions asserted by test_m5_train_cpu.py.  Buffers the kernels write start NaN-filled, so an
element left out fails the comparison; every refusal is returned before any launch."""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frontend_restate as FR
import m5_train_restate as T
from audiopure_amd import _native as N

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_m5_train_v1.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _module(sd, nc, no, dev):
    from audiopure_amd.audio_models.M5.M5Net import M5
    m5 = M5(n_input=1, n_output=no, n_channel=nc)
    m5.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m5.to(dev).train()


def _grads_of(m5, xg):
    got = {k: p.grad.detach().cpu() for k, p in m5.named_parameters()}
    got["x"] = xg.grad.detach().cpu()
    return got


@functools.lru_cache(maxsize=None)
def _step(shape):
    """one train-mode forward + backward of a case through the module, shared by the tests that read it"""
    dev = torch.device("cuda:0")
    B, L, nc, no = shape
    sd, x, y, _, _, _ = T.reference(shape)
    m5 = _module(sd, nc, no, dev)
    xg = x.to(dev).requires_grad_(True)
    out = m5(xg)
    loss = F.nll_loss(out, y.to(dev))
    loss.backward()
    return m5, out.detach().cpu(), float(loss.detach()), _grads_of(m5, xg)


@pytest.mark.parametrize("shape", T.SHAPES)
def test_train_forward_matches_float64(dev, shape):
    """model.train(); model(x): log-probabilities from batch statistics, the running statistics moved with momentum 0.1 and
    the unbiased variance (n / (n - 1): 4 / 3 in stage 4 of the first case), num_batches_tracked counted."""
    _, _, _, ref, _, _ = T.reference(shape)
    m5, out, _, _ = _step(shape)
    err = float((out.double() - ref["logp"].detach()).abs().max())
    rerr = max(float((dict(m5.named_buffers())[k].cpu().double() - v).abs().max()) for k, v in ref["running"].items())
    print(f"m5 train forward {shape}: max |d logp| = {err:.2e}, max |d running| = {rerr:.2e} (bound {T.FWD_BOUND:.2e})")
    assert err <= T.FWD_BOUND and rerr <= T.FWD_BOUND
    assert all(int(bn.num_batches_tracked) == 101 for bn in m5._bns())


def test_momentum_none_averages_and_no_grad_moves_the_statistics(dev):
    shape = T.SHAPES[2]
    B, L, nc, no = shape
    sd, x, _, _, _, _ = T.reference(shape)
    m5 = _module(sd, nc, no, dev)
    for bn in m5._bns():
        bn.momentum = None                                                   # cumulative average: m = 1 / num_batches_tracked
    with torch.no_grad():
        out = m5(x.to(dev))
        ref = T.forward(T.tensors(sd, torch.float64, False), x.double(), momentum=1.0 / 101)
    assert out.grad_fn is None and m5._train_forward(x.to(dev), keep=False)[1] is None      # nothing kept for a backward
    assert float((out.cpu().double() - ref["logp"]).abs().max()) <= T.FWD_BOUND
    assert all(int(bn.num_batches_tracked) == 102 for bn in m5._bns())
    # the second call above moved them again, with m = 1 / 102, from the first call's values
    t = T.tensors(sd, torch.float64, False)
    t.update(ref["running"])
    ref2 = T.forward(t, x.double(), momentum=1.0 / 102)["running"]
    for k, v in ref2.items():
        assert float((dict(m5.named_buffers())[k].cpu().double() - v).abs().max()) <= T.FWD_BOUND, k
        assert float((v - torch.as_tensor(sd[k]).double()).abs().max()) > T.FWD_BOUND           # they did move
    # the no_grad forward is the grad-mode forward's value, bit for bit
    m5b = _module(sd, nc, no, dev)
    for bn in m5b._bns():
        bn.momentum = None
    assert torch.equal(m5b(x.to(dev)).detach(), out)


@pytest.mark.parametrize("shape", T.SHAPES)
def test_parameter_and_input_gradients_match_float64_autograd(dev, shape):
    """Every parameter gradient and dx against float64 autograd of the restatement: max |d| / max |ref| per tensor within
    4 x the float32-torch figure (a conv bias, an exact zero, by max |dW| of its stage).  Every clip is decided, so nothing
    but rounding separates the two.  At L = 16000 stage 2 has 3 pre-pool positions beyond 4 Q_2: dW_2 formed without their dz
    is outside the bound of what the kernels give -- the test sees that branch."""
    ref = T.reference(shape)[5]
    assert bool(T.decided(T.reference(shape)[3], shape).all())
    _, _, _, got = _step(shape)
    errs = T.grad_errors(got, ref)
    print(f"m5 train gradients {shape}: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()) + f" (bound {T.GRAD_BOUND:.1e})")
    assert max(errs.values()) <= T.GRAD_BOUND, errs                           # (NaN fails)
    if shape == T.SHAPES[4]:
        wrong, ntail = T.dw2_without_tail(shape)
        assert ntail == 3
        assert float((wrong - got["conv2.weight"].double()).abs().max() / ref["conv2.weight"].abs().max()) > T.GRAD_BOUND


def test_first_maximum_wins_on_exact_ties(dev):
    """m5_train_restate.tie_clips: 2491 open windows of stage 1 hold four bit-equal values (the kernel computes the four
    positions of a window with the same FMA chain on the same samples).  nn.MaxPool1d hands the gradient to the first; a
    last-maximum-wins kernel would be off by the size of dx itself (asserted on the CPU)."""
    sd, x, y, ref, _, g64 = T.tie_reference()
    B, L, nc, no = T.TIE_SHAPE
    m5 = _module(sd, nc, no, dev)
    xg = x.to(dev).requires_grad_(True)
    out = m5(xg)
    F.nll_loss(out, y.to(dev)).backward()
    assert float((out.detach().cpu().double() - ref["logp"].detach()).abs().max()) <= T.FWD_BOUND
    errs = T.grad_errors(_grads_of(m5, xg), g64)
    print(f"m5 train ties: " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()) + f" (bound {T.GRAD_BOUND:.1e})")
    assert max(errs.values()) <= T.GRAD_BOUND, errs


def test_negative_gamma_takes_the_max_after_the_affine(dev):
    shape = T.SHAPES[2]
    sd, x, _, ref, _, _ = T.reference(shape)
    with torch.no_grad():
        wrong = T.forward(T.tensors(sd, torch.float64, False), x.double(), max_then_affine=True)["logp"]
    assert float((wrong - ref["logp"].detach()).abs().max()) > 100 * T.FWD_BOUND
    out = _step(shape)[1].double()
    assert float((out - ref["logp"].detach()).abs().max()) <= T.FWD_BOUND
    assert float((out - wrong).abs().max()) > 50 * T.FWD_BOUND


@pytest.mark.parametrize("c", [0, 1])
def test_the_references_own_numbers(dev, c):
    """tests/golden/golden_m5_train_v1.npz: the reference's M5 in .train(), float32 on the CPU.  Two float32 evaluations: the
    kernels' bound against float64 plus the float32-torch figure the reference's own run is good for."""
    g = np.load(GOLDEN)
    shape = tuple(int(v) for v in g[f"{c}/shape"])
    m5, out, loss, got = _step(shape)
    assert float(np.abs(out.numpy() - g[f"{c}/logp"]).max()) <= T.FWD_BOUND and abs(loss - float(g[f"{c}/loss"])) <= T.FWD_BOUND
    ref = {k: torch.from_numpy(g[f"{c}/grad/{k}"]) for k in T.PARAMS}
    ref["x"] = torch.from_numpy(g[f"{c}/dx"])
    errs = T.grad_errors(got, ref)
    assert max(errs.values()) <= T.GRAD_BOUND + T.GRAD_F32_ERR, errs
    for k, v in m5.named_buffers():
        assert float(np.abs(v.cpu().numpy().astype(np.float64) - g[f"{c}/run1/{k}"]).max()) <= T.FWD_BOUND, k


def test_three_adam_steps_follow_float64_and_eval_refolds(dev):
    """M5/train.py's loop: Adam(lr 0.01, weight_decay 1e-4), three steps.  Each step's loss stays within the forward bound
    plus 4 x the float32-torch trajectory figure of the float64 trajectory; then .eval(): the folded native forward is the
    float64 folded forward of the UPDATED parameters and running statistics -- the eval handle re-folded by itself."""
    shape = T.SHAPES[2]
    B, L, nc, no = shape
    sd, x, y = T.case_inputs(shape)
    l64, _ = T.adam_trajectory(sd, x, y)
    m5 = _module(sd, nc, no, dev)
    xd, yd = x.to(dev), y.to(dev)
    m5.eval()
    with torch.no_grad():
        before = m5(xd).cpu()
    m5.train()
    opt = torch.optim.Adam(m5.parameters(), lr=0.01, weight_decay=1e-4)
    losses = []
    for _ in range(3):
        loss = F.nll_loss(m5(xd), yd)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"m5 adam: losses {losses}, float64 {l64}, bound {T.TRAJ_BOUND:.1e}")
    assert max(abs(a - b) for a, b in zip(losses, l64)) <= T.TRAJ_BOUND
    assert all(int(bn.num_batches_tracked) == 103 for bn in m5._bns())
    m5.eval()
    with torch.no_grad():
        after = m5(xd).cpu()
    now = {k: v.detach().cpu().numpy() for k, v in m5.state_dict().items()}
    ref, _ = FR.m5_forward(now, x.double())
    assert float((after.double() - ref).abs().max()) <= T.EVAL_FWD_BOUND
    assert float((after - before).abs().max()) > 1000 * T.EVAL_FWD_BOUND         # the stale fold would be far away


# ---- the C-ABI itself ---------------------------------------------------------------------------------------------------
def _handle_and_blob(shape, dev):
    B, L, nc, no = shape
    sd = T.weights(no, nc)
    m5 = _module(sd, nc, no, dev)
    blob = torch.cat([t.detach().reshape(-1).float() for t in m5._tensors()]).contiguous()
    return m5, m5._train_handle(blob), blob


def _cabi_step(shape, dev, want_dx=True, ws_bytes=None, L=None):
    """ap_m5_train_fwd(keep) + ap_m5_train_bwd into NaN-filled outputs and a NaN-filled workspace -> (rc, rc, outputs)"""
    B, L0, nc, no = shape
    L = L or L0
    lib = N.lib()
    m5, h, blob = _handle_and_blob(shape, dev)
    x = T.clips(B, L, 7).to(dev)
    v = FR.m5_cotangent(B, no).to(dev)
    nan = lambda n: torch.full((n,), float("nan"), device=dev, dtype=torch.float32)   # noqa: E731
    need = lib.ap_m5_train_workspace_bytes(h, B, L)
    nws = need if ws_bytes is None else ws_bytes
    ws = nan(max(nws, 4) // 4 + 1)
    out, run, grads, dx = nan(B * no), nan(2 * 6 * nc), nan(lib.ap_m5_param_elems(h)), nan(B * L)
    rc1 = lib.ap_m5_train_fwd(h, N.ptr(blob), N.ptr(x), N.ptr(out), N.ptr(run), 0.1, ws.data_ptr(), nws, 1, B, L, N.stream())
    e1 = lib.ap_last_error().decode() if rc1 else ""
    rc2 = lib.ap_m5_train_bwd(h, N.ptr(blob), N.ptr(x), N.ptr(v), N.ptr(grads), N.ptr(dx) if want_dx else None, ws.data_ptr(), nws,
                              B, L, N.stream())
    e2 = lib.ap_last_error().decode() if rc2 else ""
    torch.cuda.synchronize()
    return (rc1, e1), (rc2, e2), (out, run, grads, dx), need, m5


def test_two_runs_give_equal_bits_and_poison_leaves_no_nan(dev):
    """Fixed summation order, no atomics: every output of two runs is bit-equal.  Workspace, gradient blob and dx start as
    NaN: none is left, so every element is written and nothing is read before it is written."""
    shape = T.SHAPES[2]
    a = _cabi_step(shape, dev)
    b = _cabi_step(shape, dev)
    assert a[0][0] == 0 and a[1][0] == 0, (a[0], a[1])
    for ta, tb in zip(a[2], b[2]):
        assert not bool(torch.isnan(ta).any())
        assert torch.equal(ta, tb)
    assert N.lib().ap_m5_param_elems(a[4]._train_handle()) == sum(p.numel() for p in a[4].parameters())
    # dx = NULL: the gradients are the same, dx is left alone
    c = _cabi_step(shape, dev, want_dx=False)
    assert torch.equal(c[2][2], a[2][2]) and bool(torch.isnan(c[2][3]).all())


def test_long_clips_train_although_the_eval_backward_refuses_them(dev):
    """L = 48000: the activations live in the workspace, not in LDS (ap_m5_bwd: 168 608 B of LDS, refused)."""
    shape = (2, 48000, 32, 10)
    fwd, bwd, outs, _, m5 = _cabi_step(shape, dev)
    assert fwd[0] == 0 and bwd[0] == 0, (fwd, bwd)
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    x = T.clips(2, 48000, 7).to(dev)
    dx = torch.empty_like(x)
    m5.eval()
    assert N.lib().ap_m5_bwd(m5._handle(), N.ptr(x), N.ptr(FR.m5_cotangent(2, 10).to(dev)), N.ptr(dx), 2, 48000, N.stream()) == -22
    assert b"bytes of LDS" in N.lib().ap_last_error()


def test_cabi_refusals_leave_the_outputs_alone(dev):
    """Too short for four stages (6847; 6848 is served), a workspace one byte short: -22 with a text, before any launch.  (The
    third refusal, n <= 1 values per channel, cannot be reached through a length the first one lets pass: Q4 >= 1 gives stage 4
    at least four positions.)"""
    shape = T.SHAPES[1]
    fwd, bwd, outs, _, m5 = _cabi_step(shape, dev, L=6847)
    assert fwd[0] == -22 and "too short for four conv/pool stages" in fwd[1]
    assert bwd[0] == -22 and "too short for four conv/pool stages" in bwd[1]
    assert all(bool(torch.isnan(t).all()) for t in outs)
    assert N.lib().ap_m5_train_workspace_bytes(m5._train_handle(), 2, 6847) == 0
    need = N.lib().ap_m5_train_workspace_bytes(m5._train_handle(), 2, 6848)
    fwd, bwd, outs, need2, _ = _cabi_step(shape, dev, ws_bytes=need - 1)
    assert need2 == need
    assert fwd[0] == -22 and f"workspace of {need - 1} bytes, {need} needed" in fwd[1]
    assert bwd[0] == -22 and "workspace of" in bwd[1]
    assert all(bool(torch.isnan(t).all()) for t in outs)
    with pytest.raises(N.NativeError, match="too short for four conv/pool stages"):
        m5.train()(T.clips(2, 6847, 7).to(dev))


def test_module_refusals_raise_before_any_launch(dev):
    shape = T.SHAPES[1]
    B, L, nc, no = shape
    sd, x, y = T.case_inputs(shape)
    xd = x.to(dev)

    def stats(m):
        return [b.clone() for b in m.buffers()]

    from audiopure_amd.audio_models.M5.M5Net import M5
    for kw in (dict(affine=False), dict(track_running_stats=False)):
        m5 = _module(sd, nc, no, dev)
        m5.bn3 = torch.nn.BatchNorm1d(2 * nc, **kw).to(dev)
        before = stats(m5)
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            m5(xd)
        assert all(torch.equal(a, b) for a, b in zip(before, stats(m5)))
    with pytest.raises(NotImplementedError, match="HIP device"):
        M5(n_input=1, n_output=no, n_channel=nc).train()(x)
    m5 = _module(sd, nc, no, dev)
    loss = F.nll_loss(m5(xd), y.to(dev))
    with pytest.raises(NotImplementedError, match="double backward"):
        loss.backward(create_graph=True)
    assert all(p.grad is None for p in m5.parameters())


def _digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# sha256 over the float32 bytes of (ap_m5_fwd log-probabilities, ap_m5_bwd dx) at B = 8, L = 16000, n_channel = 32, n_output = 10,
# frontend_restate's weights, clips and cotangent -- taken on an MI355X from a library built from the commit before the
# train-mode kernels (the parent commit's sources, the same compiler and flags)
EVAL_DIGEST = "e31c6f3bf7904b85e893eaa22d61e75660bfd46b1122f83528e3b5eba7380565"


def test_eval_mode_is_bit_for_bit_what_it_was(dev):
    from audiopure_amd.audio_models.M5.M5Net import M5
    m5 = M5(n_input=1, n_output=10, n_channel=32)
    m5.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in FR.m5_weights(10, 32).items()})
    m5 = m5.to(dev).eval()
    x, v = FR.m5_clips(8, 16000).to(dev), FR.m5_cotangent(8, 10).to(dev)
    out, dx = torch.empty((8, 10), device=dev), torch.empty_like(x)
    N.check(N.lib().ap_m5_fwd(m5._handle(), N.ptr(x), N.ptr(out), 8, 16000, N.stream()), "ap_m5_fwd")
    N.check(N.lib().ap_m5_bwd(m5._handle(), N.ptr(x), N.ptr(v), N.ptr(dx), 8, 16000, N.stream()), "ap_m5_bwd")
    assert _digest(out, dx) == EVAL_DIGEST
    # and through the module, after a detour through train mode and back
    with torch.no_grad():
        assert torch.equal(m5(x), out)
    state = {k: t.clone() for k, t in m5.state_dict().items()}
    m5.train()
    with torch.no_grad():
        m5(x)
    m5.load_state_dict(state)
    m5.eval()
    xg = x.clone().requires_grad_(True)
    lp = m5(xg)
    (g,) = torch.autograd.grad(lp, xg, v)
    assert torch.equal(lp.detach(), out) and torch.equal(g, dx)
