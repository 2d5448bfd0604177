"""The KWS classifier's training step on the device (ap_kws_train_bwd, ap_kws_set_weights, KWSModel in train()) against the
float64 references of kws_train_restate.py.  Every output and the workspace are NaN-filled before a call, so an element a kernel
leaves out, or reads before it is written, fails the comparison.  The parameter-gradient bound is 8 x the float32 error of the
reference on these very cases, per tensor, of the tensor's largest reference entry; the log-probabilities and the input gradient
keep the bounds of the inference route (kws_restate.py), whose bits they are.  The case table and the conditions on the reference
are asserted by test_kws_train_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import kws_restate as R
import kws_train_restate as TR
from audiopure_amd import _native as N

pytestmark = pytest.mark.gpu
ids = lambda c: "-".join(map(str, c))       # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nan_like(shape, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def _new_model(shape, weights=None):
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    n_mels, H, Kc = shape
    m = KWSModel(in_size=n_mels, hidden_size=H, num_classes=Kc)
    m.load_state_dict(weights if weights is not None else R.kws_weights(*shape))
    return m.to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _model(shape):
    return _new_model(shape).eval()


def _inputs(case, dev):
    n_mels, H, Kc, T, B = case
    return R.kws_mel(n_mels, T, B)[:, 0].contiguous().to(dev), R.kws_cotangent(n_mels, T, B, Kc).to(dev)


def _train_bwd(m, xd, vd, dx, dp, ws=None):
    """into dx [B,n_mels,T] (or None) and dp [blob]; the workspace is NaN-filled: each save is written before it is read"""
    B, _, T = xd.shape
    n = N.lib().ap_kws_train_workspace_elems(m._handle(), B, T)
    assert n > 0
    ws = nan_like((n,), xd.device) if ws is None else ws
    return N.lib().ap_kws_train_bwd(m._handle(), N.ptr(xd), N.ptr(vd), N.ptr(dx), N.ptr(dp), N.ptr(ws), ws.numel(), B, T, N.stream())


def _split(m, dp):
    out, at = {}, 0
    for k, v in m.state_dict().items():
        out[k] = dp[at:at + v.numel()].view(v.shape)
        at += v.numel()
    assert at == dp.numel()
    return out


def _blob(m):
    return N.lib().ap_kws_blob_elems(m.in_size, m.hidden_size, m.num_classes)


@pytest.mark.parametrize("case", TR.TRAIN_CASES + TR.TRAIN_BWD_ONLY_CASES, ids=ids)
def test_parameter_gradients_match_float64_and_keep_the_input_gradients_bits(dev, case):
    """T = 5, 19, 20 / 21: the second GRU step appears (before it weight_hh and the attention's own gradients are exactly 0);
    (20, 128, 64) fills the sweep's static arrays and gives whole 64 x 64 tiles, (60, 96, 12) and (32, 8, 1) partial ones;
    B = 1: 5 items over 16 slices, most of them empty; B = 67: slices of 20 and 21 items; B = 300: more clips than compute units;
    T = 1001: the backward alone, past the forward's LDS limit."""
    n_mels, H, Kc, T, B = case
    m = _model(case[:3])
    lp_ref, dx_ref, g_ref = TR.train_reference(case)
    xd, vd = _inputs(case, dev)
    dx, dp = nan_like((B, n_mels, T), dev), nan_like((_blob(m),), dev)
    N.check(_train_bwd(m, xd, vd, dx, dp), "ap_kws_train_bwd")
    got = {k: v.cpu().double() for k, v in _split(m, dp).items()}
    assert list(got) == list(g_ref)
    worst = 0.0
    for k, ref in g_ref.items():
        assert bool(torch.isfinite(got[k]).all()), k
        err = TR.tensor_rel_err(got[k], ref)
        worst = max(worst, err)
        if TR.exact_zero(k, Kc, T):
            assert bool((got[k] == 0.0).all()), k
        else:
            assert err <= TR.TRAIN_GRAD_BOUND, (k, err)
    print(f"kws train {case}: parameter gradients to {worst:.2e} of max |ref| (bound {TR.TRAIN_GRAD_BOUND:.1e})")
    # the input gradient: float64, and the bits of ap_kws_bwd
    if Kc == 1:
        assert bool((dx == 0.0).all())
    else:
        err = R.per_clip_rel_err(dx.cpu().double(), dx_ref)
        assert float(err.max()) <= R.KWS_GRAD_BOUND, err.tolist()
    plain = nan_like((B, n_mels, T), dev)
    ns = N.lib().ap_kws_bwd_scratch_elems(m._handle(), B, T)
    N.check(N.lib().ap_kws_bwd(m._handle(), N.ptr(xd), N.ptr(vd), N.ptr(plain), N.ptr(nan_like((ns,), dev)), B, T, N.stream()), "ap_kws_bwd")
    assert torch.equal(plain, dx)
    # determinism under poisoning, and dmel == NULL: the same parameter bits
    dx2, dp2, dp3 = nan_like((B, n_mels, T), dev), nan_like((_blob(m),), dev), nan_like((_blob(m),), dev)
    N.check(_train_bwd(m, xd, vd, dx2, dp2), "ap_kws_train_bwd")
    N.check(_train_bwd(m, xd, vd, None, dp3), "ap_kws_train_bwd")
    assert torch.equal(dx2, dx) and torch.equal(dp2, dp) and torch.equal(dp3, dp)
    if case in TR.TRAIN_CASES:
        # train-mode forward = eval-mode forward, to float64
        x4 = xd[:, None]
        with torch.no_grad():
            lp_eval = m(x4)
        m.train()
        try:
            lp_train = m(x4)
            with torch.no_grad():
                lp_nograd = m(x4)
        finally:
            m.eval()
        assert lp_train.requires_grad and not lp_nograd.requires_grad
        assert torch.equal(lp_train.detach(), lp_eval) and torch.equal(lp_nograd, lp_eval)
        assert float((lp_eval.cpu().double() - lp_ref).abs().max()) <= (0.0 if Kc == 1 else R.KWS_LOGP_BOUND)


def test_the_references_own_numbers_through_the_public_module(dev):
    """The reference's KWSModel in train(), CrossEntropyLoss on its log-probabilities (train.py:79,148-149), backward(): loss,
    log-probabilities, x.grad and every parameter gradient of the golden file; then the B = 1 squeeze path."""
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    G, W = np.load(TR.GOLDEN_TRAIN), np.load(R.ROOT + "/tests/golden/golden_kws_v1.npz")
    for tag, n_mels, T, B in (("m32/T161_B3", 32, 161, 3), ("m40/T81_B1", 40, 81, 1)):
        m = KWSModel(in_size=n_mels)
        m.load_state_dict({k.split("/sd/")[1]: torch.from_numpy(W[k]) for k in W.files if k.startswith(f"m{n_mels}/sd/")})
        m = m.cuda().train()
        x = TR.golden_input(n_mels, T, B).to(dev).requires_grad_(True)
        lp = m(x)
        loss = torch.nn.CrossEntropyLoss()(lp, TR.train_targets(B, 4).to(dev))
        loss.backward()
        assert abs(float(loss.detach()) - float(G[f"{tag}/loss"])) <= R.KWS_LOGP_BOUND      # a mean of log-probabilities
        assert x.grad.shape == x.shape
        assert float(R.per_clip_rel_err(x.grad.cpu().double(), torch.from_numpy(G[f"{tag}/dx"]).double()).max()) <= R.KWS_GRAD_BOUND
        names = [k.split("/grad/")[1] for k in G.files if k.startswith(f"{tag}/grad/")]
        assert len(names) == (len(m.state_dict()) if B == 3 else 4)
        grads = dict(m.named_parameters())
        for k in names:
            err = TR.tensor_rel_err(grads[k].grad.cpu(), torch.from_numpy(G[f"{tag}/grad/{k}"]))
            assert err <= TR.TRAIN_GRAD_BOUND, (tag, k, err)
        if B == 3:
            assert float((lp.detach().cpu() - torch.from_numpy(G[f"{tag}/logp"])).abs().max()) <= R.KWS_LOGP_BOUND


def test_pgd_shaped_use_in_train_mode(dev):
    """train.py:84-121 calls the model in train() for the input gradient: one backward gives the input's and the parameters'
    gradients; a second backward accumulates into .grad as torch's own would; zero_grad starts over; a double backward raises;
    with every parameter frozen the input-gradient node of the inference route runs and no parameter gets a .grad."""
    case = R.GOLDEN_SHAPE + (37, 8)
    n_mels, H, Kc, T, B = case
    m = _new_model(case[:3]).train()
    _, dx_ref, g_ref = TR.train_reference(case)
    v = R.kws_cotangent(n_mels, T, B, Kc).to(dev)
    x = R.kws_mel(n_mels, T, B).to(dev).requires_grad_(True)
    lp = m(x)
    assert type(lp.grad_fn).__name__ == "_KwsTrainFnBackward"
    lp.backward(v)
    assert float(R.per_clip_rel_err(x.grad[:, 0].cpu().double(), dx_ref).max()) <= R.KWS_GRAD_BOUND
    once = {k: p.grad.clone() for k, p in m.named_parameters()}
    for k, ref in g_ref.items():
        assert once[k].shape == ref.shape and TR.tensor_rel_err(once[k].cpu(), ref) <= TR.TRAIN_GRAD_BOUND, k
    m(x.detach()).backward(2.0 * v)                              # the input asks for nothing this time
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, once[k] + 2.0 * once[k]), k   # doubling the cotangent doubles every product and sum exactly
    m.zero_grad()
    assert all(p.grad is None or not bool(p.grad.any()) for p in m.parameters())
    lp = m(x)
    (gx,) = torch.autograd.grad(lp, x, v.clone().requires_grad_(True), create_graph=True)    # a graph through the backward itself
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    lp = m(x)
    assert type(lp.grad_fn).__name__ == "_KwsInputGradBackward"
    (gx,) = torch.autograd.grad(lp, x, v)
    assert torch.equal(gx, x.grad) and all(p.grad is None for p in m.parameters())
    assert not m(x.detach()).requires_grad


def test_three_adam_steps_follow_float64_and_refresh_the_handle_in_place(dev):
    """train.py:80,147-153: Adam(weight_decay=1e-5), zero_grad, backward, step.  The parameters after three steps follow the
    float64 run of the oracle; the handle keeps its address (the refresh went through ap_kws_set_weights, not destroy + create);
    and eval() afterwards classifies with the updated weights."""
    n_mels, H, Kc, T, B = TR.ADAM_CASE
    p64, mask = TR.adam_reference()
    m = _new_model(TR.ADAM_CASE[:3]).train()
    x, y = R.kws_mel(n_mels, T, B).to(dev), TR.train_targets(B, Kc).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=TR.ADAM_LR, weight_decay=TR.ADAM_WD)
    handles = []
    for _ in range(TR.ADAM_STEPS):
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(m(x), y).backward()
        handles.append(m._h.value)
        opt.step()
    err = TR.adam_err(dict(m.state_dict()), p64, mask)
    print(f"three Adam steps: {err:.2e} lr off the float64 run (bound {TR.ADAM_BOUND:.1e} lr)")
    assert err <= TR.ADAM_BOUND
    with torch.no_grad():
        lp = m.eval()(x)
    handles.append(m._h.value)
    assert handles[0] is not None and len(set(handles)) == 1
    fresh = _new_model(TR.ADAM_CASE[:3], {k: v.detach().cpu() for k, v in m.state_dict().items()}).eval()
    with torch.no_grad():
        assert torch.equal(fresh(x), lp)
        old = _model(TR.ADAM_CASE[:3])(x)
    assert float((old - lp).abs().max()) > 1e-3                   # the step moved the log-probabilities: stale weights would show


def test_cabi_refusals_leave_the_outputs_untouched(dev):
    case = R.GOLDEN_SHAPE + (21, 2)
    n_mels, H, Kc, T, B = case
    m = _model(case[:3])
    h = m._handle()
    xd, vd = _inputs(case, dev)
    dx, dp = nan_like((B, n_mels, T), dev), nan_like((_blob(m),), dev)
    n = N.lib().ap_kws_train_workspace_elems(h, B, T)
    ws = nan_like((n,), dev)
    lib, st = N.lib(), N.stream()
    assert lib.ap_kws_train_workspace_elems(None, B, T) == 0 and lib.ap_kws_train_workspace_elems(h, 0, T) == 0
    assert lib.ap_kws_train_workspace_elems(h, B, 4) == 0
    full = (h, N.ptr(xd), N.ptr(vd), N.ptr(dx), N.ptr(dp), N.ptr(ws), n, B, T, st)
    for i in (0, 1, 2, 4, 5):                                      # null handle / mel / dlogprobs / dparams / workspace
        assert lib.ap_kws_train_bwd(*[None if j == i else a for j, a in enumerate(full)]) == -22
        assert b"null" in lib.ap_last_error()
    assert lib.ap_kws_train_bwd(*full[:7], 0, T, st) == -22 and b"B = 0" in lib.ap_last_error()
    assert lib.ap_kws_train_bwd(*full[:7], B, 4, st) == -22 and b"too few" in lib.ap_last_error()
    assert lib.ap_kws_train_bwd(*full[:6], n - 1, B, T, st) == -22 and b"workspace" in lib.ap_last_error()
    blob = torch.zeros(_blob(m), device=dev)
    assert lib.ap_kws_set_weights(None, N.ptr(blob), blob.numel(), st) == -22
    assert lib.ap_kws_set_weights(h, None, blob.numel(), st) == -22
    assert lib.ap_kws_set_weights(h, N.ptr(blob), blob.numel() - 1, st) == -22 and b"expected" in lib.ap_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(dp).all()) and bool(torch.isnan(ws).all())
    # and the handle's weights are the ones it had: the refused set_weights copied nothing
    out, ref = nan_like((B, Kc), dev), nan_like((B, Kc), dev)
    N.check(lib.ap_kws_fwd(h, N.ptr(xd), N.ptr(out), B, T, st), "ap_kws_fwd")
    fresh = _new_model(case[:3])
    N.check(lib.ap_kws_fwd(fresh._handle(), N.ptr(xd), N.ptr(ref), B, T, st), "ap_kws_fwd")
    assert torch.equal(out, ref)


def test_module_refusals_in_train_mode_come_before_any_launch(dev):
    m = _new_model(R.GOLDEN_SHAPE).train()
    x = R.kws_mel(40, 81, 2).to(dev)
    with pytest.raises(NotImplementedError, match="initial GRU state"):
        m(x, hidden=torch.zeros(4, 2, 64, device=dev))
    with pytest.raises(ValueError, match="expected"):
        m(x[:, :, :39])
    assert m._h is None                                            # nothing was built, nothing ran
    out = m(x[:0])
    assert out.shape == (0, 4) and not out.requires_grad          # B == 0 as in eval
    with pytest.raises(N.NativeError, match="too few"):
        m(x[..., :4])
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    with pytest.raises(NotImplementedError, match="inference only"):
        KWSModel().train()(x.cpu())
