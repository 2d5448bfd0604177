"""The loss head on the device (csrc/ap_loss.hip, audiopure_amd/losses.py) against the float64 restatement of tests/loss_restate.py at
its cases (B in {1, 5, 257}, K in {1, 2, 12, 64, 65, 200} -- one lane-held row, the first strided one, several strides; one
workgroup, a partly filled one, 65 of them --, logits in +-4 and +-100) within LOSS_BOUND / DIN_BOUND (4 x float32 torch's own error);
pred and n_correct exact, the tie included; equal bits of two runs; the NaN row of a bad label; the refusals; the mixup kernels bit
for bit against torch's CPU expression; the autograd surface with a non-unit upstream scale.  On the parent commit the library has no
ap_class_loss and the package no losses module."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
from audiopure_amd import _native as N  # noqa: E402
import loss_restate as L  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def run(dev, x, labels, soft, mode, stats=True, grad=True):
    """one ap_class_loss call -> dict of host arrays"""
    B, K = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    yd = None if labels is None else torch.from_numpy(labels).to(dev)
    qd = None if soft is None else torch.from_numpy(np.ascontiguousarray(soft)).to(dev)
    rows = torch.full((B,), 7.0, device=dev)
    loss = torch.full((1,), 7.0, device=dev)
    din = torch.full((B, K), 7.0, device=dev) if grad else None
    pred = torch.full((B,), -7, device=dev, dtype=torch.int64) if stats else None
    cnt = torch.full((1,), -7, device=dev, dtype=torch.int64) if stats and yd is not None else None
    ip = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    N.check(N.lib().ap_class_loss(N.ptr(xd), ip(yd), N.ptr(qd), mode, N.ptr(rows), N.ptr(loss), N.ptr(din), ip(pred), ip(cnt), B, K,
                                  N.stream()), "ap_class_loss")
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(rows=host(rows), loss=host(loss)[0], din=host(din), pred=host(pred), n_correct=None if cnt is None else int(cnt))


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("c", [c for c in L.CASES if not c[3]], ids=L.case_id)
def test_class_loss_matches_float64(dev, c, mode):
    z, y, soft = L.case(c)
    ref = L.reference(c, mode)
    x = L.mode_input(c, mode)
    got = run(dev, x, y, soft if mode == 1 else None, mode)
    el, er, ed = L.rel(got["loss"], ref["loss"]), L.rel(got["rows"], ref["rows"]), L.rel(got["din"], ref["din"])
    print(f"{L.case_id(c)} mode {mode}: loss {el:.2e}, rows {er:.2e} (bound {L.LOSS_BOUND:.2e}), din {ed:.2e} (bound {L.DIN_BOUND:.2e})")
    assert el <= L.LOSS_BOUND and er <= L.LOSS_BOUND and ed <= L.DIN_BOUND
    assert np.array_equal(got["pred"], ref["pred"]) and got["n_correct"] == ref["n_correct"]
    again = run(dev, x, y, soft if mode == 1 else None, mode)
    for k in ("rows", "din", "pred"):
        assert np.array_equal(got[k], again[k]), k
    assert got["loss"].tobytes() == again["loss"].tobytes() and got["n_correct"] == again["n_correct"]
    # the optional outputs change nothing; mode 1 without labels has no count
    bare = run(dev, x, None if mode == 1 else y, soft if mode == 1 else None, mode, stats=False, grad=False)
    assert bare["loss"].tobytes() == got["loss"].tobytes() and np.array_equal(bare["rows"], got["rows"])


def test_bad_label_is_a_nan_row(dev):
    c = next(c for c in L.CASES if c[3])
    z, y, soft = L.case(c)
    for mode in (0, 2):
        ref = L.reference(c, mode)
        got = run(dev, L.mode_input(c, mode), y, None, mode)
        assert np.isnan(got["loss"]) and np.array_equal(np.isnan(got["rows"]), np.isnan(ref["rows"]))
        assert np.array_equal(np.isnan(got["din"]), np.isnan(ref["din"]))
        keep = ~np.isnan(ref["rows"])
        assert L.rel(got["rows"][keep], ref["rows"][keep]) <= L.LOSS_BOUND and L.rel(got["din"][keep], ref["din"][keep]) <= L.DIN_BOUND
        assert np.array_equal(got["pred"], ref["pred"]) and got["n_correct"] == ref["n_correct"]
    got, ref = run(dev, z, y, soft, 1), L.reference(c, 1)
    assert L.rel(got["din"], ref["din"]) <= L.DIN_BOUND and got["n_correct"] == ref["n_correct"]


def test_refusals(dev):
    lib = N.lib()
    x = torch.zeros(4, 8, device=dev)
    y = torch.zeros(4, dtype=torch.int64, device=dev)
    rows, loss = torch.zeros(4, device=dev), torch.zeros(1, device=dev)
    call = lambda K, B=4, mode=0, lab=y.data_ptr(), soft=None, din=None, cnt=None: lib.ap_class_loss(  # noqa: E731
        N.ptr(x), lab, soft, mode, N.ptr(rows), N.ptr(loss), din, None, cnt, B, K, N.stream())
    assert call(8) == 0
    for kw, word in ((dict(K=0), b"K = 0"), (dict(K=4097), b"K = 4097"), (dict(K=8, B=0), b"B = 0"), (dict(K=8, B=65536), b"B = 65536"),
                     (dict(K=8, mode=3), b"mode"), (dict(K=8, lab=None), b"labels"), (dict(K=8, mode=1), b"soft"),
                     (dict(K=8, din=N.ptr(x)), b"overlaps"), (dict(K=8, cnt=y.data_ptr()), b"n_correct")):
        assert call(**kw) == -22 and word in lib.ap_last_error(), word
    buf = torch.zeros(3 * 10, device=dev)
    idx = torch.tensor([1, 0], device=dev)
    w = torch.full((2,), 0.25, device=dev)
    assert lib.ap_mixup_rows(N.ptr(buf), idx.data_ptr(), N.ptr(w), N.ptr(buf[10:]), 2, 10, N.stream()) == -22
    assert b"overlaps" in lib.ap_last_error()
    assert lib.ap_mixup_rows(N.ptr(buf), idx.data_ptr(), N.ptr(w), N.ptr(buf), 1, 10, N.stream()) == -22
    assert lib.ap_mixup_targets(y.data_ptr(), idx.data_ptr(), N.ptr(w), N.ptr(buf), 2, 0, N.stream()) == -22
    torch.cuda.synchronize()


@pytest.mark.parametrize("B", (1, 2, 5))
def test_mixup_kernels_are_torch_bits(dev, B):
    from audiopure_amd import losses
    K = 12
    w = np.linspace(0.1, 0.9, B).astype(np.float32) * np.float32(1.0 / 3.0) + np.float32(0.3)
    idx = np.roll(np.arange(B), 1)
    if B == 5:
        idx = np.array([1, 0, 2, 4, 3])              # a permutation with a fixed point
    y = (np.arange(B, dtype=np.int64) * 5 + 1) % K
    wt = torch.from_numpy(w)
    for n in (1, 1023, 1024, 1025):
        x = torch.from_numpy(np.random.RandomState(n).uniform(-3, 3, (B, 1, 1, n)).astype(np.float32))
        want = wt.view(B, 1, 1, 1) * x + (1 - wt.view(B, 1, 1, 1)) * x[idx]          # mixup.py:46-49 on the CPU
        oh = lambda t: torch.zeros(B, K).scatter_(1, t.view(-1, 1), 1)  # noqa: E731
        want_t = wt.view(B, 1) * oh(torch.from_numpy(y)) + (1 - wt.view(B, 1)) * oh(torch.from_numpy(y[idx]))
        got, got_t = losses.mixup_with(x.to(dev), torch.from_numpy(y).to(dev), K, w, idx)
        assert got.shape == x.shape and torch.equal(got.cpu(), want) and torch.equal(got_t.cpu(), want_t), n
        assert np.array_equal(got.cpu().numpy(), L.mixup_rows(x.numpy(), idx, w))
    # mixup(): the reference's host draws under np.random.seed
    x = torch.from_numpy(L.mixup_inputs(B, K)[0])
    np.random.seed(B)
    got, got_t = losses.mixup(x.to(dev), torch.from_numpy(y).to(dev), K)
    w2, idx2 = L.mixup_draws(B, B)
    assert np.array_equal(got.cpu().numpy(), L.mixup_rows(x.numpy(), idx2, w2))
    assert np.array_equal(got_t.cpu().numpy(), L.mixup_targets(y, idx2, w2, K))
    if (B, K) in L.MIXUP_GOLDEN:
        y_g = torch.from_numpy(L.mixup_inputs(B, K)[1])
        np.random.seed(B)
        g_x, g_t = losses.mixup(x.to(dev), y_g.to(dev), K)
        assert np.array_equal(g_x.cpu().numpy(), L.golden()[f"mixup/{B}/inputs"]) and np.array_equal(g_t.cpu().numpy(), L.golden()[f"mixup/{B}/targets"])
    # a bad index: NaN in that row, nothing else
    if B > 1:
        lib = N.lib()
        xd = x.to(dev).contiguous()
        out = torch.zeros_like(xd)
        bad = torch.from_numpy(idx).to(dev).clone()
        bad[0] = B
        N.check(lib.ap_mixup_rows(N.ptr(xd), bad.data_ptr(), N.ptr(wt.to(dev)), N.ptr(out), B, x[0].numel(), N.stream()))
        assert torch.isnan(out[0]).all() and torch.isfinite(out[1:]).all()


def test_losses_through_autograd_with_an_upstream_scale(dev):
    from audiopure_amd import losses
    c = (5, 12, 4.0, False)
    z, y, soft = L.case(c)
    yd = torch.from_numpy(y).to(dev)
    calls = {0: lambda x: losses.cross_entropy(x, yd, return_stats=True),
             1: lambda x: losses.mixup_cross_entropy_loss(x, torch.from_numpy(soft).to(dev), labels=yd, return_stats=True),
             2: lambda x: losses.nll_loss(x, yd, return_stats=True)}
    for mode in L.MODES:
        ref = L.reference(c, mode)
        x = torch.from_numpy(L.mode_input(c, mode)).to(dev).requires_grad_(True)
        loss, pred, n_correct = calls[mode](x)
        assert loss.shape == () and loss.is_cuda and pred.is_cuda and n_correct.is_cuda and not pred.requires_grad
        (loss * 4.0).backward()                                  # the upstream cotangent is a device scalar, 4 (an exact product)
        assert L.rel(loss.detach().cpu().numpy(), ref["loss"]) <= L.LOSS_BOUND
        assert L.rel(x.grad.cpu().numpy(), 4.0 * ref["din"]) <= L.DIN_BOUND
        assert np.array_equal(pred.cpu().numpy(), ref["pred"]) and int(n_correct) == ref["n_correct"]
    x = torch.from_numpy(z).to(dev).requires_grad_(True)
    crit = losses.CrossEntropyLoss()
    loss = crit(x, yd)
    loss.backward()
    assert L.rel(x.grad.cpu().numpy(), L.reference(c, 0)["din"]) <= L.DIN_BOUND
    total = losses.mixup_cross_entropy_loss(x.detach(), torch.from_numpy(soft).to(dev), size_average=False)
    assert L.rel(total.cpu().numpy(), L.reference(c, 1)["loss"] * 5) <= L.LOSS_BOUND + 2.0 ** -24   # (+ the rounding of the product by B = 5)
    with pytest.raises(N.NativeError):
        losses.cross_entropy(torch.from_numpy(z), yd)
