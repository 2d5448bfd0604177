"""The float64 restatement of the loss head (tests/loss_restate.py) pinned, on the CPU, to torch's own F.cross_entropy / F.nll_loss with
autograd in float64, to the reference's mixup_cross_entropy_loss and mixup (the golden), and the conditions and recorded bounds the
GPU test (test_gpu_loss.py) rests on; plus the host-side surface of audiopure_amd.losses."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_restate as L  # noqa: E402

GOOD = [c for c in L.CASES if not c[3]]


def test_conditions_hold_at_the_first_seed_that_meets_them():
    for c in L.CASES:
        seed = L.seed_of(c)
        assert all(not (L.conditions(c, s)[0] > 1e-4 and L.conditions(c, s)[1] > 1e-3) for s in range(seed)), L.case_id(c)
        gap, clamp = L.conditions(c, seed)
        assert gap > 1e-4 and clamp > 1e-3, L.case_id(c)
        z, y, soft = L.case(c)
        B, K = z.shape
        if B > L.TIE_ROW and K >= 2:                 # the deliberate tie is exact and is the row's maximum
            top = np.sort(z[L.TIE_ROW])[-2:]
            assert top[0] == top[1] == z[L.TIE_ROW].max()
            assert L.reference(c, 0)["pred"][L.TIE_ROW] == int(np.flatnonzero(z[L.TIE_ROW] == top[1])[0])
        assert ((y < 0) | (y >= K)).sum() == (1 if c[3] else 0)
    # the +-100 cases are what they are for: a softmax without the maximum subtracted overflows, and the clamp is live
    z, _, _ = L.case((5, 12, 100.0, False))
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(z.astype(np.float32) * np.float32(1.0))).any()
    assert (L.softmax64(z) < L.CLAMP).sum() > 0 and (L.softmax64(L.case((5, 12, 4.0, False))[0]) < L.CLAMP).sum() == 0


@pytest.mark.parametrize("c", GOOD, ids=L.case_id)
def test_restatement_is_torch_in_float64(c):
    z, y, soft = L.case(c)
    for mode in L.MODES:
        ref = L.reference(c, mode)
        got = L.torch_loss(L.mode_input(c, mode), y, soft, mode, torch.float64)
        assert L.rel(got["loss"], ref["loss"]) <= 1e-14 and L.rel(got["din"], ref["din"]) <= 1e-14, mode
        assert np.array_equal(torch.from_numpy(L.mode_input(c, mode)).max(1)[1].numpy(), ref["pred"])   # outputs.max(1): the first maximum
        assert ref["n_correct"] == int((ref["pred"] == y).sum())
    assert 0 < L.reference(c, 0)["n_correct"] < z.shape[0] or z.shape[0] == 1 or z.shape[1] == 1


def test_out_of_range_label_is_a_nan_row_and_nothing_else():
    c = next(c for c in L.CASES if c[3])
    for mode in (0, 2):
        ref = L.reference(c, mode)
        assert np.isnan(ref["rows"]).sum() == 1 and np.isnan(ref["rows"][2]) and np.isnan(ref["loss"])
        assert np.isnan(ref["din"][2]).all() and np.isfinite(np.delete(ref["din"], 2, 0)).all()
    assert np.isfinite(L.reference(c, 1)["din"]).all()          # mode 1 reads the labels for n_correct only


def test_recorded_bounds_are_what_float32_torch_measures():
    l, d = L.measure_f32()
    print(f"float32 torch against float64: loss {l:.2e} (recorded {L.LOSS_F32_ERR:.2e}), din {d:.2e} (recorded {L.DIN_F32_ERR:.2e})")
    assert l <= 4 * L.LOSS_F32_ERR <= 16 * l and d <= 4 * L.DIN_F32_ERR <= 16 * d
    assert L.LOSS_BOUND == 4 * L.LOSS_F32_ERR and L.DIN_BOUND == 4 * L.DIN_F32_ERR


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_mode_1_matches_the_reference(c):
    G = L.golden()
    ref = L.reference(c, 1)
    pre = f"mce/{L.case_id(c)}/"
    assert L.rel(G[pre + "loss"], ref["loss"]) <= L.LOSS_BOUND
    d = np.abs(G[pre + "din"].astype(np.float64) - ref["din"].reshape(-1)[:L.GOLDEN_FULL]).max()   # (the golden holds the first 4096 elements)
    assert d / (np.abs(ref["din"]).max() or 1.0) <= L.DIN_BOUND   # (K = 1: an exact-zero gradient, the absolute figure, as L.rel)


def test_mixup_expressions_are_torch_bits_and_the_reference():
    G = L.golden()
    for B, K in L.MIXUP_GOLDEN:
        x, y = L.mixup_inputs(B, K)
        w, idx = L.mixup_draws(B, B)
        assert np.array_equal(L.mixup_rows(x, idx, w), G[f"mixup/{B}/inputs"])
        assert np.array_equal(L.mixup_targets(y, idx, w, K), G[f"mixup/{B}/targets"])
        wt = torch.from_numpy(w).view(B, 1, 1, 1)
        xt = torch.from_numpy(x)
        assert np.array_equal(L.mixup_rows(x, idx, w), (wt * xt + (1 - wt) * xt[idx]).numpy())
    # not an fma, and 1 - w rounded first: some element of a generic row differs from both other evaluations
    x, _ = L.mixup_inputs(5, 12)
    w, idx = L.mixup_draws(5, 5)
    w64 = w.astype(np.float64).reshape(-1, 1, 1, 1)
    exact = (w64 * x + (1 - w64) * x[idx]).astype(np.float32)
    assert (exact != L.mixup_rows(x, idx, w)).any()


def test_losses_surface_on_the_host():
    from audiopure_amd import _native as N
    from audiopure_amd import losses
    z = torch.zeros(3, 4)
    y = torch.zeros(3, dtype=torch.int64)
    for call in (lambda: losses.cross_entropy(z, y), lambda: losses.nll_loss(z, y), lambda: losses.mixup_cross_entropy_loss(z, z),
                 lambda: losses.mixup(torch.zeros(3, 1, 4, 4), y, 4), lambda: losses.CrossEntropyLoss()(z, y)):
        with pytest.raises(N.NativeError):
            call()
    for kw in (dict(weight=torch.ones(4)), dict(ignore_index=0), dict(reduction="sum"), dict(label_smoothing=0.1)):
        with pytest.raises(ValueError):
            losses.CrossEntropyLoss(**kw)
    lib = N.lib()
    assert lib.ap_class_loss(None, None, None, 0, None, None, None, None, None, 1, 1, None) == -22
