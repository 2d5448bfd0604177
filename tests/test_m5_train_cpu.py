"""CPU checks behind test_gpu_m5_train.py: the float64 restatement of train-mode M5 (m5_train_restate.py) reproduces the
reference's own numbers (tests/golden/golden_m5_train_v1.npz, written by tests/golden/make_golden_m5_train.py from the
reference's ``M5Net.M5`` in ``.train()``), and the conditions the GPU bounds rest on hold for the case table."""
import os

import numpy as np
import pytest
import torch

import frontend_restate as FR
import m5_train_restate as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_m5_train_v1.npz")
REMEASURED = 2.0               # a float32 figure measured again on another CPU (other summation order) stays within 2 x the record


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("c", [0, 1])
def test_restatement_reproduces_the_reference(golden, c):
    """The reference ran in float32; the restatement in float64 agrees with it to the float32 error recorded for the GPU
    bound (every clip of both cases is decided, so no selection separates the two)."""
    shape = tuple(int(v) for v in golden[f"{c}/shape"])
    assert shape == T.SHAPES[1 + c]
    sd, x, y, out, loss, grads = T.reference(shape)
    assert float(np.abs(out["logp"].detach().numpy() - golden[f"{c}/logp"]).max()) <= T.FWD_BOUND
    assert abs(float(loss) - float(golden[f"{c}/loss"])) <= T.FWD_BOUND
    got = {k: torch.from_numpy(golden[f"{c}/grad/{k}"]) for k in T.PARAMS}
    got["x"] = torch.from_numpy(golden[f"{c}/dx"])
    errs = T.grad_errors(got, grads)
    assert max(errs.values()) <= T.GRAD_BOUND, errs
    # running statistics after one and after two forwards of the same clips (momentum 0.1, the variance unbiased)
    t = T.tensors(sd, torch.float64, False)
    for step in (1, 2):
        with torch.no_grad():
            run = T.forward(t, x.double())["running"]
        for k, v in run.items():
            assert float((v - torch.from_numpy(golden[f"{c}/run{step}/{k}"]).double()).abs().max()) <= T.FWD_BOUND, (step, k)
            t[k] = v
        assert int(golden[f"{c}/run{step}/bn1.num_batches_tracked"]) == 100 + step


def test_unbiased_running_variance_is_visible_at_the_smallest_case():
    """B = 1, L = 6848: stage 4 has four values per channel, so n / (n - 1) = 4 / 3 -- a biased update is far outside the bound."""
    shape = T.SHAPES[0]
    sd, x, y, out, _, _ = T.reference(shape)
    z4 = out["z"][3].detach()
    assert z4.shape[0] * z4.shape[2] == 4
    biased = 0.9 * torch.as_tensor(sd["bn4.running_var"]).double() + 0.1 * z4.var(dim=(0, 2), unbiased=False)
    assert float((biased - out["running"]["bn4.running_var"]).abs().max()) > 100 * T.FWD_BOUND


def test_case_table_conditions():
    """Every case with a seed has EVERY clip decided at its tau = 4 x its float32 pre-pool error (re-measured here at the
    default seed); at most two cases are loose; the named tail positions are the ones the lengths give."""
    loose = [s for s in T.SHAPES if T.CLIP_SEED[s] is None]
    assert len(loose) <= T.MAX_LOOSE
    for shape in T.SHAPES:
        B, L, nc, no = shape
        e = T.prepool_f32_error(T.weights(no, nc), T.clips(B, L, T.DEFAULT_SEED))
        print(f"{shape}: float32 pre-pool error {e:.2e} (recorded {T.PREPOOL_F32_ERR[shape]:.1e})")
        assert e <= REMEASURED * T.PREPOOL_F32_ERR[shape]
        if T.CLIP_SEED[shape] is not None:
            out = T.reference(shape)[3]
            assert bool(T.decided(out, shape).all()), shape
            # and float32 at the case's own clips stays below tau / 2, the condition m5_decided states
            sd, x, _ = T.case_inputs(shape)
            assert T.prepool_f32_error(sd, x) < T.tau(shape) / 2
    tails = lambda L: [p - 4 * q for p, q in zip(_P(L), FR.m5_dims(L)[1:])]   # noqa: E731
    assert tails(16000) == [0, 3, 3, 0] and tails(8000) == [0, 2, 0, 1]
    assert FR.m5_dims(6848)[4] == 1 and FR.m5_dims(6847)[4] == 0


def _P(L):
    P1, Q1, Q2, Q3, _ = FR.m5_dims(L)
    return [P1, Q1 - 2, Q2 - 2, Q3 - 2]


@pytest.mark.parametrize("shape", T.SHAPES)
def test_float32_gradient_error_and_exact_zero_of_the_conv_bias(shape):
    """The figure the GPU bound is 4 x of: float32 torch autograd of the restatement against float64, per parameter.  And
    every conv bias gradient of float64 is below 1e-12 of max |d beta| of its stage -- the exact zero that lets the GPU test
    normalise a conv bias gradient by max |dW| instead."""
    sd, x, y, _, _, g64 = T.reference(shape)
    for i in (1, 2, 3, 4):
        assert float(g64[f"conv{i}.bias"].abs().max()) < 1e-12 * float(g64[f"bn{i}.bias"].abs().max())
    _, _, g32, _ = T.loss_and_grads(sd, x, y, torch.float32)
    errs = T.grad_errors(g32, g64)
    print(f"{shape}: float32 gradient errors {({k: f'{v:.1e}' for k, v in errs.items()})}")
    assert max(errs.values()) <= REMEASURED * T.GRAD_F32_ERR


def test_dropping_the_tail_positions_fails_the_gradient_bound():
    """dW_2 without the dz of the 3 pre-pool positions beyond 4 Q_2 (L = 16000) is orders outside the bound."""
    shape = T.SHAPES[4]
    ref = T.reference(shape)[5]["conv2.weight"]
    wrong, ntail = T.dw2_without_tail(shape)
    assert ntail == 3
    assert float((wrong - ref).abs().max() / ref.abs().max()) > 100 * T.GRAD_BOUND


def test_max_before_the_affine_is_wrong_for_a_negative_gamma():
    shape = T.SHAPES[2]
    sd, x, _, out, _, _ = T.reference(shape)
    assert all((np.asarray(sd[f"bn{i}.weight"]) < 0).any() for i in (1, 2, 3, 4))
    with torch.no_grad():
        wrong = T.forward(T.tensors(sd, torch.float64, False), x.double(), max_then_affine=True)["logp"]
    assert float((wrong - out["logp"].detach()).abs().max()) > 100 * T.FWD_BOUND
    # ... and it is the flipped signs that do it: with every gamma positive the two orders agree
    pos = {k: (np.abs(v) if k.endswith("weight") and k.startswith("bn") else v) for k, v in sd.items()}
    with torch.no_grad():
        a = T.forward(T.tensors(pos, torch.float64, False), x.double(), max_then_affine=True)["logp"]
        b = T.forward(T.tensors(pos, torch.float64, False), x.double())["logp"]
    assert float((a - b).abs().max()) < 1e-12


def test_adam_trajectory_in_float32_stays_near_float64():
    """Three Adam steps (lr 0.01, weight_decay 1e-4) in float32 torch against float64: the figure the GPU trajectory bound is
    4 x of.  Adam divides by sqrt(v): where a gradient element is at the size of its float32 error the step's sign is not
    determined, so parameters are not compared element by element -- the losses are."""
    shape = T.SHAPES[2]
    sd, x, y = T.case_inputs(shape)
    l64, _ = T.adam_trajectory(sd, x, y)
    l32, _ = T.adam_trajectory(sd, x, y, dtype=torch.float32)
    errs = [abs(a - b) for a, b in zip(l32, l64)]
    print(f"losses float64 {l64}, float32 deviations {errs}")
    assert l64[2] < l64[0]                                                    # it trains
    assert max(errs) <= REMEASURED * T.TRAJ_F32_ERR


def test_tie_case_has_exact_ties_and_a_stable_reference():
    """The tie clips: in stage 1 thousands of open pooling windows hold four equal values, every other window of every stage
    is decided; float32 torch agrees with float64 to the recorded figure (the ties are exact in both, so both hand the
    gradient to the first position); a last-maximum-wins rule moves dx by the order of dx itself."""
    sd, x, y, out, _, g64 = T.tie_reference()
    y1 = out["y"][0].detach()
    tied = T.tied_windows(y1)
    assert int((tied & (y1[..., ::4][..., :tied.shape[-1]] > 0)).sum()) > 2000
    assert bool(T.decided_or_tied(out["y"], T.TIE_TAU).all())
    assert not bool(FR.m5_decided(out["y"], T.TIE_TAU).any())                 # (without the ties' exemption no clip is decided)
    assert T.prepool_f32_error(sd, x) < T.TIE_TAU / 2
    _, _, g32, _ = T.loss_and_grads(sd, x, y, torch.float32)
    assert max(T.grad_errors(g32, g64).values()) <= REMEASURED * T.GRAD_F32_ERR
    _, _, glast, _ = T.loss_and_grads(sd, x, y, stage1_last_max=True)
    assert T.grad_errors(glast, g64)["x"] > 1000 * T.GRAD_BOUND
