"""``ap_nes_perturb`` / ``ap_nes_grad`` (ap_kernels.hip) away from the one shape tests/test_gpu_certify.py runs them at: the
quad tail (L % 4 != 0), one quad, S = 2, the lead copy at other sizes, accumulation over garbage and over a known buffer, and
the refusals; ``ap_philox_normal`` at lengths around one quad against the numpy oracle.

The noise z_p of audio a is the Philox stream of utterance a S/2 + p; ``ap_philox_normal`` materialises it (the same device
function the kernels call; tests/test_gpu_parity.py shows the filled and the in-kernel stream are the same bits), and the
float64 restatement (tests/nes_restate.py) runs on those values.

One-line defects these cases catch and the shape A=3, S=10, L=4000 (a multiple of 4) does not: a quad tail written past L
(the guard after every output); a tail quad skipped because ``t + 3 >= L`` (L = 1, 3, 5, 1023, 1025); ``accumulate = 0``
that still reads the buffer (NaN prefill); the utterance offset truncated to 32 bits in the fill (``2^33 + 5`` against ``5``)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nes_restate as R  # noqa: E402
from audiopure_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = ((1, 2, 1, 0), (1, 2, 3, 1), (3, 4, 5, 1), (2, 10, 1023, 0), (2, 6, 1025, 1), (3, 10, 4096, 1))
SEED, DRAW, SIGMA, GUARD, SENTINEL = 0x5DEECE66D1234567, 6, 0.001, 64, -77.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _noise(dev, A, S, L):
    """z [A, S/2, L] fp32: row a S/2 + p of the stream (seed, draw), utterances from 0."""
    z = torch.empty(A * (S // 2), L, device=dev)
    N.check(N.lib().ap_philox_normal(N.ptr(z), SEED, DRAW, 0, A * (S // 2), L, N.stream()), "ap_philox_normal")
    return z.cpu().numpy().reshape(A, S // 2, L)


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("A,S,L,lead", SHAPES)
def test_perturb_every_copy_to_one_ulp(dev, A, S, L, lead):
    rng = np.random.default_rng([A, S, L, lead])
    x = rng.uniform(-1, 1, (A, L)).astype(np.float32)
    z = _noise(dev, A, S, L)
    n = A * (S + lead) * L
    out = torch.full((n + GUARD,), SENTINEL, device=dev)
    N.check(N.lib().ap_nes_perturb(N.ptr(torch.from_numpy(x).to(dev)), N.ptr(out), SIGMA, SEED, DRAW, A, S, lead, L,
                                   N.stream()), "ap_nes_perturb")
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all())                                  # nothing past the last copy (the quad tail)
    got = out[:n].cpu().numpy().reshape(A, S + lead, L)
    assert not (got == SENTINEL).any()
    want = R.perturb(x, z, SIGMA, S, lead)
    want32 = want.astype(np.float32)
    assert np.all(np.abs(got.astype(np.float64) - want32) <= _ulp(want32))
    if lead:
        assert np.array_equal(got[:, 0], x)
    half = S // 2
    plus, minus = got[:, lead:lead + half].astype(np.float64), got[:, lead + half:].astype(np.float64)
    assert np.all(np.abs((plus - x[:, None]) + (minus - x[:, None])) <= np.maximum(_ulp(plus), _ulp(minus)))
    assert np.abs(plus - x[:, None]).max() > 1e-2 * SIGMA                     # the copies really are perturbed


def _losses(rng, A, S):
    """Multiples of 1/64 below 8: loss[p] - loss[p + S/2] is exact in fp32, as tests/nes_restate.grad_bound assumes, and no
    pair is equal."""
    while True:
        loss = rng.integers(-512, 513, (A, S)).astype(np.float32) / 64
        if np.all(loss[:, :S // 2] != loss[:, S // 2:]):
            return loss


@pytest.mark.parametrize("A,S,L,lead", SHAPES)
def test_grad_against_fp64_within_the_fma_chain_bound(dev, A, S, L, lead):
    """(lead does not enter ap_nes_grad: the caller drops the lead copy's loss first.)"""
    rng = np.random.default_rng([A, S, L, 99])
    loss = _losses(rng, A, S)
    z = _noise(dev, A, S, L)
    want, bound = R.grad(loss, z, S), R.grad_bound(loss, z, S)
    assert np.all(bound > 0)
    lib, ld = N.lib(), torch.from_numpy(loss).to(dev)
    # accumulate = 0 over garbage: the buffer is overwritten, not read
    g = torch.full((A * L + GUARD,), float("nan"), device=dev)
    N.check(lib.ap_nes_grad(N.ptr(ld), N.ptr(g), SEED, DRAW, A, S, L, 0, N.stream()), "ap_nes_grad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(g[A * L:]).all())
    got = g[:A * L].cpu().numpy().reshape(A, L).astype(np.float64)
    assert np.isfinite(got).all()
    excess = (np.abs(got - want) / bound).max()
    print(f"nes_grad A={A} S={S} L={L}: max |d| / bound = {excess:.3f}")
    assert excess <= 1.0
    # accumulate = 1 onto a known buffer: the same estimate added, one more rounding
    g0 = rng.uniform(-2, 2, (A, L)).astype(np.float32)
    g = torch.full((A * L + GUARD,), SENTINEL, device=dev)
    g[:A * L] = torch.from_numpy(g0).to(dev).reshape(-1)
    N.check(lib.ap_nes_grad(N.ptr(ld), N.ptr(g), SEED, DRAW, A, S, L, 1, N.stream()), "ap_nes_grad")
    torch.cuda.synchronize()
    assert bool((g[A * L:] == SENTINEL).all())
    got = g[:A * L].cpu().numpy().reshape(A, L)
    total = g0.astype(np.float64) + want
    assert np.all(np.abs(got.astype(np.float64) - total) <= bound + _ulp(total))
    assert np.abs(got - g0).max() > 0


@pytest.mark.parametrize("L", (1, 2, 3, 5, 1025))
def test_philox_fill_matches_the_numpy_oracle_around_one_quad(dev, L):
    from oracle.philox import philox_normal
    seed, draw, off, B = 0x1234567890ABCDEF, 3, (1 << 33) + 5, 3
    t = torch.full((B * L + GUARD,), SENTINEL, device=dev)
    N.check(N.lib().ap_philox_normal(N.ptr(t), seed, draw, off, B, L, N.stream()), "ap_philox_normal")
    torch.cuda.synchronize()
    assert bool((t[B * L:] == SENTINEL).all())
    got = t[:B * L].cpu().numpy().reshape(B, L)
    ref = philox_normal(seed, draw, off, B, L)
    assert np.abs(got - ref).max() <= 2e-6
    assert len(np.unique(got[:, :4])) == got[:, :4].size                     # rows and quad lanes all differ
    low = philox_normal(seed, draw, 5, B, L)                                  # the high word of the offset is in the key
    assert np.abs(got - low).max() > 1e-3


def test_refusals_return_22_and_leave_the_outputs_alone(dev):
    lib = N.lib()
    A, S, L = 2, 4, 9
    x = torch.zeros(A, L, device=dev)
    loss = torch.ones(A, S, device=dev)
    out = torch.full((A * (S + 1) * L,), SENTINEL, device=dev)
    grad = torch.full((A * L,), SENTINEL, device=dev)
    px, pl, po, pg, st = N.ptr(x), N.ptr(loss), N.ptr(out), N.ptr(grad), N.stream()
    for a, s, lead, length in ((A, 3, 0, L), (A, 0, 0, L), (A, -2, 0, L), (A, S, 2, L), (A, S, -1, L), (A, S, 1, 0), (0, S, 1, L)):
        assert lib.ap_nes_perturb(px, po, SIGMA, SEED, DRAW, a, s, lead, length, st) == -22, (a, s, lead, length)
        assert b"ap_nes_perturb" in lib.ap_last_error()
    assert lib.ap_nes_perturb(None, po, SIGMA, SEED, DRAW, A, S, 1, L, st) == -22
    assert lib.ap_nes_perturb(px, None, SIGMA, SEED, DRAW, A, S, 1, L, st) == -22
    for a, s, length in ((A, 3, L), (A, 0, L), (A, -2, L), (A, S, 0), (0, S, L)):
        for acc in (0, 1):
            assert lib.ap_nes_grad(pl, pg, SEED, DRAW, a, s, length, acc, st) == -22, (a, s, length)
            assert b"ap_nes_grad" in lib.ap_last_error()
    assert lib.ap_nes_grad(None, pg, SEED, DRAW, A, S, L, 0, st) == -22
    assert lib.ap_nes_grad(pl, None, SEED, DRAW, A, S, L, 0, st) == -22
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((grad == SENTINEL).all())
