"""tests/nes_restate.py against the reference's own arithmetic (robustness_eval/_NES.py:19-24 the query batch, :44-52 the
estimate: torch ``cat`` / ``mean`` on the noise tensor) on the Philox draws the kernels regenerate (oracle/philox.py), without
a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nes_restate as R  # noqa: E402
from oracle.philox import philox_normal  # noqa: E402

SHAPES = ((1, 2, 1, 0), (1, 2, 3, 1), (3, 4, 5, 1), (2, 10, 1023, 0), (2, 6, 1025, 1), (3, 10, 4096, 1))


@pytest.mark.parametrize("A,S,L,lead", SHAPES)
def test_restatement_equals_the_reference_arithmetic(A, S, L, lead):
    rng = np.random.default_rng([A, S, L, lead])
    half, sigma = S // 2, 0.001
    z = philox_normal(7, 3, 0, A * half, L).reshape(A, half, L)               # z_p of audio a: utterance a S/2 + p
    x = rng.uniform(-1, 1, (A, L)).astype(np.float32)
    s32 = float(np.float32(sigma))
    # :19-24 in float64
    xt = torch.from_numpy(x).double().unsqueeze(1)                            # [A, 1 (channel), L]
    noise = torch.from_numpy(z).double().unsqueeze(2)                         # [A, S/2, 1, L]
    noise = torch.cat((noise, -noise), 1)
    if lead:
        noise = torch.cat((torch.zeros_like(xt).unsqueeze(1), noise), 1)
    eval_input = (noise * s32 + xt.unsqueeze(1)).view(-1, 1, L)
    got = R.perturb(x, z, sigma, S, lead)
    assert got.shape == (A, S + lead, L) and got.dtype == np.float64
    assert np.array_equal(got.reshape(-1, 1, L), eval_input.numpy())
    if lead:
        assert np.array_equal(got[:, 0], x.astype(np.float64))
    # :39-47
    loss = torch.from_numpy(rng.normal(size=(A * (S + lead),))).view(A, -1)
    if lead:
        loss, noise = loss[..., 1:], noise[:, 1:, :, :]
    want = torch.mean(loss.unsqueeze(2).unsqueeze(3) * noise, 1)[:, 0].numpy()
    got = R.grad(loss.numpy(), z, S)
    assert got.shape == (A, L)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    # the bound sums the magnitudes of the same terms: (S/2 + 1) roundings of at least |estimate| each, and at S = 2 (one term)
    # exactly that
    bound = R.grad_bound(loss.numpy(), z, S)
    assert bound.shape == (A, L) and np.all(bound >= (half + 1) * R.U * np.abs(got) * (1 - 1e-12))
    if S == 2:
        assert np.allclose(bound, 2 * R.U * np.abs(got), rtol=1e-12, atol=0)


def test_antithetic_pairs_cancel_in_the_estimate():
    z = philox_normal(1, 0, 0, 4, 9).reshape(2, 2, 9)
    same = np.tile(np.array([[1.5, -2.0]]), (2, 2))                          # loss[p] == loss[p + S/2]: no gradient signal
    assert np.all(R.grad(same, z, 4) == 0) and np.all(R.grad_bound(same, z, 4) == 0)
    one = np.zeros((2, 4))
    one[0, 1], one[1, 2] = 4.0, 4.0                                           # copy 1 of audio 0: +z_1; copy 2 of audio 1: -z_0
    g = R.grad(one, z, 4)
    assert np.array_equal(g[0], z[0, 1].astype(np.float64)) and np.array_equal(g[1], -z[1, 0].astype(np.float64))
