"""float64 restatement of the NES query batch and gradient estimate (robustness_eval/_NES.py:14-55) on materialised noise, as
``ap_nes_perturb`` / ``ap_nes_grad`` form them: copy s of audio a is the unperturbed audio (the lead copy of the first batch),
then S/2 copies x + sigma z_p and S/2 copies x - sigma z_p; the estimate is the mean over the S copies of loss * noise with
noise = [z, -z].  Test infrastructure only: tests/test_nes_restate_cpu.py pins it to the reference's own torch arithmetic,
tests/test_gpu_nes_edges.py pins the kernels to it."""
import numpy as np

U = 2.0 ** -24                                      # fp32 unit roundoff


def perturb(x, z, sigma, S, lead):
    """x [A, L], z [A, S/2, L] -> the query batch [A, S + lead, L] in float64.  sigma is used as the fp32 value the kernel
    receives."""
    x, z = np.asarray(x, dtype=np.float64), np.asarray(z, dtype=np.float64)
    A, L = x.shape
    assert z.shape == (A, S // 2, L) and S % 2 == 0 and lead in (0, 1)
    sz = float(np.float32(sigma)) * z
    parts = ([x[:, None]] if lead else []) + [x[:, None] + sz, x[:, None] - sz]
    return np.concatenate(parts, axis=1)


def grad(loss, z, S):
    """loss [A, S], z [A, S/2, L] -> mean over the S copies of loss * noise, noise = [z, -z]: [A, L] in float64."""
    loss, z = np.asarray(loss, dtype=np.float64), np.asarray(z, dtype=np.float64)
    half = S // 2
    assert loss.shape == (z.shape[0], S) and z.shape[1] == half
    w = loss[:, :half] - loss[:, half:]
    return (w[:, :, None] * z).sum(axis=1) / S


def grad_bound(loss, z, S):
    """Worst case of the kernel's fp32 chain against ``grad``: S/2 fmas, each rounding a partial sum no larger than
    sum_p |w_p z_p|, and the division by S: (S/2 + 1) 2^-24 sum_p |w_p z_p| / S per element.  It assumes w_p = loss[p] -
    loss[p + S/2] exact in fp32 (the tests choose such losses)."""
    loss, z = np.asarray(loss, dtype=np.float64), np.asarray(z, dtype=np.float64)
    half = S // 2
    w = loss[:, :half] - loss[:, half:]
    return (half + 1) * U * np.abs(w[:, :, None] * z).sum(axis=1) / S
