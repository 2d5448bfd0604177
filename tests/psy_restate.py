"""numpy / torch-fp64 restatement of the attack's stage-2 masker and hinge loss (robustness_eval/white_box_attack.py:36-273,
:610-710), written from the arithmetic DESIGN.md 3.9 and INTEGRATION.md 1b describe.  Test infrastructure only: the CPU
tests pin it to the reference's recorded outputs, the GPU tests pin the kernels to it."""
import numpy as np
import torch

from audiopure_amd.robustness_eval.psychoacoustic import PsychoacousticMasker, hann_periodic

N = 2048


def psd_db(x, hop):
    """fp32 PSD in dB [1025, F] and its maximum: float64 rFFT of window64 * frame rounded to complex64, then fp32."""
    F = 1 + (len(x) - N) // hop
    frames = np.stack([x[f * hop:f * hop + N] for f in range(F)], axis=1).astype(np.float32)
    X = np.fft.rfft(hann_periodic(N)[:, None] * frames, axis=0).astype(np.complex64)
    with np.errstate(divide="ignore"):
        p = (20 * np.log10(np.abs(float(np.sqrt(8.0 / 3.0)) * X / N))).clip(min=-200)
    return p, p.max()


def frame_threshold(p, bark, ath):
    """Global threshold in dB (float64) of one normalised fp32 PSD frame p [1025]."""
    k = np.nonzero((p[1:-1] > p[:-2]) & (p[1:-1] > p[2:]))[0] + 1
    m = 10 * np.log10(np.sum([10 ** (p[k + i] / 10) for i in (-1, 0, 1)], axis=0))
    sel = m > ath[k]
    k, m = k[sel], m[sel]
    keep = np.ones(len(k), dtype=bool)
    ip = 0
    for i in range(1, len(k)):                     # positions in the list index the bark table, as the reference does
        if bark[i] - bark[ip] < 0.5:
            if m[ip] < m[i]:
                keep[ip], ip = False, ip + 1
            else:
                keep[i] = False
        else:
            ip = i
    k, m = k[keep], m[keep]
    s = np.zeros(len(bark))
    for kj, mj in zip(k, m):
        dz = bark - bark[kj]
        spread = 27 * dz
        spread[dz > 0] = (-27 + 0.37 * max(mj - 40, 0)) * dz[dz > 0]
        s = s + 10 ** ((mj + (-6.025 - 0.275 * bark[kj]) + spread) / 10)
    with np.errstate(divide="ignore"):
        return 10 * np.log10(s + 10 ** (ath / 10))


def threshold(x, hop=512, sample_rate=16000):
    """(threshold dB fp32 [1025, F], psd_max fp32) of a clip x (L,)."""
    m = PsychoacousticMasker(hop_size=hop, sample_rate=sample_rate)
    p, mx = psd_db(np.asarray(x, dtype=np.float32), hop)
    p = 96.0 - mx + p
    thr = np.zeros_like(p)
    for f in range(p.shape[1]):
        thr[:, f] = frame_threshold(p[:, f], m.bark, m.absolute_threshold_hearing)
    return thr, mx


def stabilised(thr_db, psd_max):
    return 10 ** (np.asarray(thr_db, dtype=np.float32) * 0.1), 10 ** (np.asarray(psd_max, dtype=np.float32) * 0.1)


def loss_and_grad(delta, thr_stab, psd_max_stab, hop=512):
    """fp64 autograd of the hinge loss: delta [B, L] -> (loss [B], grad [B, L]), numpy float64."""
    d = torch.tensor(np.asarray(delta, dtype=np.float64).reshape(len(thr_stab), -1), requires_grad=True)
    X = torch.stft(d, n_fft=N, hop_length=hop, win_length=N, center=False, window=torch.hann_window(N, dtype=torch.float64),
                   return_complex=True)
    P = 10.0 ** 9.6 / torch.tensor(np.asarray(psd_max_stab, dtype=np.float64)).reshape(-1, 1, 1) \
        * (np.sqrt(8.0 / 3.0) * X.abs() / N) ** 2
    loss = torch.relu(P - torch.tensor(np.asarray(thr_stab, dtype=np.float64))).mean(dim=(1, 2))
    loss.sum().backward()
    return loss.detach().numpy(), d.grad.numpy()
