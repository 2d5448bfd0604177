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


def frame_maskers(p, bark, ath):
    """Maskers of one normalised fp32 PSD frame p [1025]: (bins that pass the local-maximum and ATH filters, bins kept by the
    bark-distance pass, their smoothed levels)."""
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
    return k, k[keep], m[keep]


def frame_threshold(p, bark, ath):
    """Global threshold in dB (float64) of one normalised fp32 PSD frame p [1025]."""
    _, k, m = frame_maskers(p, bark, ath)
    s = np.zeros(len(bark))
    for kj, mj in zip(k, m):
        dz = bark - bark[kj]
        spread = 27 * dz
        spread[dz > 0] = (-27 + 0.37 * max(mj - 40, 0)) * dz[dz > 0]
        s = s + 10 ** ((mj + (-6.025 - 0.275 * bark[kj]) + spread) / 10)
    with np.errstate(divide="ignore"):
        return 10 * np.log10(s + 10 ** (ath / 10))


def normalised(psd_db):
    """The clip maximum of an un-normalised fp32 PSD and the PSD shifted to 96 dB in fp32, as the kernel does (96.0f - mx, then
    shift + p)."""
    psd_db = np.asarray(psd_db, dtype=np.float32)
    mx = psd_db.max()
    return (np.float32(96.0) - mx) + psd_db, mx


def threshold_from_psd(psd_db, bark, ath):
    """(threshold dB fp32 [1025, F], clip maximum fp32) of an un-normalised fp32 PSD in dB [F, 1025], the layout the kernel
    stores it in."""
    p, mx = normalised(psd_db)
    thr = np.zeros((p.shape[1], p.shape[0]), dtype=np.float32)
    for f in range(p.shape[0]):
        thr[:, f] = frame_threshold(p[f], bark, ath)
    return thr, mx


def threshold(x, hop=512, sample_rate=16000):
    """(threshold dB fp32 [1025, F], psd_max fp32) of a clip x (L,)."""
    m = PsychoacousticMasker(hop_size=hop, sample_rate=sample_rate)
    p, _ = psd_db(np.asarray(x, dtype=np.float32), hop)
    return threshold_from_psd(np.ascontiguousarray(p.T), m.bark, m.absolute_threshold_hearing)


def stabilised(thr_db, psd_max):
    return 10 ** (np.asarray(thr_db, dtype=np.float32) * 0.1), 10 ** (np.asarray(psd_max, dtype=np.float32) * 0.1)


def _power(d, psd_max_stab, hop):
    """fp64 normalised PSD of the perturbation d [B, L] (torch): [B, 1025, F]."""
    X = torch.stft(d, n_fft=N, hop_length=hop, win_length=N, center=False, window=torch.hann_window(N, dtype=torch.float64),
                   return_complex=True)
    return 10.0 ** 9.6 / torch.tensor(np.asarray(psd_max_stab, dtype=np.float64)).reshape(-1, 1, 1) \
        * (np.sqrt(8.0 / 3.0) * X.abs() / N) ** 2


def loss_and_grad(delta, thr_stab, psd_max_stab, hop=512):
    """fp64 autograd of the hinge loss: delta [B, L] -> (loss [B], grad [B, L]), numpy float64."""
    d = torch.tensor(np.asarray(delta, dtype=np.float64).reshape(len(thr_stab), -1), requires_grad=True)
    P = _power(d, psd_max_stab, hop)
    loss = torch.relu(P - torch.tensor(np.asarray(thr_stab, dtype=np.float64))).mean(dim=(1, 2))
    loss.sum().backward()
    return loss.detach().numpy(), d.grad.numpy()


def power(delta, psd_max_stab, hop=512):
    """The fp64 normalised PSD P [B, 1025, F] the hinge compares with the threshold, numpy float64."""
    d = torch.tensor(np.asarray(delta, dtype=np.float64).reshape(np.asarray(psd_max_stab).size, -1))
    return _power(d, psd_max_stab, hop).numpy()


def active_share(delta, thr_stab, psd_max_stab, hop=512):
    """Share of the (bin, frame) cells of each clip where the fp64 hinge is positive: [B]."""
    return (power(delta, psd_max_stab, hop) > np.asarray(thr_stab, dtype=np.float64)).mean(axis=(1, 2))


# ---- seeded clips for the edge tests (tests/test_gpu_psy_edges.py runs them on the kernels, tests/test_psy_cpu.py asserts on
# the restatement that each really contains what its name claims) ----
EDGE_L = 2048 + 5 * 512 + 300
SILENT = slice(2560, 5120)                          # frame 5 of a hop-512 clip of EDGE_L samples lies wholly inside


def _noise(rng, L, sd):
    return (sd * rng.standard_normal(L)).astype(np.float32)


def edge_clips(seed=20):
    """name -> (clip fp32 [L], hop); sample rate 16 kHz throughout."""
    rng = np.random.default_rng(seed)
    n = np.arange(EDGE_L)
    clips = {
        "noise": (_noise(rng, EDGE_L, 0.2), 512),
        "one_frame": (_noise(rng, N, 0.2), 512),
        "hop2048": (_noise(rng, 3 * 2048 + 17, 0.2), 2048),
        "hop700": (_noise(rng, 2048 + 3 * 700 + 699, 0.2), 700),
        "quiet": (_noise(rng, EDGE_L, 1e-6), 512),
        "constant": (np.full(EDGE_L, 0.25, dtype=np.float32), 512),
    }
    x = _noise(rng, EDGE_L, 0.2)
    x[SILENT] = 0
    clips["silent_middle"] = (x, 512)
    tones = 0.5 * np.sin(2 * np.pi * n / N) + 0.5 * np.sin(2 * np.pi * 1023 * n / N)
    clips["end_bins"] = ((tones + 1e-3 * rng.standard_normal(EDGE_L)).astype(np.float32), 512)
    x = np.zeros(EDGE_L, dtype=np.float32)
    x[[600, 4000]] = 0.5                            # every frame holds exactly one of the two: |X| is flat up to rounding
    clips["impulses"] = (x, 512)
    return clips


def loudness_batch(seed=21):
    """Three clips of EDGE_L samples whose maxima lie orders of magnitude apart, the third with a silent frame: [3, L]."""
    rng = np.random.default_rng(seed)
    x = np.stack([_noise(rng, EDGE_L, 1.0), _noise(rng, EDGE_L, 1e-3), _noise(rng, EDGE_L, 0.2)])
    x[2, SILENT] = 0
    return x


LOSS_CASES = ((512, 2048), (2048, 6161), (700, 4847), (256, 3583), (64, 2309), (1, 2060))


def loss_case(hop, L, times_sd, seed=24):
    """(x [2, L], delta [2, L]) fp32: clips x ~ 0.2 N(0, 1) and a perturbation with times_sd times their deviation.  At hop 1
    the 13 frames are nearly one frame, so a clip's active share scatters by +-0.03 around 0.23; the seed is one of those at
    which the fp64 restatement puts every clip of every case inside [0.2, 0.8] (tests/test_psy_cpu.py asserts it)."""
    rng = np.random.default_rng([seed, hop, L])
    x = np.stack([_noise(rng, L, 0.2), _noise(rng, L, 0.2)])
    delta = np.stack([_noise(rng, L, 0.2 * times_sd), _noise(rng, L, 0.2 * times_sd)])
    return x, delta
