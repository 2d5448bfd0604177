"""Stage 2 of the white-box attack (Qin et al. 2019) on the GPU: the masking threshold and the hinge loss with its gradient
(ap_psy.hip) against the reference's recorded outputs (tests/golden/golden_psy_v1.npz) and the fp64 restatement
(tests/psy_restate.py), finite differences, determinism across batch sizes, and stage-2 iterations through a native
AcousticSystem with torch.stft unavailable."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import psy_restate as R  # noqa: E402
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.robustness_eval import psychoacoustic as P  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIPS = ("noise", "tones", "silent", "hop256", "sr44k")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_psy_v1.npz"))


@pytest.mark.parametrize("name", CLIPS)
def test_threshold_matches_the_reference_in_every_bin_and_frame(G, dev, name):
    hop, sr = int(G[f"thr/{name}/hop"]), int(G[f"thr/{name}/sr"])
    m = P.PsychoacousticMasker(hop_size=hop, sample_rate=sr)
    x = torch.from_numpy(G[f"thr/{name}/x"]).to(dev)[None]
    stab, pstab, db, pdb = (t.cpu().numpy() for t in m.threshold_and_psd_maximum(x, db=True))
    want = G[f"thr/{name}/db"]
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(db[0]), fin) and np.all(db[0][~fin] == want[~fin])     # -inf where the reference has it
    assert np.abs(db[0][fin] - want[fin]).max() <= 1e-3
    want_stab, want_pstab = R.stabilised(want, G[f"thr/{name}/psd_max"])
    assert np.array_equal(stab[0] == 0, want_stab == 0)
    nz = want_stab != 0
    assert np.abs(stab[0][nz] / want_stab[nz] - 1).max() <= 2e-4
    assert abs(float(pdb[0]) - float(G[f"thr/{name}/psd_max"])) <= 1e-5
    assert abs(float(pstab[0]) / float(want_pstab) - 1) <= 2e-5


def test_numpy_contract_of_calculate_threshold_and_psd_maximum(G, dev):
    thr, pmax = P.PsychoacousticMasker().calculate_threshold_and_psd_maximum(G["thr/tones/x"])
    assert thr.shape == (1025, 13) and thr.dtype == np.float32 and isinstance(pmax, np.float32)
    assert np.abs(thr - G["thr/tones/db"]).max() <= 1e-3


def test_loss_and_grad_along_the_recorded_attack_trajectory(G, dev):
    thr = torch.from_numpy(G["traj/thr_stab"]).to(dev)
    pm = torch.from_numpy(G["traj/psd_max_stab"]).to(dev)
    for i in range(G["traj/delta"].shape[0]):
        grad, loss = P.masking_threshold_loss_and_grad(torch.from_numpy(G["traj/delta"][i]).to(dev), thr, pm)
        assert grad.shape == (2, 1, 6144) and loss.shape == (2,)
        want_l, want_g = G["traj/loss"][i], G["traj/grad"][i]
        assert np.abs(loss.cpu().numpy() / want_l - 1).max() <= 1e-5, (i, loss, want_l)
        g = grad.cpu().numpy()
        for b in range(2):
            assert np.abs(g[b] - want_g[b]).max() <= 1e-4 * np.abs(want_g[b]).max(), (i, b)
    # the thresholds the trajectory ran on, from the clean clips
    stab, pstab = P.PsychoacousticMasker().threshold_and_psd_maximum(torch.from_numpy(G["traj/x"]).to(dev))
    want = G["traj/thr_stab"]
    nz = want != 0
    assert np.array_equal(stab.cpu().numpy() == 0, ~nz)
    assert np.abs(stab.cpu().numpy()[nz] / want[nz] - 1).max() <= 2e-4
    assert np.abs(pstab.cpu().numpy() / G["traj/psd_max_stab"] - 1).max() <= 2e-5


def _random_case(dev, B=3, L=9000, seed=4, delta_sd=0.01):
    g = torch.Generator().manual_seed(seed)
    x = (0.2 * torch.randn(B, 1, L, generator=g)).to(dev)
    delta = (delta_sd * torch.randn(B, 1, L, generator=g)).to(dev)
    thr, pm = P.PsychoacousticMasker().threshold_and_psd_maximum(x)
    return delta, thr, pm


@pytest.mark.parametrize("delta_sd", (0.01, 0.4))
def test_gradient_against_fp64_autograd_and_finite_differences(dev, delta_sd):
    """delta_sd 0.01 is a stage-2 perturbation: the hinge is active in well under 1 % of the cells.  At 0.4, twice the clips'
    deviation, it is active in most of them, so a threshold read from the wrong cell cannot pass."""
    delta, thr, pm = _random_case(dev, delta_sd=delta_sd)
    if delta_sd == 0.4:
        share = R.active_share(delta[:, 0].cpu().numpy(), thr.cpu().numpy(), pm.cpu().numpy())
        assert np.all(share >= 0.2) and np.all(share <= 0.8), share
    grad, loss = P.masking_threshold_loss_and_grad(delta, thr, pm)
    want_l, want_g = R.loss_and_grad(delta.cpu().numpy(), thr.cpu().numpy(), pm.cpu().numpy())
    assert np.abs(loss.cpu().numpy() / want_l - 1).max() <= 1e-5
    g = grad[:, 0].double().cpu().numpy()
    for b in range(3):
        assert np.abs(g[b] - want_g[b]).max() <= 1e-4 * np.abs(want_g[b]).max()
    L = delta.shape[-1]
    assert float(grad[..., 2048 + 13 * 512:].abs().max()) == 0.0          # samples past the last frame (F = 14)
    # central differences of the native loss on the largest-gradient coordinates of clip 0
    # (the loss is quadratic in delta: at delta_sd 0.4 a step of 1e-3 changes it by 7e-6 of itself, a hundred fp32 ulps, and
    # rounding alone would cost 1e-2 of the 2e-2 allowed; ten times the step keeps it at 1e-3, the hinge's kinks at 3e-3)
    for t in np.argsort(-np.abs(g[0][:L - 900]))[:3]:
        h = 1e-3 if delta_sd == 0.01 else 1e-2
        dp, dm = delta.clone(), delta.clone()
        dp[0, 0, t] += h
        dm[0, 0, t] -= h
        lp = P.masking_threshold_loss_and_grad(dp, thr, pm)[1][0].double()
        lm = P.masking_threshold_loss_and_grad(dm, thr, pm)[1][0].double()
        fd = float(lp - lm) / (2 * h)
        assert abs(fd - g[0][t]) <= 2e-2 * abs(g[0][t]), (t, fd, g[0][t])


def test_outputs_are_deterministic_and_independent_of_the_batch(dev):
    g = torch.Generator().manual_seed(9)
    x = (0.2 * torch.randn(64, 1, 16000, generator=g)).to(dev)
    delta = (0.01 * torch.randn(64, 1, 16000, generator=g)).to(dev)
    m = P.PsychoacousticMasker()
    t1, p1 = m.threshold_and_psd_maximum(x)
    t2, p2 = m.threshold_and_psd_maximum(x)
    g1, l1 = P.masking_threshold_loss_and_grad(delta, t1, p1)
    g2, l2 = P.masking_threshold_loss_and_grad(delta, t2, p2)
    for a, b in ((t1, t2), (p1, p2), (g1, g2), (l1, l2)):
        assert torch.equal(a, b)
    ts, ps = m.threshold_and_psd_maximum(x[:2].clone())
    gs, ls = P.masking_threshold_loss_and_grad(delta[:2].clone(), ts, ps)
    for a, b in ((ts, t1[:2]), (ps, p1[:2]), (gs, g1[:2]), (ls, l1[:2])):
        assert torch.equal(a, b)


def test_stage_2_iterations_through_a_native_acoustic_system_without_torch_stft(dev, monkeypatch):
    """white_box_attack.py:474-608 drives the hooks as below: thresholds once from x, then per iteration model(x + delta),
    criterion(...).backward(), the hinge loss gradient, delta -= lr (grad_net + alpha grad_theta), clamp."""
    from audiopure_amd.acoustic_system import AcousticSystem
    from audiopure_amd.audio_models.M5.M5Net import M5
    from audiopure_amd.diffusion_models.diffwave_ddpm import DiffWave
    from audiopure_amd.diffusion_models.diffwave_sde import RevDiffWave
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams

    def no_stft(*a, **k):
        raise AssertionError("torch.stft was called")
    monkeypatch.setattr(torch, "stft", no_stft)
    cfg = synth.mini_wavenet_config(64, 12, 12)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, 1).items()})
    dw = DiffWave(model=net.to(dev), diffusion_hyperparams=calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG),
                  reverse_timestep=2)
    runner = RevDiffWave.from_model(dw, types.SimpleNamespace(t=2, rand_t=False, t_delta=0, use_bm=False, sample_step=1,
                                                              score_type="guided_diffusion"))
    m5 = M5(n_input=1, n_output=10)
    m5.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.m5_state_dict(10).items()})
    model = AcousticSystem(classifier=m5.to(dev).eval(), transform=None, defender=runner, defense_type="wave")
    x = torch.from_numpy(synth.waveforms(2, 16000, seed=31)).to(dev)
    y = torch.tensor([4, 6], device=dev)
    dw.set_noise_source(("philox", 5, 0))
    masker = P.PsychoacousticMasker()
    thr, pm = masker.threshold_and_psd_maximum(x)
    delta = torch.zeros_like(x, requires_grad=True)
    delta.data = 0.002 * torch.sign(torch.randn(x.shape, generator=torch.Generator().manual_seed(3))).to(dev)
    lr, alpha = 2.0 ** -15, torch.full((2, 1, 1), 0.05, device=dev)
    losses = []
    for _ in range(3):
        out = model(x + delta)
        torch.nn.functional.cross_entropy(out, y).backward()
        g_theta, loss_theta = P.masking_threshold_loss_and_grad(delta, thr, pm)
        assert g_theta.shape == delta.grad.shape and torch.isfinite(g_theta).all()
        delta.data = delta.data - lr * (delta.grad.data + alpha * g_theta)
        delta.data = (x + delta.data).clamp(-1, 1) - x
        delta.grad.zero_()
        losses.append(loss_theta.cpu())
    losses = torch.stack(losses)
    assert torch.isfinite(losses).all() and float(losses.min()) > 0
