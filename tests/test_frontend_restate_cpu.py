"""CPU side of test_gpu_frontends.py and test_gpu_unet_primitives.py: pins the float64 restatements of frontend_restate.py
to the golden-pinned fp32 oracle, and checks -- on the float64 reference alone -- every condition on the inputs that the GPU
tests rely on, so that a GPU run is never the first place one of them fails.  The float32-arithmetic errors that the GPU
tolerances are derived from are re-measured here against the constants recorded there."""
import numpy as np
import pytest
import torch

import frontend_restate as R
from oracle import diffwave_oracle as O

PIN = 5e-5                     # restatement vs the fp32 oracle; measured 1.2e-6 (M5 log-probabilities), 1.1e-5 dB (mel)


@pytest.mark.parametrize("L,nc,no", [(6848, 32, 10), (8000, 32, 35), (16037, 32, 10), (16000, 64, 64)])
def test_m5_restatement_matches_the_oracle(L, nc, no):
    sd, x = R.m5_weights(no, nc), R.m5_clips(8, L)
    lp, pre = R.m5_forward(sd, x.double())
    assert lp.shape == (8, no) and lp.dtype == torch.float64
    P1, Q1, Q2, Q3, Q4 = R.m5_dims(L)
    assert [p.shape[1:] for p in pre] == [(nc, P1), (nc, Q1 - 2), (2 * nc, Q2 - 2), (2 * nc, Q3 - 2)]
    assert float((lp - O.m5_forward(sd, x).double()).abs().max()) < PIN


def test_m5_lengths_are_the_cases_they_are_named_for():
    """The lengths of the GPU tests sit where launch_m5 / launch_m5_bwd / m5_stage_bwd branch (ap_frontend.hip)."""
    assert R.m5_dims(6848)[4] == 1 and R.m5_dims(6847)[4] == 0                 # smallest legal clip, first illegal one
    assert R.m5_dims(16016)[0] % 4 == 1 and R.m5_dims(16037)[0] % 4 == 2       # windows dropped by stage 1's floor pooling
    # 37 samples without a gradient: 5 that no conv-1 window reads and 32 read only by the two windows the pooling drops
    assert (16037 - 80) % 16 == 5 and (4 * R.m5_dims(16037)[1] - 1) * 16 + 80 == 16000
    for L in (8000, 16000):
        assert (L - 80) % 16 == 0 and R.m5_dims(L)[0] % 4 == 0                 # (what the earlier tests had only)

    def fwd_bytes(L, nc):
        _, Q1, Q2, Q3, Q4 = R.m5_dims(L)
        act = nc * Q1 + nc * Q2 + 2 * nc * Q3 + 2 * nc * Q4 + 2 * nc + 64
        staged = (act + L) * 4 <= 150 * 1024
        return (act + (L if staged else 0)) * 4, staged

    def bwd_bytes(L, nc):
        _, Q1, Q2, Q3, Q4 = R.m5_dims(L)
        act = nc * Q1 + nc * Q2 + 2 * nc * Q3 + 2 * nc * Q4
        return (act + 2 * nc + 128) * 4 + ((act + 15) & ~15)

    assert fwd_bytes(16000, 32)[1] and not fwd_bytes(32000, 32)[1]
    assert fwd_bytes(48000, 32) == (134784, False)
    assert fwd_bytes(16000, 64) == (152832, True) and not fwd_bytes(16400, 64)[1]
    assert fwd_bytes(64000, 32) == (179456, False)                             # refused: > 160 KB
    for L, nc, _ in R.M5_FWD_CASES:
        assert fwd_bytes(L, nc)[0] <= 160 * 1024
    for L, nc in R.M5_GRAD_CASES:
        assert bwd_bytes(L, nc) <= 160 * 1024
    assert bwd_bytes(48000, 32) == 168608 and bwd_bytes(24000, 64) == 167744   # refused, where the forward is not:
    assert fwd_bytes(48000, 32)[0] == 134784 and fwd_bytes(24000, 64)[0] == 134144


M5_F32_GRAD_ERR = 3.3e-7       # recorded in test_gpu_frontends.py, whose bound on decided clips is 8 x this
# a float32 error moves with the summation order of the machine's BLAS and vector maths: a re-measurement confirms a recorded
# figure when it is no more than this factor above it
REMEASURED = 1.5


@pytest.mark.parametrize("L,nc", R.M5_GRAD_CASES)
def test_m5_gradient_cases_have_enough_decided_clips(L, nc):
    """At tau = 7e-6 the float64 reference has 6, 6, 6, 6, 6, 4 and 4 decided clips of 8; on them float32 autograd of the same
    formula is within 3.3e-7 of float64 (per clip, max |d| / max |ref|), and its pre-pool activations within tau / 2."""
    no = 64 if nc == 64 else 10
    sd, x, v = R.m5_weights(no, nc), R.m5_clips(8, L), R.m5_cotangent(8, no)
    xr = x.double().requires_grad_(True)
    lp, pre = R.m5_forward(sd, xr)
    (g64,) = torch.autograd.grad(lp, xr, v.double())
    dec = R.m5_decided(pre, R.M5_TAU)
    assert int(dec.sum()) >= R.M5_MIN_DECIDED
    assert int(dec.sum()) == (4 if nc == 64 else 6)                            # (measured)
    xf = x.clone().requires_grad_(True)
    lpf, pref = R.m5_forward(sd, xf)
    (g32,) = torch.autograd.grad(lpf, xf, v)
    assert max(float((a.detach().double() - b.detach()).abs().max()) for a, b in zip(pref, pre)) < R.M5_TAU / 2
    err = (g32.double() - g64).abs().amax(dim=(1, 2)) / g64.abs().amax(dim=(1, 2))
    assert float(err[dec].max()) <= REMEASURED * M5_F32_GRAD_ERR
    if L == 16037:
        assert float(g64[..., 16000:].abs().max()) == 0.0                      # nothing that survives the pooling reads the tail


def test_m5_decided_flags_near_ties_and_near_zero_maxima():
    pre = [torch.tensor([[[3.0, 1.0, 0.5, 0.2, -1.0, -2.0, -3.0, -4.0, 9.0]]], dtype=torch.float64)]      # the 9th is dropped
    assert bool(R.m5_decided(pre, 1e-3)[0])
    for i, val in ((1, 3.0 - 1e-4), (0, 1.0 + 1e-4)):                          # a tie at the top of a positive window
        p = [pre[0].clone()]
        p[0][0, 0, i] = val
        assert not bool(R.m5_decided(p, 1e-3)[0])
    p = [pre[0].clone()]
    p[0][0, 0, :4] = torch.tensor([1e-4, -1.0, -1.0, -1.0], dtype=torch.float64)   # a maximum next to the ReLU's kink
    assert not bool(R.m5_decided(p, 1e-3)[0])
    p[0][0, 0, 0] = -1e-4
    assert not bool(R.m5_decided(p, 1e-3)[0])
    p[0][0, 0, 4:8] = torch.tensor([-5.0, -5.0 + 1e-9, -6.0, -7.0], dtype=torch.float64)
    p[0][0, 0, 0] = 2.0
    assert bool(R.m5_decided(p, 1e-3)[0])                                      # a tie in a closed window decides nothing


@pytest.mark.parametrize("n_mels", [32, 40, 128])
@pytest.mark.parametrize("L", [1, 513, 5000, 16000])
def test_mel_restatement_matches_the_oracle(L, n_mels):
    x = R.mel_noise(3, L)
    for mode in (0, 1):
        got = R.mel_db(x.double(), n_mels, mode)
        ref = O.melspec_db(x, n_mels=n_mels, ref_max=bool(mode), top_db=80.0 if mode else None)
        assert got.shape == ref.shape == (3, 1, n_mels, 1 + L // 512)
        assert float((got - ref.double()).abs().max()) < PIN


@pytest.mark.parametrize("n_mels", R.MEL_FWD_MELS)
def test_mel_stretch_clip_reaches_the_floor_from_both_causes(n_mels):
    """Mode 1 on the four-stretch clip: elements at exactly -80 whose power is under the 1e-10 clamp (the zeros), elements
    at exactly -80 whose power is above it (the very quiet stretch), and elements above -80.  Measured floor share 0.44."""
    x = R.mel_stretch_clips(R.MEL_FWD_STRETCHES)
    mel = R.mel_power(x.double(), n_mels)
    out = R.mel_db(x.double(), n_mels, 1)[:, 0]
    for b in range(x.shape[0]):
        floor = out[b] == -80.0
        assert int((floor & (mel[b] <= 1e-10)).sum()) > 0 and int((floor & (mel[b] > 1e-10)).sum()) > 0
        assert int((out[b] > -80.0).sum()) > 0 and float(out[b].max()) == 0.0
        assert 0.3 < float(floor.float().mean()) < 0.6
    for mode in (0, 1):
        ref = O.melspec_db(x, n_mels=n_mels, ref_max=bool(mode), top_db=80.0 if mode else None)
        assert float((R.mel_db(x.double(), n_mels, mode) - ref.double()).abs().max()) < PIN


@pytest.mark.parametrize("n_mels", R.MEL_GRAD_MELS)
def test_mel_gradient_inputs_stay_away_from_the_clamp(n_mels):
    for L in R.MEL_GRAD_L:
        assert R.mel_clamp_is_far(R.mel_power(R.mel_noise(2, L).double(), n_mels))
    x = R.mel_stretch_clips(R.MEL_GRAD_STRETCHES)
    mel = R.mel_power(x.double(), n_mels)
    assert R.mel_clamp_is_far(mel)
    assert int((mel < 1e-12).sum()) > 0                                        # the clamp branch is entered ...
    silent = R.mel_silent_samples(mel, x.shape[-1])
    assert silent.sum(dim=1).tolist() == [6656, 5120]                          # ... and whole stretches of dx must be 0
    xr = x.double().requires_grad_(True)
    (g,) = torch.autograd.grad(R.mel_db(xr, n_mels), xr, R.mel_cotangent("s", 2, n_mels, x.shape[-1]).double())
    assert float(g[:, 0][silent].abs().max()) == 0.0
    assert bool(torch.isfinite(g).all())
    # the gradient scales as 1 / power: the quiet stretch dwarfs the loud one, which only a local scale looks at
    loud, quiet = g[0, 0, :4096].abs().max(), g[0, 0, 4096:8192].abs().max()
    assert float(quiet) > 100 * float(loud) > 0


def test_mel_silent_samples_counts_covering_frames():
    mel = torch.ones(1, 2, 5, dtype=torch.float64)                             # L = 2048: frames 0..4
    mel[0, :, 2] = 0.0
    assert int(R.mel_silent_samples(mel, 2048).sum()) == 0                     # every sample has a covering frame with power
    mel[0, :, 1:4] = 0.0
    mel[0, :, 0] = 0.0
    assert R.mel_silent_samples(mel, 2048)[0].nonzero().flatten().tolist() == list(range(0, 1024))


@pytest.mark.parametrize("case", R.GN_BWD_CASES)
def test_groupnorm_restatement_and_its_relu_condition(case):
    import torch.nn.functional as F
    B, C, H, W, G, act, use_ss = case
    x, g, b, ss, _ = R.gn_inputs(B, C, H, W)
    y, y1 = R.groupnorm_film_act(x.double(), g.double(), b.double(), ss.double() if use_ss else None, G, act)
    ref = F.group_norm(x, G, g, b, 1e-5)
    if use_ss:
        ref = ref * (1 + ss[:, :C, None, None]) + ss[:, C:, None, None]
    ref = ref * torch.sigmoid(ref) if act == 2 else ref.relu() if act == 1 else ref
    assert float((y - ref.double()).abs().max()) < PIN
    if act == 1:
        dec = R.groupnorm_decided(y1, G, R.GN_TAU)
        assert dec.shape == (B, G)
        assert float((~dec).float().mean()) <= R.GN_MAX_SKIPPED               # measured: 0 of 64 slabs in both cases
        assert 0.05 < float((y1 > 0).float().mean()) < 0.95                    # the ReLU is open and shut
        y1[0, 0, 0, 0] = 0.5 * R.GN_TAU
        assert not bool(R.groupnorm_decided(y1, G, R.GN_TAU)[0, 0])


# float32 torch against float64, max |d| / max |ref|, (forward, gradient): measured values the peaked cases' tolerances are
# 4 x of in test_gpu_unet_primitives.py
ATT_F32_ERR = {(64, 128, 2): (6.7e-6, 3.9e-6), (32, 100, 1): (2.7e-6, 1.2e-6), (64, 256, 3): (7.0e-6, 3.9e-6)}


@pytest.mark.parametrize("ch,T,heads,peaked", R.ATT_CASES)
def test_attention_restatement_and_the_float32_error_of_the_peaked_cases(ch, T, heads, peaked):
    qkv, do = R.att_inputs(ch, T, heads, peaked)
    assert 2 * ch * T * 4 <= 160 * 1024                                        # K and V of one head fit the LDS
    q64 = qkv.double().requires_grad_(True)
    o64 = R.qkv_attention(q64, heads)
    (g64,) = torch.autograd.grad(o64, q64, do.double())
    q, k, v = torch.split(qkv.reshape(R.ATT_B * heads, 3 * ch, T), ch, dim=1)  # the legacy formulation (scale on q and on k)
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * ch ** -0.25, k * ch ** -0.25), dim=-1)
    legacy = torch.einsum("bts,bcs->bct", w, v).reshape(R.ATT_B, heads * ch, T)
    assert float((o64.detach() - legacy.double()).abs().max()) < PIN
    if peaked:
        q32 = qkv.clone().requires_grad_(True)
        o32 = R.qkv_attention(q32, heads)
        (g32,) = torch.autograd.grad(o32, q32, do)
        rel = lambda a, r: float((a.detach().double() - r.detach()).abs().max() / r.detach().abs().max())
        assert rel(o32, o64) <= REMEASURED * ATT_F32_ERR[(ch, T, heads)][0]
        assert rel(g32, g64) <= REMEASURED * ATT_F32_ERR[(ch, T, heads)][1]
        assert float(torch.softmax(torch.einsum("bct,bcs->bts", q, k).double() / ch ** 0.5, dim=-1).max()) > 0.5   # peaked


def test_attention_shapes_sit_on_both_sides_of_the_limits():
    assert 2 * 64 * 300 * 4 == 153600 and 2 * 64 * 321 * 4 == 164352 > 160 * 1024
    scalar = [(ch, T) for ch, T, _, _ in R.ATT_CASES if T % 4]
    assert (8, 17) in scalar and (32, 301) in scalar
    assert any(T % 4 == 0 and T > 256 for _, T, _, _ in R.ATT_CASES)


TEMB_NUMPY_F32_ERR = {2: 3.0e-8, 128: 5.0e-8}      # recorded in test_gpu_unet_primitives.py (tolerance: 4 x)


@pytest.mark.parametrize("dim", [2, 128])
def test_timestep_embedding_reference_and_the_float32_error_of_numpy(dim):
    t, freqs = R.temb_inputs(257, dim)
    ref, a = R.temb_reference(t, freqs)
    assert ref.shape == (257, dim) and a.dtype == np.float32
    assert set(np.unique(t).tolist()) == set(R.TEMB_T)
    got = np.concatenate([np.cos(a), np.sin(a)], axis=1)
    assert got.dtype == np.float32
    assert float(np.abs(got.astype(np.float64) - ref).max()) <= REMEASURED * TEMB_NUMPY_F32_ERR[dim]
    assert np.array_equal(ref[t == 0.0][:, :dim // 2], np.ones_like(ref[t == 0.0][:, :dim // 2]))


@pytest.mark.parametrize("n", R.SMALL_N)
def test_small_kernel_inputs_clip_at_both_ends(n):
    x, eps, z = R.small_inputs(n)
    c = R.PSAMPLE_COEF
    p = np.float32(c["r1"]) * x - np.float32(c["r2"]) * eps
    if n > 1:
        assert p.min() < -1.0 and p.max() > 1.0 and ((p > -1.0) & (p < 1.0)).any()
    on, off = R.psample_forms(x, eps, z, clip=1, **c), R.psample_forms(x, eps, z, clip=0, **c)
    assert len(on) == len(off) == 18 and len(R.psample_forms(x, eps, None, clip=1, **c)) == 9
    if n > 1:
        assert not np.array_equal(on[0], off[0])
    # form 0 is plain float32 numpy in the kernel's written order
    v = np.float32(c["c1"]) * np.clip(p, np.float32(-1), np.float32(1)) + np.float32(c["c2"]) * x
    assert np.array_equal(on[0], v + np.float32(c["sigma"]) * z)
    assert np.array_equal(R.axpbyc_forms(x, eps, 0.3, -1.7, 0.25)[0], (np.float32(0.3) * x + np.float32(-1.7) * eps) + np.float32(0.25))
    assert np.array_equal(R.axpbyc_forms(x, None, 0.3, 0.0, 0.25)[0], np.float32(0.3) * x + np.float32(0.25))
    assert float(R.ulp_distance_to_nearest(on[0], on).max()) == 0.0
    assert float(R.ulp_distance_to_nearest(np.nextafter(on[0], np.float32(np.inf)), on[:1]).min()) >= 0.5
