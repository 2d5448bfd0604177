"""ap_augment.hip on the GPU: each kernel alone and SpeechCommandsAugment end to end against the float64 restatement
(tests/augment_restate.py).  The bar of every compared quantity is 4 x the error of the wrapped float32 evaluation of the same
restatement on the same inputs, computed here on the CPU; lanes that no transform touches must be bit-exact copies."""
import os
import random

import numpy as np
import pytest
import torch

import augment_restate as R
from audiopure_amd import _native as N
from audiopure_amd.transforms.augment import PAD_MODES, SpeechCommandsAugment, draw_augment

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_aug_v1.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def nan_like(shape, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)


def run_wave(x, t, L_out, dev):
    xd = torch.from_numpy(x).to(dev)
    out = nan_like((len(x), L_out), dev)
    ln, ni, ap = _i32(t.length, dev), _i32(t.n_interp, dev), _i32(t.speed_applied, dev)
    amp, fac = torch.from_numpy(t.amp).to(dev), torch.from_numpy(t.speed_fac).to(dev)
    N.check(N.lib().ap_aug_wave(N.ptr(xd), ln.data_ptr(), N.ptr(amp), fac.data_ptr(), ni.data_ptr(), ap.data_ptr(), N.ptr(out), len(x),
                                x.shape[1], L_out, N.stream()), "ap_aug_wave")
    return out.cpu().numpy()


def run_stft(w, pad_mode, dev):
    wd = torch.from_numpy(w).to(dev)
    nf = 1 + w.shape[1] // R.HOP
    out = nan_like((len(w), nf, R.NBIN, 2), dev)
    N.check(N.lib().ap_stft(N.ptr(wd), N.ptr(out), PAD_MODES[pad_mode], len(w), w.shape[1], N.stream()), "ap_stft")
    return out.cpu().numpy()


def run_vocoder(D, t, dev):
    Dd = torch.from_numpy(R.device_layout(D)).to(dev)
    out = nan_like(tuple(Dd.shape), dev)
    rate, no, ap, sh = torch.from_numpy(t.rate).to(dev), _i32(t.n_out, dev), _i32(t.stretch_applied, dev), _i32(t.shift, dev)
    N.check(N.lib().ap_phase_vocoder_shift(N.ptr(Dd), N.ptr(out), rate.data_ptr(), no.data_ptr(), ap.data_ptr(), sh.data_ptr(), len(D),
                                           D.shape[2], N.stream()), "ap_phase_vocoder_shift")
    return out.cpu().numpy()


def run_mel(D, noise_lane, p, n_mels, dev):
    Dd = torch.from_numpy(R.device_layout(D)).to(dev)
    B = len(noise_lane)
    out = nan_like((B, n_mels, D.shape[2]), dev)
    nl, pd = _i32(noise_lane, dev), torch.from_numpy(np.asarray(p, dtype=np.float32)).to(dev)
    N.check(N.lib().ap_mel_from_stft(N.ptr(Dd), nl.data_ptr(), N.ptr(pd), N.ptr(out), n_mels, B, len(D), D.shape[2], N.stream()), "ap_mel_from_stft")
    return out.cpu().numpy()


def test_wave_interp_pad_and_cut(dev):
    """lengths 9000 / 16000 / 19000 into 16000, factors on both sides of 1 (padded and cut outputs), a last position in (len-1, len),
    and the lanes without a speed change, which are scaled copies to the bit"""
    x, t = R.wave_case()
    got = run_wave(x, t, R.WAVE_L_OUT, dev)
    top = float(np.abs(x).max())
    e32 = egpu = 0.0
    for i, (length, fac, amp) in enumerate(R.WAVE_LANES):
        args = (length, t.amp[i], fac is not None, fac or 1.0, R.WAVE_L_OUT)
        ref, f32 = R.aug_wave(x[i].astype(np.float64), *args), R.aug_wave(x[i], *args)
        assert f32.dtype == np.float32
        if fac is None:
            assert np.array_equal(got[i], f32), i                                  # x * amp in float32, padded or cut
        else:
            n = min(int(t.n_interp[i]), R.WAVE_L_OUT)
            assert not got[i, n:].any()
            e32, egpu = max(e32, float(np.abs(f32 - ref).max()) / top), max(egpu, float(np.abs(got[i] - ref).max()) / top)
    last = int(t.n_interp[0]) - 1
    assert last * t.speed_fac[0] > R.WAVE_LANES[0][0] - 1 and got[0, last] == np.float32(t.amp[0]) * x[0, R.WAVE_LANES[0][0] - 1]
    print(f"ap_aug_wave: {egpu:.2e} of max |x| (float32 restatement {e32:.2e})")
    assert egpu <= R.MARGIN * e32


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("L", [16000, 4000])
def test_stft_both_pad_modes(dev, pad_mode, L):
    x = R.clips(4, L, seed=26)
    x[3] = 0.0
    got = R.from_device_layout(run_stft(x, pad_mode, dev))
    ref = np.stack([R.stft(v.astype(np.float64), pad_mode) for v in x])
    f32 = np.stack([R.stft(v, pad_mode) for v in x])
    assert got.shape == ref.shape == (4, R.NBIN, 1 + L // R.HOP) and f32.dtype == np.complex64
    assert not got[3].any()
    ec, ec32 = R.err_of_max(got, ref), R.err_of_max(f32, ref)
    em, em32 = R.err_of_max(np.abs(got), np.abs(ref)), R.err_of_max(np.abs(f32), np.abs(ref))
    print(f"ap_stft {pad_mode} L={L}: complex {ec:.2e} (float32 {ec32:.2e}), magnitude {em:.2e} (float32 {em32:.2e}) of max |D|")
    assert ec <= R.MARGIN * ec32 and em <= R.MARGIN * em32


@pytest.mark.parametrize("nf", [32, 8])
def test_phase_vocoder_shift_and_fix(dev, nf):
    """rates 0.8 (40 steps, the last ones on the padded columns), 1.2 (27 steps), 0.9137, 1.0 applied (alpha = 0); shifts -8, 0, +8;
    the lanes without a stretch are shifted copies to the bit; at F = 8 a copy shifted by +-8 is empty"""
    D, t = R.vocoder_case(nf)
    raw = run_vocoder(D, t, dev)
    got = R.from_device_layout(raw)
    bar_c, bar_m = (R.MARGIN * e for e in R.vocoder_errors(D, t, True))
    top = float(np.abs(D).max())
    ec = em = 0.0
    for i, (rate, shift) in enumerate(R.VOCODER_LANES[nf]):
        if rate is None:
            assert np.array_equal(raw[i], R.device_layout(R.shift_fix(D[i], shift, nf)[None])[0]), i
            continue
        ref = R.vocoder_shift(D[i].astype(np.complex128), True, rate, shift)
        assert ref.shape == got[i].shape and np.array_equal(got[i] == 0, ref == 0), i          # the same frames survive
        ec, em = max(ec, float(np.abs(got[i] - ref).max()) / top), max(em, float(np.abs(np.abs(got[i]) - np.abs(ref)).max()) / top)
    if nf == 8:
        assert not raw[0].any() and not raw[1].any()
    else:
        assert not np.array_equal(raw[2], R.device_layout(D[2:3])[0])                    # rate 1.0 applied runs the vocoder
    print(f"ap_phase_vocoder_shift F={nf}: complex {ec:.2e} (bar {bar_c:.2e}), magnitude {em:.2e} (bar {bar_m:.2e}) of max |D|")
    assert ec <= bar_c and em <= bar_m


@pytest.mark.parametrize("n_mels", [32, 40])
@pytest.mark.parametrize("nf", [32, 8])
def test_mel_from_stft_with_and_without_noise(dev, nf, n_mels):
    """noise lane -1, p = 0 and p = 0.45; an all-zero clip, whose mel is exactly 0"""
    D, _ = R.vocoder_case(nf)
    D = D.copy()
    D[3] = 0
    noise_lane, p = [-1, 4, len(D) - 1, -1], np.asarray([0.0, 0.0, 0.45, 0.0], dtype=np.float32)
    got = run_mel(D, noise_lane, p, n_mels, dev)
    e32 = egpu = 0.0
    for b, nl in enumerate(noise_lane):
        ref = R.mel_db(D[b].astype(np.complex128), n_mels, D[nl].astype(np.complex128) if nl >= 0 else None, float(p[b]))
        f32 = R.mel_db(D[b], n_mels, D[nl] if nl >= 0 else None, float(p[b]))
        assert f32.dtype == np.float32 and ref.max() == 0.0 and got[b].max() == 0.0
        e32, egpu = max(e32, float(np.abs(f32 - ref).max())), max(egpu, float(np.abs(got[b] - ref).max()))
    assert not got[3].any()
    assert np.array_equal(got[0], run_mel(D, [-1], p[:1], n_mels, dev)[0])
    print(f"ap_mel_from_stft F={nf} n_mels={n_mels}: {egpu:.2e} dB (float32 restatement {e32:.2e} dB)")
    assert egpu <= R.MARGIN * e32


@pytest.fixture(scope="module")
def golden_items():
    g = np.load(GOLDEN)
    samples, bg = R.golden_inputs()
    items = [R.golden_draws(int(g[f"{i}/seed"]), n) for i, n in enumerate(R.GOLDEN_LENGTHS)]
    return samples, bg, items, np.stack([g[f"{i}/mel"] for i in range(len(items))])


@pytest.mark.parametrize("first", [0, 4])
def test_module_replays_the_golden_seeds(dev, golden_items, first):
    """the reference's own classes on eight seeded items (every transform applied and not, five noise mixes) against the module, four
    items to a batch (6 and 7 lanes)"""
    samples, bg, items, want = golden_items
    sel = slice(first, first + 4)
    x, d, want, lengths = samples[sel], R.merge_draws(items[sel]), want[sel], list(R.GOLDEN_LENGTHS[sel])
    assert d.lanes <= 8
    m = SpeechCommandsAugment(bg).to(dev)
    out = m(torch.from_numpy(x).to(dev), lengths, draws=d)
    assert out.shape == (4, 32, 32) and out.dtype == torch.float32
    f32 = R.pipeline(x, bg, d, dtype=np.float32)["mel"]
    ref = R.pipeline(x, bg, d)["mel"]
    e32, egpu = float(np.abs(f32 - want).max()), float(np.abs(out.cpu().numpy() - want).max())
    print(f"SpeechCommandsAugment on golden items {first}..{first + 3}: {egpu:.2e} dB (float32 restatement {e32:.2e} dB; "
          f"float64 restatement without the reference's float32 casts {float(np.abs(ref - want).max()):.2e} dB)")
    assert egpu <= R.MARGIN * e32


def test_module_draws_from_its_own_rng_and_two_runs_give_equal_bits(dev, golden_items):
    samples, bg, _, _ = golden_items
    xd, lengths = torch.from_numpy(samples[:4]).to(dev), list(R.GOLDEN_LENGTHS[:4])
    m = SpeechCommandsAugment(bg, rng=random.Random(7)).to(dev)
    first = m(xd, lengths)
    d = draw_augment(random.Random(7), 4, R.GOLDEN_N_BG, lengths)
    assert 4 < d.lanes <= 8 and d.noise_applied.any() and d.stretch_applied.any() and d.speed_applied.any() and d.shift.any()
    second, third = m(xd, lengths, draws=d), m(xd, lengths, draws=d)
    assert torch.equal(first, second) and torch.equal(second, third)
    assert not torch.equal(first, m(xd, lengths))                               # the rng has moved on


@pytest.mark.parametrize("pad_mode,n_mels", [("constant", 32), ("reflect", 40)])
def test_module_on_quarter_second_clips(dev, pad_mode, n_mels):
    """L = 4000 (8 frames): an unstretched clip shifted by +-8 has no frame left and its mel is exactly 0, as is the all-zero clip's"""
    L, bg = 4000, R.background(2)
    x = R.clips(5, L, seed=27)
    x[2] = 0.0
    d = R.table(6, n_clips=5, n_frames=8, length=[L] * 5 + [16000], source=[0, 1, 2, 3, 4, 1], shift=[8, -8, 0, 3, 0, -2],
                rate=[1.0, 1.0, 1.2, 0.8, 1.0, 1.1], speed_fac=[1.0, 1.0, 1.0, 1.25, 1 / 1.1, 1.0], amp=[1.0, 0.8, 1.0, 1.0, 1.1, 0.9],
                noise_lane=[-1, -1, -1, 5, 5], p=[0.0, 0.0, 0.0, 0.3, 0.45])
    m = SpeechCommandsAugment(bg, n_mels=n_mels, pad_mode=pad_mode, out_length=L).to(dev)
    out = m(torch.from_numpy(x).to(dev), [L] * 5, draws=d).cpu().numpy()
    assert out.shape == (5, n_mels, 8) and not out[:3].any()
    ref = R.pipeline(x, bg, d, n_mels=n_mels, pad_mode=pad_mode, L_out=L)["mel"]
    f32 = R.pipeline(x, bg, d, n_mels=n_mels, pad_mode=pad_mode, L_out=L, dtype=np.float32)["mel"]
    assert not ref[:3].any()
    e32, egpu = float(np.abs(f32 - ref).max()), float(np.abs(out - ref).max())
    print(f"SpeechCommandsAugment L=4000 {pad_mode} n_mels={n_mels}: {egpu:.2e} dB (float32 restatement {e32:.2e} dB)")
    assert egpu <= R.MARGIN * e32


def test_refusals(dev):
    lib, st = N.lib(), N.stream()
    x, out = nan_like((2, 1024), dev), nan_like((2, 3, R.NBIN, 2), dev)
    assert lib.ap_stft(N.ptr(x), N.ptr(out), 1, 2, 1024, st) == -22 and b"reflect" in lib.ap_last_error()
    assert lib.ap_stft(N.ptr(x), N.ptr(out), 2, 2, 1024, st) == -22
    assert lib.ap_stft(None, N.ptr(out), 0, 2, 1024, st) == -22
    t = _i32([0, 0], dev)
    r = torch.ones(2, dtype=torch.float64, device=dev)
    assert lib.ap_phase_vocoder_shift(N.ptr(out), N.ptr(out), r.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 3, st) == -22
    mel = nan_like((2, 129, 3), dev)
    assert lib.ap_mel_from_stft(N.ptr(out), t.data_ptr(), N.ptr(x), N.ptr(mel), 129, 2, 2, 3, st) == -22
    assert lib.ap_mel_from_stft(N.ptr(out), t.data_ptr(), N.ptr(x), N.ptr(mel), 32, 3, 2, 3, st) == -22
    assert lib.ap_aug_wave(N.ptr(x), t.data_ptr(), N.ptr(x), r.data_ptr(), t.data_ptr(), t.data_ptr(), N.ptr(x), 2, 1024, 1024, st) == -22
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(mel).all()) and bool(torch.isnan(x).all())
    m = SpeechCommandsAugment(R.background(1)).to(dev)
    with pytest.raises(N.NativeError):
        m(torch.zeros(1, 16000), [16000])
    with pytest.raises(ValueError, match="length"):
        m(torch.zeros(1, 16000, device=dev), [16001])
