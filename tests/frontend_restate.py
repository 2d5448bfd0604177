"""float64 restatements, in plain torch, of the operators behind three groups of product kernels: the M5 classifier
(ap_frontend.hip; M5Net.py:20-38 as SURVEY.md records it), the Slaney mel-dB front-end (ap_mel.hip; SURVEY.md Appendix A.4,
DESIGN.md) and two UNet primitives (GroupNorm32 + scale-shift + activation, QKVAttention; ap_convnet.hip, ap_unet_bwd.hip).
Every function works in the dtype of its input and is differentiable, so autograd of the float64 call is the reference
gradient and the float32 call measures what float32 arithmetic alone costs.  Test infrastructure only:
test_frontend_restate_cpu.py pins these to the golden-pinned fp32 oracle and checks the conditions the GPU tests rely on;
the GPU tests pin the kernels to these.  The input builders live here too, so both sides see the same numbers."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from audiopure_amd import synth

# ---- M5 ------------------------------------------------------------------------------------------------------------------
M5_TAU = 7e-6            # 4 x the 1.7e-6 float32 error of the pre-pool activations on these inputs (measured on the CPU)
# forward cases (L, n_channel, n_output); the LDS figures are launch_m5's: activations + the staged clip
M5_FWD_CASES = [(L, 32, no) for no in (10, 35) for L in (6848, 8000, 16000, 16016, 16037, 32000, 48000)] + [(16000, 64, 64), (16400, 64, 64)]
M5_GRAD_CASES = [(6848, 32), (8000, 32), (16000, 32), (16037, 32), (32000, 32), (8000, 64), (16000, 64)]      # (L, n_channel)
M5_MIN_DECIDED = 4       # of 8 clips, in every gradient case


def m5_weights(n_output, n_channel):
    return synth.m5_state_dict(n_output, n_channel=n_channel)


def m5_clips(B, L):
    return torch.from_numpy(synth.waveforms(B, L, seed=4))


def m5_cotangent(B, n_output):
    return torch.from_numpy(synth.uniform("m5v", (B, n_output), 1, -1.0, 1.0))


def m5_dims(L, k1=80, stride=16):
    """(P1, Q1, Q2, Q3, Q4): conv-1 positions and the pooled lengths of the four stages (floor pooling)."""
    P1 = (L - k1) // stride + 1
    Q1 = P1 // 4
    Q2 = (Q1 - 2) // 4
    Q3 = (Q2 - 2) // 4
    Q4 = (Q3 - 2) // 4
    return P1, Q1, Q2, Q3, Q4


def m5_forward(sd, x, stride=16, eps=1e-5):
    """x [B,1,L] -> (log-probabilities [B,n_output], [pre1..pre4]): four times conv -> BatchNorm(eval) -> ReLU ->
    MaxPool(4), then the mean over time, the linear layer and log_softmax.  pre_i is the BatchNorm output of stage i, the
    value the ReLU and the pooling select on."""
    t = {k: torch.as_tensor(np.asarray(v)).to(x.dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    h, pres = x, []
    for i, s in ((1, stride), (2, 1), (3, 1), (4, 1)):
        h = F.conv1d(h, t[f"conv{i}.weight"], t[f"conv{i}.bias"], stride=s)
        scale = t[f"bn{i}.weight"] / torch.sqrt(t[f"bn{i}.running_var"] + eps)
        h = (h - t[f"bn{i}.running_mean"][None, :, None]) * scale[None, :, None] + t[f"bn{i}.bias"][None, :, None]
        pres.append(h)
        h = F.max_pool1d(torch.relu(h), 4)
    h = h.mean(dim=-1)
    return F.log_softmax(h @ t["fc1.weight"].T + t["fc1.bias"], dim=1), pres


def m5_decided(pre, tau):
    """bool [B]: clip b is decided if, in every pooling window of every stage whose maximum is positive, the maximum and
    its gap to the runner-up both exceed tau -- a float32 evaluation whose pre-pool error is below tau / 2 then selects the
    same elements, so its gradient differs from the reference by rounding alone.  A window whose maximum is within tau
    below zero is undecided as well (float32 may open it)."""
    ok = torch.ones(pre[0].shape[0], dtype=torch.bool)
    for p in pre:
        B, C, P = p.shape
        w = p.detach()[:, :, :(P // 4) * 4].reshape(B, C, P // 4, 4)
        top = w.topk(2, dim=-1).values
        mx, gap = top[..., 0], top[..., 0] - top[..., 1]
        bad = ((mx > 0) & ((mx <= tau) | (gap <= tau))) | ((mx <= 0) & (mx >= -tau))
        ok &= ~bad.reshape(B, -1).any(dim=1)
    return ok


def m5_gradient_errors(got, ref):
    """per clip: (max |got - ref| / max |ref|, median |got - ref| / max |ref|), float64 [B,1,L] tensors"""
    d, top = (got - ref).abs().reshape(got.shape[0], -1), ref.abs().reshape(ref.shape[0], -1).amax(dim=1)
    return (d.amax(dim=1) / top).tolist(), (d.median(dim=1).values / top).tolist()


def assert_m5_gradient(got, ref, decided, decided_bound):
    """A decided clip must agree with the float64 gradient to decided_bound of its largest entry: nothing but rounding
    separates the two.  An undecided clip may differ where a selection flipped: 1e-3 of its largest entry at isolated
    samples, 2e-6 in the median.  (NaN fails either.)"""
    mx, med = m5_gradient_errors(got, ref)
    for b in range(got.shape[0]):
        if bool(decided[b]):
            assert mx[b] <= decided_bound, (b, mx[b])
        else:
            assert mx[b] < 1e-3 and med[b] < 2e-6, (b, mx[b], med[b])


# ---- Slaney mel-dB ----------------------------------------------------------------------------------------------------------
NFFT, HOP = 2048, 512
MEL_FWD_L = (1, 511, 512, 513, 1023, 1024, 2047, 2048, 2049, 5000, 16000, 16384)
MEL_FWD_MELS = (32, 40, 64, 128)
MEL_GRAD_L = (1, 513, 2049, 5000, 16384)
MEL_GRAD_MELS = (32, 128)


def _hz_to_mel(f):
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    return min_log_hz / f_sp + math.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp


def _mel_to_hz(m):
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return torch.where(m >= min_log_mel, min_log_hz * torch.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(n_mels, sample_rate=16000, n_fft=NFFT):
    """float64 [n_fft/2+1, n_mels]: triangles between n_mels + 2 corners equally spaced on the Slaney mel scale from 0 to
    sample_rate / 2, each scaled by 2 / (its width in Hz) (Slaney area normalisation)."""
    freqs = torch.linspace(0, sample_rate / 2, n_fft // 2 + 1, dtype=torch.float64)
    pts = _mel_to_hz(torch.linspace(_hz_to_mel(0.0), _hz_to_mel(sample_rate / 2), n_mels + 2, dtype=torch.float64))
    lo, mid, hi = pts[:-2], pts[1:-1], pts[2:]
    up = (freqs[:, None] - lo[None]) / (mid - lo)[None]
    down = (hi[None] - freqs[:, None]) / (hi - mid)[None]
    return torch.clamp(torch.minimum(up, down), min=0.0) * (2.0 / (hi - lo))[None]


def mel_power(x, n_mels):
    """[B,1,L] -> mel power [B,n_mels,1+L//512]: zero-padded centred frames, periodic Hann 2048, |rFFT|^2, filterbank."""
    B, L = x.shape[0], x.shape[-1]
    w = F.pad(x.reshape(B, L), (NFFT // 2, NFFT // 2))
    frames = w.unfold(1, NFFT, HOP)                                           # [B, 1 + L // 512, 2048]
    n = torch.arange(NFFT, dtype=torch.float64)
    win = (0.5 - 0.5 * torch.cos(2 * math.pi * n / NFFT)).to(x.dtype)
    spec = torch.fft.rfft(frames * win, dim=-1)
    power = spec.real ** 2 + spec.imag ** 2
    return (power @ mel_filterbank(n_mels).to(x.dtype)).transpose(1, 2)


def mel_db(x, n_mels, mode=0):
    """[B,1,L] -> [B,1,n_mels,frames].  mode 0: 10 log10(max(mel, 1e-10)).  mode 1: that minus its maximum over the
    clip, floored at -80 (librosa power_to_db(ref=np.max, top_db=80) on the mode-0 values)."""
    db = 10.0 * torch.log10(torch.clamp(mel_power(x, n_mels), min=1e-10))
    if mode == 1:
        db = torch.clamp(db - db.reshape(db.shape[0], -1).max(dim=1).values[:, None, None], min=-80.0)
    return db.unsqueeze(1)


def mel_noise(B, L):
    return torch.from_numpy(synth.waveforms(B, L, seed=5))


def mel_stretch_clips(gains_per_clip, L=16384):
    """Clips made of equal stretches of synth.waveforms noise, each times its gain (0.0: exact zeros).  The stretch length
    is a multiple of 512, so a frame overlaps a stretch by at least 512 samples or not at all."""
    x = torch.from_numpy(synth.waveforms(len(gains_per_clip), L, seed=6)).clone()
    for b, gains in enumerate(gains_per_clip):
        n = L // len(gains)
        assert n % 512 == 0 and n * len(gains) == L
        for i, g in enumerate(gains):
            x[b, 0, i * n:(i + 1) * n] *= g
    return x


LOUD, QUIET, VERY_QUIET, ZERO = 1.0, 1e-3, 3e-5, 0.0
# forward: very quiet is below the -80 dB floor of mode 1 and above the 1e-10 clamp
MEL_FWD_STRETCHES = [(LOUD, QUIET, VERY_QUIET, ZERO), (ZERO, VERY_QUIET, LOUD, QUIET), (QUIET, ZERO, VERY_QUIET, LOUD)]
# gradient: nothing between the clamp and well above it (the clamp's derivative jumps at 1e-10)
MEL_GRAD_STRETCHES = [(LOUD, QUIET, ZERO, ZERO), (ZERO, QUIET, LOUD, ZERO)]


def mel_cotangent(tag, B, n_mels, L):
    return torch.from_numpy(synth.uniform(f"melv{tag}", (B, 1, n_mels, 1 + L // HOP), 1, -1.0, 1.0))


def mel_clamp_is_far(mel):
    """No mel power in (1e-12, 1e-8): every element is either far above the 1e-10 clamp or (zeros) far below it."""
    return not bool(((mel > 1e-12) & (mel < 1e-8)).any())


def mel_silent_samples(mel, L):
    """bool [B,L]: samples all of whose covering frames (f with 512 f - 1024 <= t < 512 f + 1024) have no mel power."""
    silent = (mel < 1e-12).all(dim=1)                                         # [B, frames]
    t = torch.arange(L)
    out = torch.ones(mel.shape[0], L, dtype=torch.bool)
    for f in range(mel.shape[2]):
        cover = (t >= HOP * f - NFFT // 2) & (t < HOP * f + NFFT // 2)
        out &= ~cover[None] | silent[:, f:f + 1]
    return out


def local_scale(ref, radius=2048):
    """max |ref| over the +-radius samples around each sample, [B,1,L] -> [B,1,L]"""
    return F.max_pool1d(ref.abs(), 2 * radius + 1, stride=1, padding=radius)


# ---- UNet primitives --------------------------------------------------------------------------------------------------------
GN_TAU = 1e-5
GN_MAX_SKIPPED = 0.02
# (B, C, H, W, groups, act, scale_shift): n = 8 < 256 threads; act = 1; H W % 4 != 0; 12 288- and 24 576-float slabs (more
# than one trip of every `i += 256` loop); 2240 blocks
GN_BWD_CASES = [(3, 64, 2, 2, 32, 2, True), (2, 64, 5, 5, 32, 1, False), (2, 96, 8, 8, 32, 0, True), (1, 384, 32, 32, 32, 2, True),
                (1, 64, 64, 48, 8, 2, False), (70, 64, 4, 4, 32, 2, True), (2, 128, 16, 8, 32, 1, True)]


def gn_inputs(B, C, H, W):
    """x (offset by +0.7: a non-zero group mean), gamma, beta, scale-shift [B,2C], dy -- all float32"""
    x = torch.from_numpy(synth.uniform(f"gnx{C}{H}{W}", (B, C, H, W), 1, -2, 2)) + 0.7
    g, b = torch.from_numpy(synth.uniform("gng", (C,), 1, 0.5, 1.5)), torch.from_numpy(synth.uniform("gnb", (C,), 1))
    ss = torch.from_numpy(synth.uniform("gns", (B, 2 * C), 1))
    dy = torch.from_numpy(synth.uniform(f"gndy{C}{H}{W}", (B, C, H, W), 1))
    return x, g, b, ss, dy


def groupnorm_film_act(x, gamma, beta, ss, groups, act, eps=1e-5):
    """(y, y1): y1 = (gamma xh + beta) (1 + scale) + shift with xh the group-normalised x (biased variance) and
    (scale, shift) the halves of ss [B,2C] (None: neither); y = y1 (act 0), relu(y1) (act 1) or y1 sigmoid(y1) (act 2)."""
    B, C = x.shape[:2]
    xg = x.reshape(B, groups, -1)
    mean = xg.mean(dim=2, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=2, keepdim=True)
    xh = ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape)
    y1 = xh * gamma[None, :, None, None] + beta[None, :, None, None]
    if ss is not None:
        y1 = y1 * (1 + ss[:, :C, None, None]) + ss[:, C:, None, None]
    y = y1 if act == 0 else torch.relu(y1) if act == 1 else y1 * torch.sigmoid(y1)
    return y, y1


def groupnorm_decided(y1, groups, tau):
    """bool [B,groups]: the (sample, group) slab has no pre-activation within tau of the ReLU's kink.  One element on the
    other side changes mean(dxh) and mean(dxh xh) and with them the gradient of the whole slab, so the unit is the slab."""
    B = y1.shape[0]
    return (y1.detach().abs().reshape(B, groups, -1) > tau).all(dim=2)


# (channels per head, T, heads, peaked).  scalar path (T % 4 != 0) at one and two trips of the `t += 256` loop; the 16-byte
# path past 256; ch = 64 off the MFMA shapes; 153 600 B of LDS, 240 B under the limit; the MFMA shapes; peaked rows (qkv x 4)
ATT_CASES = [(8, 17, 2, False), (32, 301, 1, False), (16, 1024, 1, False), (32, 300, 2, False), (64, 128, 2, False),
             (64, 300, 1, False), (64, 64, 4, False), (64, 256, 3, False), (64, 128, 2, True), (32, 100, 1, True), (64, 256, 3, True)]
ATT_B = 2


def att_inputs(ch, T, heads, peaked):
    qkv = torch.from_numpy(synth.uniform(f"qkv{ch}", (ATT_B, heads * 3 * ch, T), 1, -1.5, 1.5))
    do = torch.from_numpy(synth.uniform(f"do{ch}", (ATT_B, heads * ch, T), 1))
    return (qkv * 4.0 if peaked else qkv), do


def qkv_attention(qkv, heads):
    """qkv [B, heads 3 ch, T] laid out [B][heads][q|k|v][ch][T] -> [B, heads ch, T]:
    out[:, t] = sum_s softmax_s(q_t . k_s / sqrt(ch)) v_s  per (sample, head)."""
    B, C3, T = qkv.shape
    ch = C3 // (3 * heads)
    q, k, v = torch.split(qkv.reshape(B * heads, 3 * ch, T), ch, dim=1)
    w = torch.softmax(torch.einsum("bct,bcs->bts", q, k) / math.sqrt(ch), dim=-1)
    return torch.einsum("bts,bcs->bct", w, v).reshape(B, heads * ch, T)


# ---- small elementwise kernels ----------------------------------------------------------------------------------------------
SMALL_N = (1, 255, 257, 100003)
# p_sample coefficients of a mid-schedule step: r1 = sqrt(1/acp), r2 = sqrt(1/acp - 1), posterior mean coefficients, sigma
PSAMPLE_COEF = dict(r1=1.25, r2=0.75, c1=0.3125, c2=0.6875, sigma=0.21)


def small_inputs(n):
    """x, eps, z: float32 [n].  r1 x - r2 eps spans about [-1.6, 1.6]: the clamp to [-1, 1] is active at both ends."""
    return (synth.uniform("smx", (n,), 1, -1.0, 1.0), synth.uniform("sme", (n,), 1, -1.0, 1.0), synth.normal("smz", (n,), 1))


def _fl(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def _fma_forms(a, x, b, y):
    """float32 values of a x + b y under every contraction C++ allows: both products rounded, or either one fused into
    the addition (the exact float64 product plus the rounded other product, rounded once more: a fused multiply-add up to
    the double rounding, which 2 ulp absorbs)."""
    a, b = np.float32(a), np.float32(b)
    ax, by = (a * x).astype(np.float32), (b * y).astype(np.float32)
    ax64, by64 = np.float64(a) * x.astype(np.float64), np.float64(b) * y.astype(np.float64)
    return [(ax + by).astype(np.float32), _fl(ax64 + by.astype(np.float64)), _fl(ax.astype(np.float64) + by64)]


def psample_forms(x, eps, z, r1, r2, c1, c2, sigma, clip):
    """Every float32 value `c1 clamp(r1 x - r2 eps) + c2 x [+ sigma z]` can take in the kernel's operation order."""
    outs = []
    for p in _fma_forms(r1, x, -np.float32(r2), eps):
        if clip:
            p = np.minimum(np.maximum(p, np.float32(-1.0)), np.float32(1.0))
        for v in _fma_forms(c1, p, c2, x):
            if z is None:
                outs.append(v)
            else:
                sz = np.float32(sigma) * z
                outs += [(v + sz).astype(np.float32), _fl(v.astype(np.float64) + np.float64(np.float32(sigma)) * z.astype(np.float64))]
    return outs


def axpbyc_forms(x, y, a, b, c):
    """Every float32 value `a x + b y + c` (y None: `a x + c`) can take."""
    c = np.float32(c)
    if y is None:
        ax = (np.float32(a) * x).astype(np.float32)
        return [(ax + c).astype(np.float32), _fl(np.float64(np.float32(a)) * x.astype(np.float64) + np.float64(c))]
    return [(s + c).astype(np.float32) for s in _fma_forms(a, x, b, y)]


def ulp_distance_to_nearest(got, forms):
    """per element: min over the forms of |got - form| in units of the form's float32 ulp"""
    got = np.asarray(got, dtype=np.float32)
    best = np.full(got.shape, np.inf)
    for f in forms:
        ulp = np.spacing(np.abs(f)).astype(np.float64)
        best = np.minimum(best, np.abs(got.astype(np.float64) - f.astype(np.float64)) / ulp)
    return best


TEMB_T = (0.0, 0.5, 37.0, 999.0)


def temb_inputs(n, dim):
    """t [n] cycling through TEMB_T and the model's float32 frequencies exp(-ln(10000) j / half)"""
    t = np.asarray([TEMB_T[i % len(TEMB_T)] for i in range(n)], dtype=np.float32)
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half).numpy()
    return t, freqs


def temb_reference(t, freqs):
    """float64 [cos | sin] of the float32 products t f (the kernel's argument)"""
    a = (t[:, None] * freqs[None, :]).astype(np.float32)
    return np.concatenate([np.cos(a.astype(np.float64)), np.sin(a.astype(np.float64))], axis=1), a
