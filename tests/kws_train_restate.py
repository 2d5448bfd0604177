"""Case table and float64 references for the KWS classifier's training step (ap_kws_train_bwd, KWSModel in train()).  The
reference is oracle.kws_oracle.kws_forward differentiated by autograd with respect to the state dict and the input, in the
input's dtype; inputs, weights and cotangents are those of kws_restate.py.  kws_backward_by_hand is the same backward written
out the way a kernel forms it, with one switch: each name in TRAIN_MUTATIONS is a mistake a hand-written parameter-gradient
contraction could make.  Test infrastructure only: test_kws_train_cpu.py checks all of it, test_gpu_kws_train.py pins the
kernels to it."""
import functools
import os

import torch
import torch.nn.functional as F

import kws_restate as R
from oracle import kws_oracle as K

GOLDEN_TRAIN = os.path.join(R.ROOT, "tests", "golden", "golden_kws_train_v1.npz")

TRAIN_T = (5, 19, 20, 21, 37, 81)                              # T2 = 1, 1, 1, 2, 3, 5: a second GRU step appears at 20 -> 21
# (n_mels, hidden, num_classes, T, B)
TRAIN_CASES = ([R.GOLDEN_SHAPE + (T, 8) for T in TRAIN_T]
               + [s + (T, 8) for s in R.KWS_SHAPES[1:] for T in (5, 21, 81)]
               + [R.GOLDEN_SHAPE + (81, 1),
                  R.GOLDEN_SHAPE + (81, 67),                   # 335 items: no multiple of the kernels' 16 slices
                  R.GOLDEN_SHAPE + (81, 300),                  # more clips than compute units
                  (32, 64, 4, 161, 8)])                        # the training script's N_MELS = 32, a 1.6 s clip
TRAIN_BWD_ONLY_CASES = [R.GOLDEN_SHAPE + (1001, 2)]            # past the forward's LDS limit, T2 = 63
SLICES = 16                                                    # KWS_SLICES of ap_kws.hip

# float32 CPU evaluation of the autograd reference against float64 over TRAIN_CASES + TRAIN_BWD_ONLY_CASES: the largest
# per-tensor max |g32 - g64| / max |g64| of a parameter gradient (measured 1.09e-5, Wx_b.bias at (20, 128, 64) T = 21; 9e-7 to
# 5.9e-6 elsewhere, Wx_b.bias the worst tensor wherever T2 > 1)
TRAIN_F32_GRAD_ERR = 1.1e-5
TRAIN_GRAD_BOUND = R.GPU_FACTOR * TRAIN_F32_GRAD_ERR

TRAIN_MUTATIONS = ("hidden_n_not_scaled_by_r", "weight_hh_with_h_t", "reverse_pairs_mirrored_input", "l1_weight_ih_forward_half")
TRAIN_MUTATION_MIN_T2 = {"hidden_n_not_scaled_by_r": 1, "weight_hh_with_h_t": 2, "reverse_pairs_mirrored_input": 2,
                         "l1_weight_ih_forward_half": 1}

# three Adam steps (train.py:80: default lr 1e-3, weight_decay 1e-5) on CrossEntropyLoss of the log-probabilities (train.py:79,
# 148-149).  Adam's first update is lr g / (|g| + 1e-8): where a gradient entry is within float32 noise of zero its sign, hence
# the whole update, is undetermined, so the comparison looks at the entries whose float64 gradient stays at or above ADAM_MASK
# of its tensor's largest entry in all three steps.  There a relative gradient error r moves an update by about r lr.
ADAM_CASE = R.GOLDEN_SHAPE + (81, 8)
ADAM_STEPS, ADAM_LR, ADAM_WD, ADAM_MASK = 3, 1e-3, 1e-5, 1e-3
# float32 CPU run against the float64 run: the largest |p32 - p64| / lr over the compared entries (measured 1.25e-4; 116 224 of
# the 143 152 entries are compared, and the steps move a parameter by up to 3.0 lr)
ADAM_F32_ERR = 1.3e-4
ADAM_BOUND = R.GPU_FACTOR * ADAM_F32_ERR


def exact_zero(name, Kc, T):
    """Is the gradient of tensor `name` exactly zero by construction?  One class: log-softmax is identically 0.  One GRU step:
    h_prev is 0 (weight_hh) and a softmax over one step is identically 1 (the attention's own parameters)."""
    if Kc == 1:
        return True
    if R.kws_dims(T)[1] == 1:
        return ".weight_hh_" in name or name.startswith("attn_layer.")
    return False


def train_targets(B, Kc):
    return torch.arange(B) * 7 % Kc


def golden_input(n_mels, T, B):
    """the mel-dB input of tests/golden/make_golden_kws_train.py"""
    from audiopure_amd import synth
    return torch.from_numpy(synth.uniform(f"kwstrain/{n_mels}/{T}", (B, 1, n_mels, T), 1, -80.0, 20.0))


def _as_dtype(sd, dtype):
    return {k: v.to(dtype).clone() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def train_reference(case, dtype=torch.float64):
    """(log-probabilities [B,K], d mel [B,n_mels,T], {name: gradient}) of kws_forward by autograd, evaluated in dtype"""
    n_mels, H, Kc, T, B = case
    sd = {k: v.requires_grad_(True) for k, v in _as_dtype(R.kws_weights(n_mels, H, Kc), dtype).items()}
    x = R.kws_mel(n_mels, T, B).to(dtype).requires_grad_(True)
    lp = K.kws_forward(sd, x, hidden=H)
    gs = torch.autograd.grad(lp, [x] + list(sd.values()), R.kws_cotangent(n_mels, T, B, Kc).to(dtype))
    return lp.detach(), gs[0][:, 0], dict(zip(sd, gs[1:]))


def tensor_rel_err(got, ref):
    """max |got - ref| / max |ref| of one tensor (the absolute error where the reference is identically 0)"""
    d, top = float((got.double() - ref.double()).abs().max()), float(ref.abs().max())
    return d / top if top > 0 else d


def kws_backward_by_hand(sd, x, v, hidden=64, mutate=None):
    """float64 forward with saves and the backward a kernel would run: (log-probabilities, d mel, {name: gradient}).
    mutate=None agrees with autograd to rounding (checked on the CPU)."""
    assert mutate is None or mutate in TRAIN_MUTATIONS
    t = {k: v_.to(x.dtype) for k, v_ in sd.items()}
    x = x.squeeze(1) if x.ndim == 4 else x
    B, n_in, T = x.shape
    H, groups = hidden, int(n_in / 20)
    cpg, opg = n_in // groups, H // groups
    w0, w1 = t["CRNN_model.sepconv.0.weight"], t["CRNN_model.sepconv.1.weight"]
    dwv = F.conv1d(x, w0, t["CRNN_model.sepconv.0.bias"], stride=2, groups=n_in)           # [B,n,T1]
    pw = F.conv1d(dwv, w1, t["CRNN_model.sepconv.1.bias"], stride=8, groups=groups)         # [B,H,T2]
    T1, T2 = dwv.shape[2], pw.shape[2]
    seqs, saves = [pw.permute(2, 0, 1)], []
    for layer in (0, 1):
        inp, outs, sv = seqs[-1], [], []
        for d, suffix in enumerate(("", "_reverse")):
            wi, wh = t[f"CRNN_model.gru.weight_ih_l{layer}{suffix}"], t[f"CRNN_model.gru.weight_hh_l{layer}{suffix}"]
            bi, bh = t[f"CRNN_model.gru.bias_ih_l{layer}{suffix}"], t[f"CRNN_model.gru.bias_hh_l{layer}{suffix}"]
            hs, out, st = torch.zeros(B, H, dtype=x.dtype), [None] * T2, [None] * T2
            for s in (range(T2) if d == 0 else range(T2 - 1, -1, -1)):
                gi, gh = inp[s] @ wi.t() + bi, hs @ wh.t() + bh
                r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
                n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
                hn = (1 - z) * n + z * hs
                st[s] = (r, z, n, gh[:, 2 * H:], hs, hn)
                hs = out[s] = hn
            outs.append(torch.stack(out))
            sv.append(st)
        seqs.append(torch.cat(outs, dim=2))
        saves.append(sv)
    out = seqs[2]                                                                           # [T2,B,2H]
    Wx, bx, vt, U = t["attn_layer.Wx_b.weight"], t["attn_layer.Wx_b.bias"], t["attn_layer.Vt.weight"], t["apply_attn.U.weight"]
    th = torch.tanh(out @ Wx.t() + bx)
    a = torch.softmax((th @ vt.t()).squeeze(2), dim=0)                                      # [T2,B]
    c = (a[:, :, None] * out).sum(0)
    logit = c @ U.t()
    lp = F.log_softmax(logit, dim=-1)
    # ---- backward ----
    g = {}
    dlogit = v - torch.softmax(logit, dim=-1) * v.sum(-1, keepdim=True)
    g["apply_attn.U.weight"] = dlogit.t() @ c
    dc = dlogit @ U
    da = (dc[None] * out).sum(2)
    de = a * (da - (a * da).sum(0, keepdim=True))
    dpre = de[:, :, None] * vt * (1 - th * th)
    g["attn_layer.Vt.weight"] = (de[:, :, None] * th).sum((0, 1))[None]
    g["attn_layer.Wx_b.weight"] = torch.einsum("tbi,tbk->ik", dpre, out)
    g["attn_layer.Wx_b.bias"] = dpre.sum((0, 1))
    dout = a[:, :, None] * dc[None] + dpre @ Wx
    for layer in (1, 0):
        inp = seqs[layer]
        din = torch.zeros_like(inp)
        for d, suffix in enumerate(("", "_reverse")):
            wi, wh = t[f"CRNN_model.gru.weight_ih_l{layer}{suffix}"], t[f"CRNN_model.gru.weight_hh_l{layer}{suffix}"]
            dwi, dwh = torch.zeros_like(wi), torch.zeros_like(wh)
            dbi, dbh = torch.zeros(3 * H, dtype=x.dtype), torch.zeros(3 * H, dtype=x.dtype)
            dh = torch.zeros(B, H, dtype=x.dtype)
            for s in (range(T2 - 1, -1, -1) if d == 0 else range(T2)):
                r, z, n, ghn, hp, hn = saves[layer][d][s]
                dht = dh + dout[s][:, d * H:(d + 1) * H]
                dn = dht * (1 - z) * (1 - n * n)
                dr = dn * ghn * r * (1 - r)
                dz = dht * (hp - n) * z * (1 - z)
                dgi, dgh = torch.cat([dr, dz, dn], 1), torch.cat([dr, dz, dn * r], 1)
                dh = dht * z + dgh @ wh
                din[s] += dgi @ wi
                # what the parameter contractions pair up
                pgh = torch.cat([dr, dz, dn], 1) if mutate == "hidden_n_not_scaled_by_r" else dgh
                pin = inp[T2 - 1 - s] if (mutate == "reverse_pairs_mirrored_input" and d == 1) else inp[s]
                if mutate == "l1_weight_ih_forward_half" and layer == 1:
                    pin = torch.cat([pin[:, :H], torch.zeros_like(pin[:, H:])], 1)
                dwi += dgi.t() @ pin
                dwh += pgh.t() @ (hn if mutate == "weight_hh_with_h_t" else hp)
                dbi += dgi.sum(0)
                dbh += pgh.sum(0)
            g[f"CRNN_model.gru.weight_ih_l{layer}{suffix}"], g[f"CRNN_model.gru.weight_hh_l{layer}{suffix}"] = dwi, dwh
            g[f"CRNN_model.gru.bias_ih_l{layer}{suffix}"], g[f"CRNN_model.gru.bias_hh_l{layer}{suffix}"] = dbi, dbh
        dout = din
    dpw = dout.permute(1, 2, 0)                                                             # [B,H,T2]
    dws = dwv[:, :, ::8][:, :, :T2]                                                         # the frames the pointwise conv reads
    g["CRNN_model.sepconv.1.bias"] = dpw.sum((0, 2))
    g["CRNN_model.sepconv.1.weight"] = torch.einsum("bgot,bgct->goc", dpw.reshape(B, groups, opg, T2),
                                                    dws.reshape(B, groups, cpg, T2)).reshape(H, cpg, 1)
    ddw = torch.zeros_like(dwv)
    ddw[:, :, 0:8 * T2:8] = torch.einsum("bgot,goc->bgct", dpw.reshape(B, groups, opg, T2),
                                         w1.reshape(groups, opg, cpg)).reshape(B, n_in, T2)
    g["CRNN_model.sepconv.0.bias"] = ddw.sum((0, 2))
    g["CRNN_model.sepconv.0.weight"] = torch.einsum("bct,bctk->ck", ddw, x.unfold(2, 5, 2))[:, None, :]
    dx = torch.zeros_like(x)
    for k in range(5):
        dx[:, :, k:k + 2 * T1 - 1:2] += ddw * w0[:, 0, k][None, :, None]
    return lp, dx, {k: g[k] for k in sd}


def by_hand(case, mutate=None):
    n_mels, H, Kc, T, B = case
    return kws_backward_by_hand(_as_dtype(R.kws_weights(n_mels, H, Kc), torch.float64), R.kws_mel(n_mels, T, B).double(),
                                R.kws_cotangent(n_mels, T, B, Kc).double(), hidden=H, mutate=mutate)


def adam_run(dtype):
    """Three Adam steps on ADAM_CASE by autograd of the oracle in dtype.  Returns (parameters after the steps {name: tensor},
    per-step gradients [{name: tensor}])."""
    n_mels, H, Kc, T, B = ADAM_CASE
    sd = {k: v.requires_grad_(True) for k, v in _as_dtype(R.kws_weights(n_mels, H, Kc), dtype).items()}
    x, y = R.kws_mel(n_mels, T, B).to(dtype), train_targets(B, Kc)
    opt = torch.optim.Adam(list(sd.values()), lr=ADAM_LR, weight_decay=ADAM_WD)
    grads = []
    for _ in range(ADAM_STEPS):
        opt.zero_grad()
        torch.nn.CrossEntropyLoss()(K.kws_forward(sd, x, hidden=H), y).backward()
        grads.append({k: v.grad.detach().clone() for k, v in sd.items()})
        opt.step()
    return {k: v.detach().clone() for k, v in sd.items()}, grads


@functools.lru_cache(maxsize=None)
def adam_reference():
    """(float64 parameters after the steps, {name: bool mask of the compared entries})"""
    p64, grads = adam_run(torch.float64)
    mask = {k: torch.stack([g[k].abs() >= ADAM_MASK * g[k].abs().max() for g in grads]).all(0) for k in p64}
    return p64, mask


def adam_err(params, p64, mask):
    """largest |p - p64| / lr over the compared entries"""
    return max(float((params[k].double().cpu() - p64[k]).abs()[mask[k]].max()) / ADAM_LR for k in p64 if bool(mask[k].any()))
