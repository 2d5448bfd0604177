"""float64 restatement, in plain torch, of M5 in train mode (M5Net.py:21-38 with nn.BatchNorm1d in training mode, as
audio_models/M5/train.py:86-103 runs it): four times conv -> BatchNorm with batch statistics -> ReLU -> MaxPool(4), the mean over
time, fc1, log_softmax; the running statistics as torch updates them; gradients by torch autograd.  Every function works in the
dtype it is given, so the float64 call is the reference and the float32 call measures what float32 arithmetic alone costs.
Test infrastructure only: test_m5_train_cpu.py pins it to the reference's own numbers (tests/golden/golden_m5_train_v1.npz)
and asserts the conditions on the case table; test_gpu_m5_train.py pins the kernels of ap_m5_train.hip to it.

    python tests/m5_train_restate.py        # re-measure the float32 errors and search the clip seeds (CPU, about a minute)
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import frontend_restate as FR
from audiopure_amd import synth

PARAMS = [f"{m}{i}.{w}" for i in (1, 2, 3, 4) for m, w in (("conv", "weight"), ("conv", "bias"), ("bn", "weight"), ("bn", "bias"))] + \
    ["fc1.weight", "fc1.bias"]                       # the order of the gradient blob (ap_m5_param_elems)
MOMENTUM, EPS, STRIDE = 0.1, 1e-5, 16

# (B, L, n_channel, n_output): each the smallest size at which something branches
#   (1, 6848)  the minimum length: Q4 = 1, four values per channel in stage 4 (the n / (n - 1) factor, the cancellation in var)
#   (2, 6848)  the same with two clips
#   (5, 8000)  odd batch; 2, 0 and 1 pre-pool positions beyond 4 Q in stages 2, 3, 4 (P = 122, 28, 5)
#   (3, 16037) L no multiple of 4 or of the stride
#   (8, 16000) the workload's length: 3, 3, 0 such positions
#   (4, 8000, 64, 64) the wide net
SHAPES = [(1, 6848, 32, 10), (2, 6848, 32, 10), (5, 8000, 32, 35), (3, 16037, 32, 10), (8, 16000, 32, 10), (4, 8000, 64, 64)]
# per shape: the float32-torch error of the pre-pool activations (BatchNorm outputs) against float64, max over the four stages,
# measured on the CPU at the default seed by this file's __main__; tau = 4 x it (the factor of frontend_restate.M5_TAU); and the
# clip seed, the first of 0..255 at which EVERY clip of the batch is decided at tau (None: no seed qualifies -> loose bounds)
PREPOOL_F32_ERR = {SHAPES[0]: 1.0e-5, SHAPES[1]: 6.6e-6, SHAPES[2]: 4.8e-6, SHAPES[3]: 3.8e-6, SHAPES[4]: 3.6e-6, SHAPES[5]: 4.1e-6}
CLIP_SEED = {SHAPES[0]: 1, SHAPES[1]: 0, SHAPES[2]: 0, SHAPES[3]: 0, SHAPES[4]: 5, SHAPES[5]: 3}
MAX_LOOSE = 2                                        # at most two of the six cases may be compared with the loose bounds
DEFAULT_SEED = 4

# the float32-torch evaluation against float64: per parameter max |d| / max |ref| (a conv bias, whose gradient is an exact zero,
# by max |ref dW| of its stage), and dx likewise -- the largest figure over the table, measured by test_m5_train_cpu.py /
# this file's __main__: 5.1e-6 (conv2.weight at B = 1, L = 6848, where stage 4 normalises four values per channel; 1.4e-6 to
# 2.0e-6 in the other five cases; dx 3.5e-7 to 3.4e-6).  The GPU bound is 4 x it.
GRAD_F32_ERR = 5.1e-6
GRAD_BOUND = 4 * GRAD_F32_ERR
# forward: frontend_restate's eval bound on the log-probabilities (2e-5 at a pre-pool error of 1.7e-6) scaled by the train-mode
# pre-pool error measured above, largest over the table
EVAL_FWD_BOUND, EVAL_PREPOOL_F32_ERR = 2e-5, 1.7e-6
FWD_BOUND = EVAL_FWD_BOUND * max(PREPOOL_F32_ERR.values()) / EVAL_PREPOOL_F32_ERR
# three Adam steps: the largest deviation of a step's float32-torch loss from the float64 one (test_m5_train_cpu.py: 5.7e-7, 1.4e-7
# and 4.9e-9 at the three steps).  A step's loss is a mean of log-probabilities, each within the forward bound of float64 at equal
# parameters, and the parameters have drifted by what the trajectory figure measures: the bound is the sum of the two.
TRAJ_F32_ERR = 5.7e-7
TRAJ_BOUND = FWD_BOUND + 4 * TRAJ_F32_ERR


def tau(shape):
    return 4 * PREPOOL_F32_ERR[shape]


def weights(n_output, n_channel):
    """synth.m5_state_dict with the sign of every fifth gamma flipped: a max taken before the affine is wrong there"""
    sd = {k: np.array(v, copy=True) for k, v in synth.m5_state_dict(n_output, n_channel=n_channel).items()}
    for i in (1, 2, 3, 4):
        sd[f"bn{i}.weight"][::5] *= -1.0
    return sd


def clips(B, L, seed):
    return torch.from_numpy(synth.waveforms(B, L, seed=seed))


def labels(B, n_output):
    return torch.arange(B) % n_output


def case_inputs(shape):
    B, L, nc, no = shape
    seed = CLIP_SEED[shape]
    return weights(no, nc), clips(B, L, DEFAULT_SEED if seed is None else seed), labels(B, no)


def tensors(sd, dtype, requires_grad=True):
    """state dict -> tensors of `dtype`; the 18 parameters are leaves that require grad"""
    t = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    if requires_grad:
        for k in PARAMS:
            t[k].requires_grad_(True)
    return t


def forward(t, x, momentum=MOMENTUM, max_then_affine=False, stage1_last_max=False):
    """x [B,1,L] -> dict: logp [B,n_output]; z, y (conv and BatchNorm outputs) and a (pooled) per stage; running: the new running
    statistics.  max_then_affine: the WRONG order a port of the eval kernel would take (max over the normalised value, then
    gamma and beta) -- equal for positive gamma, different for a negative one.  stage1_last_max: the WRONG tie rule in stage 1 (the
    last maximum of a window wins; P_1 must be a multiple of 4)."""
    h, zs, ys, acts, running = x, [], [], [], {}
    for i, s in ((1, STRIDE), (2, 1), (3, 1), (4, 1)):
        z = F.conv1d(h, t[f"conv{i}.weight"], t[f"conv{i}.bias"], stride=s)
        rm, rv = t[f"bn{i}.running_mean"].detach().clone(), t[f"bn{i}.running_var"].detach().clone()
        g, be = t[f"bn{i}.weight"], t[f"bn{i}.bias"]
        if max_then_affine:
            xh = F.batch_norm(z, None, None, None, None, training=True, eps=EPS)
            y = xh * g[None, :, None] + be[None, :, None]
            h = torch.relu(F.max_pool1d(xh, 4) * g[None, :, None] + be[None, :, None])
        else:
            y = F.batch_norm(z, rm, rv, g, be, training=True, momentum=momentum, eps=EPS)
            if stage1_last_max and i == 1:
                assert y.shape[-1] % 4 == 0
                h = F.max_pool1d(torch.relu(y).flip(-1), 4).flip(-1)
            else:
                h = F.max_pool1d(torch.relu(y), 4)
        running[f"bn{i}.running_mean"], running[f"bn{i}.running_var"] = rm, rv
        zs.append(z), ys.append(y), acts.append(h)
    feat = h.mean(dim=-1)
    return {"logp": F.log_softmax(feat @ t["fc1.weight"].T + t["fc1.bias"], dim=1), "z": zs, "y": ys, "a": acts, "running": running}


def loss_and_grads(sd, x, y, dtype=torch.float64, extra=(), **kw):
    """-> (out dict of forward, loss, {parameter or 'x': gradient}, [gradient of each tensor in extra(out)])"""
    t = tensors(sd, dtype)
    xr = x.to(dtype).clone().requires_grad_(True)
    out = forward(t, xr, **kw)
    loss = F.nll_loss(out["logp"], y)
    ext = list(extra(out)) if extra else []
    gs = torch.autograd.grad(loss, [t[k] for k in PARAMS] + [xr] + ext)
    grads = {k: g.detach() for k, g in zip(PARAMS + ["x"], gs)}
    return out, loss.detach(), grads, [g.detach() for g in gs[len(PARAMS) + 1:]]


@functools.lru_cache(maxsize=None)
def reference(shape):
    """the float64 evaluation of a case, computed once and shared: (sd, x, y, out, loss, grads)"""
    sd, x, y = case_inputs(shape)
    out, loss, grads, _ = loss_and_grads(sd, x, y)
    return sd, x, y, out, loss, grads


def decided(out, shape):
    """bool [B]: frontend_restate.m5_decided on the train-mode pre-pool activations at the case's tau"""
    return FR.m5_decided(out["y"], tau(shape))


# ---- exact ties: first maximum wins -------------------------------------------------------------------------------------
# Clips made of 256-sample segments, each 16 copies of its own 16-sample pattern.  Stage 1 has stride 16, so inside a segment every
# position sees the same samples: of each four pooling windows (64 samples apart, 128 samples wide) three lie inside one segment and
# hold four EQUAL values -- bit-equal in any arithmetic that treats the positions alike -- and nn.MaxPool1d hands the gradient to the
# first.  The segments differ, so the batch statistics are ordinary.  Every other window of every stage is decided at TIE_TAU.
TIE_SHAPE = (2, 6848, 32, 10)
TIE_PREPOOL_F32_ERR = 3.4e-6        # float32-torch pre-pool error of this case, measured by __main__
TIE_TAU = 4 * TIE_PREPOOL_F32_ERR
TIE_SEED = 0


def tie_clips(B, L, seed):
    nseg = (L + 255) // 256
    pat = torch.from_numpy(synth.uniform("m5tie", (B, nseg, 16), seed, -0.5, 0.5))
    return pat.repeat_interleave(16, dim=1).reshape(B, 1, nseg * 256)[..., :L].contiguous()


def tied_windows(y):
    """bool [B,C,Q]: the four values of the pooling window are equal"""
    B, C, P = y.shape
    w = y.detach()[:, :, :(P // 4) * 4].reshape(B, C, P // 4, 4)
    return w.max(dim=-1).values == w.min(dim=-1).values


def decided_or_tied(ys, t):
    """bool [B]: every pooling window of the clip is decided at t (frontend_restate.m5_decided) or exactly tied"""
    ok = torch.ones(ys[0].shape[0], dtype=torch.bool)
    for y in ys:
        B, C, P = y.shape
        w = y.detach()[:, :, :(P // 4) * 4].reshape(B, C, P // 4, 4)
        top = w.topk(2, dim=-1).values
        mx, gap = top[..., 0], top[..., 0] - top[..., 1]
        bad = ((mx > 0) & ((mx <= t) | ((gap <= t) & ~tied_windows(y)))) | ((mx <= 0) & (mx >= -t))
        ok &= ~bad.reshape(B, -1).any(dim=1)
    return ok


@functools.lru_cache(maxsize=None)
def tie_reference():
    B, L, nc, no = TIE_SHAPE
    sd, x, y = weights(no, nc), tie_clips(B, L, TIE_SEED), labels(B, no)
    out, loss, grads, _ = loss_and_grads(sd, x, y)
    return sd, x, y, out, loss, grads


def grad_errors(got, ref):
    """{name: max |got - ref| / max |ref|}; a conv bias by max |ref dW| of its stage (its own reference is an exact zero)"""
    errs = {}
    for k, r in ref.items():
        top = ref[k.replace("bias", "weight")].abs().max() if k.startswith("conv") and k.endswith("bias") else r.abs().max()
        errs[k] = float((got[k].double() - r.double()).abs().max() / top)
    return errs


def dw2_without_tail(shape):
    """dW_2 as an implementation would form it that drops the dz of the pre-pool positions at and beyond 4 Q_2"""
    sd, x, y = case_inputs(shape)
    out, _, _, (dz2,) = loss_and_grads(sd, x, y, extra=lambda o: [o["z"][1]])
    Q2 = dz2.shape[-1] // 4
    dz2 = dz2.clone()
    dz2[..., 4 * Q2:] = 0.0
    return torch.einsum("bop,bcpt->oct", dz2, out["a"][0].detach().unfold(2, 3, 1)), dz2.shape[-1] - 4 * Q2


def adam_trajectory(sd, x, y, steps=3, dtype=torch.float64, lr=0.01, weight_decay=1e-4):
    """`steps` steps of the reference's training loop (M5/train.py:40,86-103: Adam, lr 0.01, weight_decay 1e-4) ->
    ([loss per step], state dict after the last step, running statistics and num_batches_tracked included)"""
    t = tensors(sd, dtype)
    opt = torch.optim.Adam([t[k] for k in PARAMS], lr=lr, weight_decay=weight_decay)
    losses, xd = [], x.to(dtype)
    for _ in range(steps):
        out = forward(t, xd)
        loss = F.nll_loss(out["logp"], y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        for k, v in out["running"].items():
            t[k] = v
        losses.append(float(loss.detach()))
    final = {k: v.detach() for k, v in t.items()}
    for i in (1, 2, 3, 4):
        final[f"bn{i}.num_batches_tracked"] = torch.as_tensor(int(sd[f"bn{i}.num_batches_tracked"]) + steps)
    return losses, final


def prepool_f32_error(sd, x):
    t64, t32 = tensors(sd, torch.float64, False), tensors(sd, torch.float32, False)
    with torch.no_grad():
        y64, y32 = forward(t64, x.double())["y"], forward(t32, x.float())["y"]
    return max(float((a.double() - b).abs().max()) for a, b in zip(y32, y64))


def search_seed(shape, t):
    B, L, nc, no = shape
    sd = weights(no, nc)
    t64 = tensors(sd, torch.float64, False)
    for seed in range(256):
        with torch.no_grad():
            ys = forward(t64, clips(B, L, seed).double())["y"]
        if bool(FR.m5_decided(ys, t).all()):
            return seed
    return None


if __name__ == "__main__":
    worst = 0.0
    for shape in SHAPES:
        B, L, nc, no = shape
        sd = weights(no, nc)
        e = prepool_f32_error(sd, clips(B, L, DEFAULT_SEED))
        seed = search_seed(shape, 4 * float(f"{e:.1e}"))
        print(f"{shape}: pre-pool float32 error {e:.1e}, tau {4 * float(f'{e:.1e}'):.1e}, first all-decided seed {seed}")
        x, y = clips(B, L, DEFAULT_SEED if seed is None else seed), labels(B, no)
        _, _, g64, _ = loss_and_grads(sd, x, y)
        _, _, g32, _ = loss_and_grads(sd, x, y, torch.float32)
        errs = grad_errors(g32, g64)
        k = max(errs, key=errs.get)
        worst = max(worst, errs[k])
        print(f"    float32 gradient error: worst {errs[k]:.2e} at {k}; dx {errs['x']:.2e}")
    print(f"largest float32 gradient error over the table: {worst:.2e}")
    B, L, nc, no = TIE_SHAPE
    sd = weights(no, nc)
    e = prepool_f32_error(sd, tie_clips(B, L, 0))
    t64 = tensors(sd, torch.float64, False)
    for seed in range(256):
        with torch.no_grad():
            ys = forward(t64, tie_clips(B, L, seed).double())["y"]
        if bool(decided_or_tied(ys, 4 * float(f"{e:.1e}")).all()):
            break
    else:
        seed = None
    print(f"ties {TIE_SHAPE}: pre-pool float32 error {e:.1e}, first seed with every window decided or tied: {seed}")
    if seed is not None:
        x, y = tie_clips(B, L, seed), labels(B, no)
        out, _, g64, _ = loss_and_grads(sd, x, y)
        _, _, g32, _ = loss_and_grads(sd, x, y, torch.float32)
        _, _, glast, _ = loss_and_grads(sd, x, y, stage1_last_max=True)
        tw = tied_windows(out["y"][0]) & (out["y"][0].detach()[..., ::4][..., :tied_windows(out["y"][0]).shape[-1]] > 0)
        errs, wrong = grad_errors(g32, g64), grad_errors(glast, g64)
        print(f"    tied open windows in stage 1: {int(tw.sum())} of {tw.numel()}; float32 error worst {max(errs.values()):.2e}; "
              f"last-max-wins differs by {wrong['x']:.2e} (dx) {wrong['conv1.weight']:.2e} (conv1.weight)")
