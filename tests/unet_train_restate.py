"""float64 restatement, in plain torch functionals, of the train step of the Improved-Diffusion UNet: the reference's
``GaussianDiffusion.training_losses`` (gaussian_diffusion.py:709-746; MSE on epsilon, T = 200 linear, q_sample with one step per sample)
around ``UNetModel(...).train()`` (unet.py:462-491, nn.Dropout(p) live in every ResBlock), gradients by torch autograd.  It walks a
parameter-holder ``UNetModel`` as oracle/unet_oracle.py does, but in the dtype of the module it is given (the oracle forces float32)
and with the dropout mask of ``ap_dropout`` (Philox4x32-10, oracle/philox.py).  The float64 call is the reference; the float32 call
measures what float32 arithmetic alone costs.  Test infrastructure only: test_unet_train_cpu.py pins it to the reference's own numbers
(tests/golden/golden_unet_train_v1.npz) and asserts the conditions the GPU bounds rest on; the GPU tests pin the kernels to it.

    python tests/unet_train_restate.py        # re-measure the float32 errors of every case (CPU)
"""
import functools
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.diffusion_models.improved_diffusion_unet import UNetModel  # noqa: E402
from oracle.philox import philox4x32_10  # noqa: E402
from synth_convnets import synth_init  # noqa: E402

T_STEPS = 200
# constructor arguments shared with the reference's own UNetModel in tests/golden/make_golden_unet_train.py
MINI = dict(in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(2, 4), channel_mult=(1, 2, 2),
            num_heads=2, use_scale_shift_norm=True)                    # tests/test_unet_oracle_golden.py::mini_unet
CASES = {
    # name: (constructor arguments, p, B, steps, seed of weights / inputs / dropout, image side)
    "a": (MINI, 0.3, 3, (0, 37, 199), 1, 32),
    "b": (MINI, 0.0, 2, (5, 120), 1, 32),
    # 64 channels per head (the MFMA attention form, T = 256) and GroupNorm32 on 64 channels (2 channels per group): model_channels =
    # 64, mult (1, 2), attention at the second level and in the middle block, both on 128 channels.  TWO heads, not one: with one head
    # those blocks would have 128 channels per head, which ap_attention_qkv does not build (8, 16, 32, 64), forward or backward.
    "c": (dict(in_channels=1, model_channels=64, out_channels=1, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
               num_heads=2, use_scale_shift_norm=True), 0.3, 2, (11, 150), 1, 32),
}
SAMPLE_OFFSET = 7                                                       # a non-zero global sample index

# ---- bounds: 4 x the error of float32 torch (this same walk in float32 with autograd, on the CPU) against the float64
# walk, per tensor as max |d| / max |ref|, maximised over tensors and cases.  Measured by this file's __main__ and re-measured by
# test_unet_train_cpu.py:
#   forward (eps, the per-sample loss terms)         a 1.05e-6   b 1.07e-6   c 7.10e-7
#   gradients (every parameter; dx)                  a 1.64e-5   b 6.31e-5   c 2.17e-6
# (a, b: the worst tensor is output_blocks.4.0.out_layers.3.bias, a plain sum of cotangents that largely cancels; c:
# output_blocks.2.0.in_layers.2.bias.)  Parameters whose gradient is 0 in exact arithmetic are scaled by their layer's max |dW|:
# `structural_zeros`.
FWD_F32_ERR = 1.07e-6
GRAD_F32_ERR = 6.31e-5
FWD_BOUND = 4 * FWD_F32_ERR
GRAD_BOUND = 4 * GRAD_F32_ERR
MIN_VAR_OVER_EPS = 100.0                                                # every (sample, group) variance entering a GroupNorm


def dropout_mask(seed, draw, sample_offset, B, n, p):
    """The multiplier of ``ap_dropout`` [B][n] float32: 0 where dropped, fp32(1 / (1 - p)) where kept.  Element e of sample b takes word
    e % 4 of Philox4x32-10(counter = (e // 4, draw, low and high word of sample_offset + b), key = the words of seed);
    u = (r >> 8) 2^-24, kept iff u >= fp32(p)."""
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    out = np.empty((B, n), np.float32)
    s = np.float32(1.0 / (1.0 - float(np.float32(p))))
    for b in range(B):
        u_ = sample_offset + b
        r = philox4x32_10(q, np.full(nq, draw), np.full(nq, u_ & 0xFFFFFFFF), np.full(nq, u_ >> 32), seed & 0xFFFFFFFF, seed >> 32)
        u = (np.stack(r, 1).reshape(-1)[:n] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
        out[b] = np.where(u >= np.float32(p), s, np.float32(0.0))
    return out


def tables():
    betas = np.linspace(0.0001, 0.02, T_STEPS, dtype=np.float64)        # script_util.py:231-269 -> gaussian_diffusion.py:27-35
    ac = np.cumprod(1.0 - betas)
    return np.sqrt(ac), np.sqrt(1.0 - ac)


def timestep_embedding(t, dim):                                         # nn.py:103-121, float32 as the reference computes it
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def _silu(x):
    return x * torch.sigmoid(x)


class Walk:
    """One train-mode evaluation of a holder UNetModel in its parameters' dtype.  drop = (seed, sample_offset, p)."""

    def __init__(self, model, drop, info=None):
        self.m, self.drop, self.draw, self.info = model, drop, 0, info

    def gn(self, g, x):
        if self.info is not None:
            xs = x.detach().reshape(x.shape[0], g.num_groups, -1)
            self.info["min_var_over_eps"] = min(self.info.get("min_var_over_eps", float("inf")),
                                                float(xs.var(2, unbiased=False).min()) / g.eps)
        return F.group_norm(x, g.num_groups, g.weight, g.bias, g.eps)

    def dropout(self, h):
        seed, offset, p = self.drop
        draw, self.draw = self.draw, self.draw + 1
        if p == 0.0:
            return h
        B, n = h.shape[0], h[0].numel()
        mask = dropout_mask(seed, draw, offset, B, n, p)
        if self.info is not None:
            self.info.setdefault("kept", []).append((float((mask > 0).mean()), B * n))
        return h * torch.from_numpy(mask).to(h.dtype).reshape(h.shape)

    def resblock(self, rb, x, emb):                                     # unet.py:180-194
        h = rb.in_layers[2](_silu(self.gn(rb.in_layers[0], x)))
        scale, shift = torch.chunk(rb.emb_layers[1](_silu(emb))[..., None, None], 2, dim=1)
        h = self.gn(rb.out_layers[0], h) * (1 + scale) + shift
        h = rb.out_layers[3](self.dropout(_silu(h)))
        return rb.skip_connection(x) + h

    def attention(self, ab, x):                                         # unet.py:226-252
        b, c, *spatial = x.shape
        xf = x.reshape(b, c, -1)
        qkv = ab.qkv(self.gn(ab.norm, xf))
        qkv = qkv.reshape(b * ab.num_heads, -1, qkv.shape[2])
        ch = qkv.shape[1] // 3
        q, k, v = torch.split(qkv, ch, dim=1)
        scale = 1 / math.sqrt(math.sqrt(ch))
        w = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale), dim=-1)
        h = torch.einsum("bts,bcs->bct", w, v).reshape(b, -1, qkv.shape[2])
        return (xf + ab.proj_out(h)).reshape(b, c, *spatial)

    def run(self, seq, h, emb):
        for layer in seq:
            name = type(layer).__name__
            if name == "ResBlock":
                h = self.resblock(layer, h, emb)
            elif name == "AttentionBlock":
                h = self.attention(layer, h)
            elif name == "Downsample":
                h = layer.op(h)
            elif name == "Upsample":
                h = layer.conv(F.interpolate(h, scale_factor=2, mode="nearest"))
            else:
                h = layer(h)
        return h

    def __call__(self, x, t):
        m = self.m
        dtype = next(m.parameters()).dtype
        emb = m.time_embed[2](_silu(m.time_embed[0](timestep_embedding(t, m.model_channels).to(dtype))))
        hs, h = [], x.to(dtype)
        for blk in m.input_blocks:
            h = self.run(blk, h, emb)
            hs.append(h)
        h = self.run(m.middle_block, h, emb)
        for blk in m.output_blocks:
            h = self.run(blk, torch.cat([h, hs.pop()], dim=1), emb)
        return m.out[2](_silu(self.gn(m.out[0], h)))


def build(name):
    """The holder module of a case with seeded float32 weights (a fresh one: callers may move or modify it)."""
    kw, p, _, _, seed, _ = CASES[name]
    return synth_init(UNetModel(dropout=p, **kw), seed)


def drop_of(name):
    _, p, _, _, seed, _ = CASES[name]
    return (0x9E3779B97F4A7C15 ^ seed, SAMPLE_OFFSET, p)                # a seed with both words in use


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (x_start, t, noise): float32 [B, 1, side, side], int64 [B], float32.  Shared by the tests: do not modify."""
    _, _, B, steps, seed, HW = CASES[name]
    x0 = torch.from_numpy(synth.uniform("unt/x/" + name, (B, 1, HW, HW), seed, -1.0, 1.0))
    z = torch.from_numpy(synth.normal("unt/z/" + name, (B, 1, HW, HW), seed))
    return x0, torch.tensor(steps, dtype=torch.long), z


def q_sample(x0, t, z, dtype):
    """_extract_into_tensor's float32 coefficients applied in `dtype`."""
    sa, sb = tables()
    a = torch.from_numpy(sa[t.numpy()].astype(np.float32)).to(dtype).reshape(-1, 1, 1, 1)
    b = torch.from_numpy(sb[t.numpy()].astype(np.float32)).to(dtype).reshape(-1, 1, 1, 1)
    return a * x0.to(dtype) + b * z.to(dtype)


def train_step(model, name, info=None):
    """One step without the optimizer in the dtype of `model`'s parameters -> dict(eps, mse [B], grads {name: d mean(mse) / d
    parameter}, dx = d mean(mse) / d x_t, x_t)."""
    dtype = next(model.parameters()).dtype
    x0, t, z = inputs(name)
    x_t = q_sample(x0, t, z, dtype).requires_grad_(True)
    for q in model.parameters():
        q.grad = None
    eps = Walk(model, drop_of(name), info)(x_t, t)
    mse = ((z.to(dtype) - eps) ** 2).flatten(1).mean(1)
    mse.mean().backward()
    grads = {k: q.grad.detach().clone() for k, q in model.named_parameters()}
    return dict(eps=eps.detach(), mse=mse.detach(), grads=grads, dx=x_t.grad.detach(), x_t=x_t.detach())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of a case -> (step dict, info).  Computed once, shared by the tests, never modified."""
    info = {}
    return train_step(build(name).double(), name, info), info


def rel(a, ref):
    """max |a - ref| / max |ref|, in float64"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    d, s = float((a - ref).abs().max()), float(ref.abs().max())
    return d / s if s > 0 else d


def structural_zeros(model):
    """Parameters whose gradient is 0 in exact arithmetic: the bias of a ResBlock's first conv when the GroupNorm32 behind it
    (unet.py:150-152) has ONE channel per group -- the norm removes a per-channel constant.  (32-channel blocks of the mini net.)
    The float64 gradient there is rounding noise; its error is scaled by the same conv's max |dW|, as the conv biases in front of a
    BatchNorm are in DESIGN 3.11 / 3.12.  -> {bias name: weight name}"""
    out = {}
    for k, mod in model.named_modules():
        if type(mod).__name__ == "ResBlock" and mod.out_layers[0].num_channels == mod.out_layers[0].num_groups:
            out[k + ".in_layers.2.bias"] = k + ".in_layers.2.weight"
    # likewise the biases that feed only the closing GroupNorm32 (`out.0`, unet.py:432-436): the last ResBlock's second conv and skip
    if model.out[0].num_channels == model.out[0].num_groups:
        last = f"output_blocks.{len(model.output_blocks) - 1}.0"
        out[last + ".out_layers.3.bias"] = last + ".out_layers.3.weight"
        if not isinstance(model.output_blocks[-1][0].skip_connection, torch.nn.Identity):
            out[last + ".skip_connection.bias"] = last + ".skip_connection.weight"
    return out


def compare(got, ref, zeros=None):
    """-> (forward error, gradient error, name of the worst gradient tensor) of a step dict against `ref`; `zeros`:
    ``structural_zeros`` of the case's module"""
    zeros = zeros or {}
    fwd = max(rel(got["mse"], ref["mse"]), rel(got["eps"], ref["eps"])) if "eps" in got else rel(got["mse"], ref["mse"])
    worst, wname = rel(got["dx"], ref["dx"]) if got.get("dx") is not None else 0.0, "dx"
    for k, r in ref["grads"].items():
        if k in zeros:
            e = float((got["grads"][k].detach().double().cpu() - r.double()).abs().max()) / float(ref["grads"][zeros[k]].abs().max())
        else:
            e = rel(got["grads"][k], r)
        if e > worst:
            worst, wname = e, k
    return fwd, worst, wname


def measure_f32(name):
    """float32 torch (this walk in float32, autograd) against the float64 walk -> (forward error, gradient error, worst tensor)"""
    m = build(name)
    return compare(train_step(m, name), reference(name)[0], structural_zeros(m))


# ---- the golden: the reference's own classes on cases a and b (tests/golden/make_golden_unet_train.py) --------------------------------
GOLDEN_FULL = ("input_blocks.0.0.weight", "input_blocks.0.0.bias", "input_blocks.1.0.in_layers.2.weight", "input_blocks.2.0.op.weight",
               "input_blocks.3.0.skip_connection.weight", "input_blocks.3.1.qkv.weight", "input_blocks.3.1.proj_out.weight",
               "input_blocks.1.0.out_layers.0.weight", "input_blocks.1.0.out_layers.0.bias", "input_blocks.1.0.emb_layers.1.weight",
               "input_blocks.1.0.emb_layers.1.bias", "time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight",
               "time_embed.2.bias", "out.2.weight", "out.2.bias")


def golden_probe(key, shape):
    """the seeded vector a gradient tensor that the golden does not hold in full is contracted with (float64)"""
    return torch.from_numpy(synth.normal("unt/probe/" + key, tuple(shape), 0)).double()


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "golden_unet_train_v1.npz")))


def compare_golden(got, name, ref):
    """-> (forward error, gradient error) of a step dict against the reference's own float32 numbers.  A tensor held in full is measured
    like ``compare``; an inner product <g, probe> is scaled by sum |ref g| |probe| (what a per-element error of max |ref g| relative
    size would move it by, at most)."""
    G, pre = golden(), name + "/"
    fwd = rel(got["mse"], torch.from_numpy(G[pre + "mse"]))
    if "eps" in got:
        fwd = max(fwd, rel(got["eps"], torch.from_numpy(G[pre + "eps"])))
    grad = rel(got["dx"], torch.from_numpy(G[pre + "dx"])) if got.get("dx") is not None else 0.0
    zeros = structural_zeros(build(name))
    for k, g in got["grads"].items():
        if k in zeros:
            continue                                                   # noise in the reference's float32 run too: see `compare`
        if pre + "grad/" + k in G:
            grad = max(grad, rel(g, torch.from_numpy(G[pre + "grad/" + k])))
        else:
            pr = golden_probe(k, g.shape)
            r = ref["grads"][k].double()
            scale = float(r.abs().max()) * float(pr.abs().sum())
            grad = max(grad, abs(float((g.double().cpu() * pr).sum()) - float(G[pre + "dot/" + k])) / scale)
    return fwd, grad


if __name__ == "__main__":
    wf = wg = 0.0
    for name in CASES:
        f, g, k = measure_f32(name)
        info = reference(name)[1]
        wf, wg = max(wf, f), max(wg, g)
        print(f"{name}: fwd {f:.2e}  grad {g:.2e} ({k})  min var / eps {info['min_var_over_eps']:.3g}  kept {info.get('kept', [])[:3]}")
    print(f"FWD_F32_ERR {wf:.2e} (recorded {FWD_F32_ERR:.2e})   GRAD_F32_ERR {wg:.2e} (recorded {GRAD_F32_ERR:.2e})")
