"""The native optimizer step under each network family's native training step: two iterations of zero_grad, native backward, native
``step()`` beside the same loop on ``torch.optim`` from the same start, and beside ``torch.optim`` handed the same gradients.  The
parameters are held to the Adam / SGD bound of tests/optim_restate.py (its units: lr for Adam and AdamW, lr x the tensor's largest
momentum entry for SGD), and the models see the update: they key their device images on (_version, data_ptr), and the kernel
writes through raw pointers, so the step bumps the version counter of every tensor it wrote -- without that the eval() output
after the steps is the one from before them."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import optim_restate as OR
from audiopure_amd import optim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERS = 2


# ---- one small case per family: -> dict(model, params (named), loss(), out() in eval mode, fresh(state_dict) -> out) ---------------------
def _resnext():
    import convnet_train_restate as R
    from audiopure_amd.convnet import NativeConvNet
    m, _, x, y = R.case("resnext")
    x, y = x.to(DEV), y.to(DEV)

    def wrap(state=None):
        mod = copy.deepcopy(m).to(DEV)
        if state is not None:
            mod.load_state_dict(state)                        # before the wrapper lowers: its eval plan folds the weights it finds
        return NativeConvNet(mod, R.CHW)
    net = wrap().train()

    def out(n):
        with torch.no_grad():
            o = n.eval()(x).clone()
        n.train()
        return o
    return dict(model=net, named=lambda: net.module.named_parameters(), loss=lambda: F.cross_entropy(net(x), y), out=lambda: out(net),
                fresh=lambda: out(wrap(net.module.state_dict())),
                opt=("SGD", dict(lr=0.05, momentum=0.9, weight_decay=1e-2)))


def _unet():
    import unet_train_restate as R
    from audiopure_amd.diffusion_models.improved_diffusion_train import training_losses
    m = R.build("b").to(DEV)
    x0, t, z = R.inputs("b")
    x, zd, ts = x0.to(DEV), z.to(DEV), t.to(DEV).float()
    seed, offset, _ = R.drop_of("b")

    def out(n):
        n.eval()
        with torch.no_grad():
            o = n(x, ts).clone()
        n.train()
        return o

    def fresh():
        n = R.build("b").to(DEV)
        n.load_state_dict(m.state_dict())
        return out(n)
    return dict(model=m, named=m.named_parameters,
                loss=lambda: training_losses(m, x, t, noise=zd, dropout=("philox", seed, offset))["loss"].mean(), out=lambda: out(m),
                fresh=fresh, opt=("AdamW", dict(lr=1e-3)), ema=0.9999, norm=True)


def _m5():
    import m5_train_restate as T
    from audiopure_amd.audio_models.M5.M5Net import M5
    shape = T.SHAPES[0]
    B, L, nc, no = shape
    sd, x, y = T.case_inputs(shape)
    xd, yd = x.to(DEV), y.to(DEV)

    def make(state):
        n = M5(n_input=1, n_output=no, n_channel=nc)
        n.load_state_dict(state)
        return n.to(DEV).train()
    m = make({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})

    def out(n):
        n.eval()
        with torch.no_grad():
            o = n(xd).clone()
        n.train()
        return o
    return dict(model=m, named=m.named_parameters, loss=lambda: F.nll_loss(m(xd), yd), out=lambda: out(m),
                fresh=lambda: out(make({k: v.detach().cpu() for k, v in m.state_dict().items()})),
                opt=("Adam", dict(lr=0.01, weight_decay=1e-4)))


def _kws():
    import kws_restate as R
    import kws_train_restate as TR
    from audiopure_amd.audio_models.RCNN_KWS import KWSModel
    n_mels, H, Kc, T_, B = TR.ADAM_CASE

    def make(state):
        n = KWSModel(in_size=n_mels, hidden_size=H, num_classes=Kc)
        n.load_state_dict(state)
        return n.to(DEV).train()
    m = make(R.kws_weights(n_mels, H, Kc))
    x, y = R.kws_mel(n_mels, T_, B).to(DEV), TR.train_targets(B, Kc).to(DEV)

    def out(n):
        n.eval()
        with torch.no_grad():
            o = n(x).clone()
        n.train()
        return o
    return dict(model=m, named=m.named_parameters, loss=lambda: torch.nn.CrossEntropyLoss()(m(x), y), out=lambda: out(m),
                fresh=lambda: out(make({k: v.detach().cpu() for k, v in m.state_dict().items()})),
                opt=("Adam", dict(lr=TR.ADAM_LR, weight_decay=TR.ADAM_WD)))


def _wavenet():
    from audiopure_amd import synth
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams, training_loss
    cfg = synth.mini_wavenet_config(32, 3, 12)                # the net of test_gpu_train.py's three-step test
    B, L, steps = 3, 300, [3, 3, 150]

    def make(state):
        n = WaveNet_Speech_Commands(**cfg)
        n.load_state_dict(state, strict=True)
        return n.to(DEV)
    m = make({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, 4).items()})
    x = torch.from_numpy(synth.waveforms(B, L, seed=31)).to(DEV)
    src = (torch.tensor(steps), torch.from_numpy(synth.noise(0, B, L, seed=31)).to(DEV))
    dh = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)

    def out(n):
        with torch.no_grad():
            return n((x, torch.tensor(steps))).clone()
    return dict(model=m, named=m.named_parameters, loss=lambda: training_loss(m, torch.nn.MSELoss(), x, dh, noise_source=src),
                out=lambda: out(m), fresh=lambda: out(make({k: v.detach().cpu() for k, v in m.state_dict().items()})),
                opt=("Adam", dict(lr=1e-3, weight_decay=1e-5)))


CASES = {"resnext": _resnext, "unet": _unet, "m5": _m5, "kws": _kws, "wavenet": _wavenet}


def reference_grad_norm(params):
    """train_util.py:254-258 _log_grad_norm: one host read per parameter"""
    sqsum = 0.0
    for p in params:
        sqsum += (p.grad ** 2).sum().item()
    return math.sqrt(sqsum)


def loop(case, module):
    """ITERS iterations with `module`'s optimizer (torch.optim or audiopure_amd.optim) -> (case, optimizer, EMA copies, norms)"""
    c = CASES[case]()
    name, kw = c["opt"]
    params = [p for _, p in c["named"]()]
    before = c["out"]()                                       # builds the device image the steps must invalidate
    opt = getattr(module, name)(params, **kw)
    ema, norms = None, []
    if "ema" in c:
        ema = opt.track_ema(c["ema"]) if module is optim else [p.detach().clone() for p in params]
    for _ in range(ITERS):
        opt.zero_grad()
        c["loss"]().backward()
        if c.get("norm"):
            norms.append((opt.grad_norm() if module is optim else None, reference_grad_norm([p for p in params if p.grad is not None])))
        opt.step()
        if ema is not None and module is not optim:
            OR.reference_update_ema(ema, params, rate=c["ema"])
    return c, opt, ema, norms, before


@functools.lru_cache(maxsize=None)
def native_loop(case):
    """the native loop of a case, shared by the tests that read it: do not modify"""
    return loop(case, optim)


def _param_err(name, lr, p, q, buf):
    d = float((p.detach().double() - q.detach().double()).abs().max())
    if name == "SGD":
        b = float(buf.abs().max())
        return d / (lr * b) if b > 0 else d
    return d / lr


@pytest.mark.parametrize("case", list(CASES))
def test_two_native_iterations_beside_torch_optim(case):
    """Two independent loops from the same start, every parameter entry held to the Adam / SGD bound.

    What makes this hold on every family is that the kernel has torch.optim's bits (test_gpu_optim.py's bit-for-bit test), so the two
    loops see the same parameters, hence the same gradients, at every iteration: the figure printed is 0.  A step that is merely
    close does not pass here.  A first version of the kernel, within 2.4e-4 lr of torch.optim when handed the same gradients, ended
    6.1e-2 lr (m5, bn2.bias) and 8.5e-2 lr (unet, an attention qkv.bias) away after two iterations, against the bound of 1.12e-3 lr:
    once the loops' parameters differ in their last bits the second backward's rounding noise differs, and where a gradient entry IS
    that noise -- |g| of 1e-10 .. 4e-8 around Adam's eps, in BatchNorm and qkv biases, or conv biases in front of a normalisation
    whose true gradient is zero -- g / (|g| + eps) takes either sign."""
    nat, opt_n, _, _, _ = native_loop(case)
    ref, opt_t, _, _, _ = loop(case, torch.optim)
    name, kw = nat["opt"]
    bound = OR.SGD_BOUND if name == "SGD" else OR.ADAM_BOUND
    worst, moved, without_grad = (0.0, ""), 0, 0
    for (k, p), (k2, q) in zip(nat["named"](), ref["named"]()):
        assert k == k2
        if q.grad is None:
            assert p.grad is None and torch.equal(p.detach(), q.detach()), k
            without_grad += 1
            continue
        if name != "SGD":
            assert opt_n.state[p]["step"].item() == opt_t.state[q]["step"].item() == ITERS
        worst = max(worst, (_param_err(name, kw["lr"], p, q, opt_t.state[q].get("momentum_buffer")), k))
        moved += 1
    print(f"{case}: {name}{kw}, {moved} tensors (+ {without_grad} without a grad): native loop against the torch.optim loop after {ITERS} "
          f"iterations {worst[0]:.2e} at {worst[1]} (bound {bound:.2e})")
    assert moved > 0 and worst[0] <= bound


@pytest.mark.parametrize("case", list(CASES))
def test_native_step_on_the_same_gradients_as_torch_optim(case):
    """The native loop drives; torch.optim steps copies of the parameters with the gradients the native loop's backward produced.
    Every entry within the Adam / SGD bound; the UNet's EMA copies against the reference's update_ema on torch.optim's parameters,
    its grad_norm() against the reference loop's per-parameter sum."""
    c = CASES[case]()
    name, kw = c["opt"]
    params = [p for _, p in c["named"]()]
    shadow = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt_n, opt_t = getattr(optim, name)(params, **kw), getattr(torch.optim, name)(shadow, **kw)
    ema_n = ema_t = None
    if "ema" in c:
        ema_n, ema_t = opt_n.track_ema(c["ema"]), [p.detach().clone() for p in shadow]
    for _ in range(ITERS):
        opt_n.zero_grad()
        c["loss"]().backward()
        for p, q in zip(params, shadow):
            q.grad = None if p.grad is None else p.grad.detach().clone()
        if c.get("norm"):
            got, want = opt_n.grad_norm(), reference_grad_norm([q for q in shadow if q.grad is not None])
            print(f"{case}: grad_norm {got!r}, the reference loop's per-parameter sum {want!r}")
            assert abs(got - want) <= 1e-6 * want
            assert got == math.sqrt(opt_n.grad_sqnorm().item())
        opt_n.step()
        opt_t.step()
        if ema_t is not None:
            OR.reference_update_ema(ema_t, shadow, rate=c["ema"])
    bound = OR.SGD_BOUND if name == "SGD" else OR.ADAM_BOUND
    worst = max(_param_err(name, kw["lr"], p, q, opt_t.state[q].get("momentum_buffer")) for p, q in zip(params, shadow) if q.grad is not None)
    print(f"{case}: {name}{kw}: native step against torch.optim on the same gradients after {ITERS} iterations {worst:.2e} (bound {bound:.2e})")
    assert worst <= bound
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(params, shadow) if q.grad is None)
    if ema_n is not None:
        e = max(float((a.double() - b.double()).abs().max() / b.double().abs().max()) for a, b in zip(ema_n, ema_t))
        print(f"{case}: EMA copies {e:.2e} (bound {OR.EMA_BOUND:.2e})")
        assert e <= OR.EMA_BOUND and any(not torch.equal(a, p.detach()) for a, p in zip(ema_n, params))


@pytest.mark.parametrize("case", list(CASES))
def test_eval_after_the_native_steps_runs_on_the_updated_weights(case):
    """The stale-image check (as test_gpu_kws_train.py's three-step test does it): after the native steps the model's eval() output
    equals, bit for bit, that of a fresh model loaded with the updated state_dict, and differs from the output before the steps --
    the eval() before them built the device image that a step without the version bump would leave in place."""
    nat, _, _, _, before = native_loop(case)
    after = nat["out"]()
    assert torch.equal(after, nat["fresh"]()), "the model ran on a stale device image"
    assert float((after - before).abs().max()) > 1e-5 * float(before.abs().max())
