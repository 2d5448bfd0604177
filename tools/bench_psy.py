"""Time the attack's stage-2 hooks on the GPU (ap_psy.hip): the masking threshold (``threshold_and_psd_maximum``) at B = 10
and B = 512, and the hinge loss with its gradient (``masking_threshold_loss_and_grad``), L = 16000.  Next to them, in the
same process: the reference's torch-operator loss (``torch.stft`` with autograd on the device, restated with
``return_complex``) and the host numpy masker (tests/psy_restate.py, the reference's per-clip, per-frame loops) at B = 10;
and one stage-2 iteration at B = 10 through the default purifier (RevDiffWave t* = 2 on the shipped WaveNet, M5), whose
share the hooks take.

    python tools/bench_psy.py [--iters 20] [--out profiles/psy_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o psy -- python tools/bench_psy.py --iters 5 --kernels-only

Times are device-event means over ``--iters`` calls after a warm-up (host wall time for the numpy masker)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from audiopure_amd import synth  # noqa: E402
from audiopure_amd.robustness_eval import psychoacoustic as P  # noqa: E402


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per call


def _torch_loss(delta, thr, pm):
    """The reference's _loss_gradient_masking_threshold on device tensors (torch.stft + autograd), minus its host copy."""
    d = delta.detach()[:, 0].clone().requires_grad_(True)
    X = torch.view_as_real(torch.stft(d, n_fft=2048, hop_length=512, win_length=2048, center=False,
                                      window=torch.hann_window(2048, device=d.device), return_complex=True))
    a = torch.sqrt(torch.sum(torch.square(float(np.sqrt(8.0 / 3.0)) * X / 2048), -1))
    psd = pow(10.0, 9.6) / pm.reshape(-1, 1, 1) * torch.square(a)
    loss = torch.mean(torch.relu(psd - thr), dim=(1, 2))
    loss.sum().backward()
    return d.grad, loss.detach()


def _stage2_iteration(dev, B, iters):
    from audiopure_amd.acoustic_system import AcousticSystem
    from audiopure_amd.audio_models.M5.M5Net import M5
    from audiopure_amd.diffusion_models.diffwave_ddpm import DiffWave
    from audiopure_amd.diffusion_models.diffwave_sde import RevDiffWave
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.WaveNet import WaveNet_Speech_Commands
    from audiopure_amd.diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
    cfg = dict(synth.FULL_WAVENET_CONFIG)
    net = WaveNet_Speech_Commands(**cfg)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.wavenet_state_dict(cfg, 0).items()})
    dw = DiffWave(model=net.to(dev), diffusion_hyperparams=calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG),
                  reverse_timestep=2)
    runner = RevDiffWave.from_model(dw, types.SimpleNamespace(t=2, rand_t=False, t_delta=0, use_bm=False, sample_step=1,
                                                              score_type="guided_diffusion"))
    m5 = M5(n_input=1, n_output=10)
    m5.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.m5_state_dict(10).items()})
    model = AcousticSystem(classifier=m5.to(dev).eval(), transform=None, defender=runner, defense_type="wave")
    x = torch.from_numpy(synth.waveforms(B, 16000, seed=3)).to(dev)
    y = torch.arange(B, device=dev) % 10
    masker = P.PsychoacousticMasker()
    thr, pm = masker.threshold_and_psd_maximum(x)
    delta = (0.002 * torch.randn_like(x)).requires_grad_(True)

    def net_part():
        out = model(x + delta)
        torch.nn.functional.cross_entropy(out, y).backward()
        delta.grad = None

    def hooks():
        P.masking_threshold_loss_and_grad(delta, thr, pm)

    return _time(net_part, iters), _time(hooks, iters), _time(lambda: masker.threshold_and_psd_maximum(x), iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="only the native launches (for a rocprofv3 kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    res = {"L": 16000, "window": 2048, "hop": 512, "iters": args.iters, "native_us": {}, "device": torch.cuda.get_device_name(0)}
    masker = P.PsychoacousticMasker()
    for B in (10, 512):
        x = (0.2 * torch.randn(B, 1, 16000, generator=g)).to(dev)
        delta = (0.01 * torch.randn(B, 1, 16000, generator=g)).to(dev)
        thr, pm = masker.threshold_and_psd_maximum(x)
        res["native_us"][f"threshold_B{B}"] = round(_time(lambda: masker.threshold_and_psd_maximum(x), args.iters), 1)
        res["native_us"][f"loss_grad_B{B}"] = round(_time(lambda: P.masking_threshold_loss_and_grad(delta, thr, pm),
                                                          args.iters), 1)
        if B == 10 and not args.kernels_only:
            res["torch_stft_autograd_loss_grad_B10_us"] = round(_time(lambda: _torch_loss(delta, thr, pm), args.iters), 1)
            import psy_restate as R
            xs = x[:, 0].cpu().numpy()
            t0 = time.perf_counter()
            for c in xs:
                R.threshold(c)
            res["host_numpy_threshold_B10_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    if not args.kernels_only:
        t_net, t_hooks, t_thr = _stage2_iteration(dev, 10, max(2, args.iters // 4))
        res["stage2_iteration_B10"] = {
            "purifier_and_classifier_fwd_bwd_us": round(t_net, 1), "loss_grad_hook_us": round(t_hooks, 1),
            "threshold_once_per_attack_us": round(t_thr, 1),
            "hook_share_of_iteration": round(t_hooks / (t_net + t_hooks), 5),
            "purifier": "RevDiffWave t*=2 (shipped WaveNet config, f32) + M5"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
