"""Write tests/golden/golden_pgd_v1.npz: what the reference's own PGD loops return on the cases of tests/pgd_restate.py.

    python tests/golden/make_golden_pgd.py /path/to/AudioPure      (or set AUDIOPURE_REFERENCE)

The two ``pgd`` functions sit inside scripts that parse arguments and open datasets when imported
(audio_models/RCNN_KWS/train.py, audio_models/ConvNets_SpeechCommands/adv_train_speech_commands.py), so the ``FunctionDef`` of each --
and of ``project_to_norm_ball`` -- is taken out of the script's source with ``ast`` at run time and compiled in a namespace that holds
``torch``, ``np``, ``Union`` and an identity ``Wave2Spect``.  ``AudioAttack`` is imported as make_golden_psy.py imports it.  Nothing of
the reference's text is written anywhere; the file holds the recorded draws of ``torch.rand_like`` and the returned tensors only.

The loops are driven by the scripted model of pgd_restate.py (recorded scores forward, a recorded gradient backward), on the CPU, so
the outputs depend on no model numerics.  Keys, per case name:  <name>/u  and  <name>/<form>/x_adv  for the forms kws, convnet,
convnet_l2, stage1_t, stage1_u, plus  <name>/<form>/success  for the two stage-1 forms; and  audio_attack/attributes, the attribute names
of an ``AudioAttack`` instance (what ``audiopure_amd.attacks.stage_1`` may read).
"""
import ast
import importlib.util
import os
import sys
from typing import Union

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pgd_restate as R  # noqa: E402
from make_golden_psy import load_reference  # noqa: E402


def functions_of(path, names, namespace):
    """compile the named top-level functions of a script, and nothing else of it, into `namespace`"""
    tree = ast.parse(open(path).read(), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in names]
    assert {d.name for d in defs} == set(names), (path, [d.name for d in defs])
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), namespace)
    return namespace


class RecordedRand:
    """torch.rand_like replaced by a recorder, seeded per call so that every form of a case starts from the same draws"""

    def __init__(self, seed):
        self.seed, self.u, self.orig = seed, None, torch.rand_like

    def __enter__(self):
        def rand_like(x, **kw):
            torch.manual_seed(self.seed)
            out = self.orig(x, **kw)
            self.u = out.detach().clone()
            return out
        torch.rand_like = rand_like
        return self

    def __exit__(self, *exc):
        torch.rand_like = self.orig


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("AUDIOPURE_REFERENCE")
    if not ref:
        raise SystemExit("usage: make_golden_pgd.py /path/to/AudioPure  (or set AUDIOPURE_REFERENCE)")
    base = dict(torch=torch, np=np, Union=Union, Wave2Spect=lambda x: x)
    kws = functions_of(os.path.join(ref, "audio_models", "RCNN_KWS", "train.py"), {"pgd"}, dict(base))
    cnn = functions_of(os.path.join(ref, "audio_models", "ConvNets_SpeechCommands", "adv_train_speech_commands.py"),
                       {"pgd", "project_to_norm_ball"}, dict(base))
    wb = load_reference(ref)
    out = {}
    for seed, name in enumerate(R.CASES):
        B, L, n = R.CASES[name]
        c = R.case(name)
        x, y, y_t = torch.from_numpy(c["x"]), torch.from_numpy(c["y"]), torch.from_numpy(c["y_t"])
        with RecordedRand(seed) as rec:
            out[f"{name}/kws/x_adv"] = kws["pgd"](R.model_of(c), lambda v: v, x.clone(), y, torch.nn.CrossEntropyLoss(),
                                                  eps=R.EPS, alpha=R.ALPHA, n=n).detach().numpy()
            u = rec.u
            out[f"{name}/convnet/x_adv"] = cnn["pgd"](R.model_of(c), x.clone(), y, eps=R.EPS, alpha=R.ALPHA, n=n, p="linf").detach().numpy()
            assert torch.equal(rec.u, u)
            out[f"{name}/convnet_l2/x_adv"] = cnn["pgd"](R.model_of(c, "G_l2"), x.clone(), y, eps=R.EPS, alpha=R.ALPHA, n=n,
                                                         p="l2").detach().numpy()
            assert torch.equal(rec.u, u)
        out[f"{name}/u"] = u.numpy()
        for form, targeted, labels in (("stage1_t", True, y_t), ("stage1_u", False, y)):
            attack = wb.AudioAttack(R.model_of(c), masker=None, criterion=torch.nn.CrossEntropyLoss(), eps=R.EPS, norm="linf",
                                    learning_rate_1=R.LR, max_iter_1=n, max_iter_2=0, eot_attack_size=1, eot_defense_size=1, verbose=0)
            x_adv, (success, _) = attack.generate(x.clone(), labels, targeted=targeted)
            out[f"{name}/{form}/x_adv"] = x_adv.detach().numpy()
            out[f"{name}/{form}/success"] = np.asarray(success, dtype=np.bool_)
    # the names an AudioAttack instance carries (with EOT: eot_model too), and that generate() leaves its `targeted` in `_targeted`
    attack = wb.AudioAttack(R.model_of(c), masker=None, max_iter_1=0, max_iter_2=0, eot_attack_size=1, eot_defense_size=1, verbose=0)
    names = set(vars(attack))
    try:                                                         # (the constructor's `from ._EOT import EOT` needs a package around the module)
        pkg_dir = os.path.join(ref, "robustness_eval")
        spec = importlib.util.spec_from_file_location("ref_robustness_eval", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
        sys.modules["ref_robustness_eval"] = importlib.util.module_from_spec(spec)
        wb.__package__ = "ref_robustness_eval"
        names |= set(vars(wb.AudioAttack(R.model_of(c), masker=None, max_iter_1=0, max_iter_2=0, eot_attack_size=2, eot_defense_size=2, verbose=0)))
    finally:
        sys.modules.pop("ref_robustness_eval", None)
    for flag in (True, False):
        attack.generate(x.clone(), y, targeted=flag)
        assert attack._targeted is flag
    out["audio_attack/attributes"] = np.array(sorted(names))
    path = os.path.join(HERE, "golden_pgd_v1.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
