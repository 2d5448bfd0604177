"""Drop-in for the reference's ``robustness_eval.white_box_attack``: the checkout's own module with the second,
imperceptible attack stage (Qin et al. 2019) on the native masker.

The checkout's ``robustness_eval/white_box_attack.py`` is loaded from the other portions of this package's path (the
package path is extended over every same-named directory, ``__init__.py``) under a module name inside ``robustness_eval``,
so that its relative ``from ._EOT import EOT`` still resolves to the checkout's ``_EOT``.  Everything it defines is
re-exported unchanged -- ``stage_1`` (PGD), ``stage_2``, ``generate``, EOT, ``project_to_norm_ball``, ``lp_norm`` -- except:

* ``PsychoacousticMasker`` is ``audiopure_amd.robustness_eval.psychoacoustic.PsychoacousticMasker`` (no librosa);
* ``AudioAttack`` is a subclass that overrides only ``_stabilized_threshold_and_psd_maximum`` and
  ``_loss_gradient_masking_threshold`` (same signatures, shapes and return types), which run on the HIP kernels instead of
  host numpy and ``torch.stft``;
* ``NativeStage1AudioAttack`` is added: ``AudioAttack`` whose ``stage_1`` (PGD), for a float32 device batch [B, 1, L] under the linf
  norm, keeps the checkout's model, EOT and criterion calls and runs the per-sample loops, the update, the projection and the final
  gather on ``ap_pgd_step_linf`` (``audiopure_amd.attacks.stage_1``): one host read after the loop, the checkout's bits.  Everything
  else -- l2, 16-bit data, CPU tensors -- calls the checkout's method.  ``AudioAttack.stage_1`` itself stays the checkout's.
"""
import importlib.util
import os
import sys

from audiopure_amd import attacks as _attacks
from audiopure_amd.robustness_eval import psychoacoustic as _psy

_HERE = os.path.dirname(os.path.abspath(__file__))
_NAME = "robustness_eval._checkout_white_box_attack"


def _checkout_module():
    if _NAME in sys.modules:
        return sys.modules[_NAME]
    pkg = sys.modules[__name__.rpartition(".")[0]]
    for d in pkg.__path__:
        f = os.path.join(d, "white_box_attack.py")
        if os.path.abspath(d) != _HERE and os.path.isfile(f):
            spec = importlib.util.spec_from_file_location(_NAME, f)
            mod = importlib.util.module_from_spec(spec)
            sys.modules[_NAME] = mod
            try:
                spec.loader.exec_module(mod)
            except BaseException:
                del sys.modules[_NAME]
                raise
            return mod
    raise ImportError(
        "robustness_eval.white_box_attack: no robustness_eval/white_box_attack.py of a reference checkout on the package path "
        f"(searched {list(pkg.__path__)}); put the checkout on sys.path, or use the native masker and hinge loss directly "
        "from audiopure_amd.robustness_eval.psychoacoustic")


_ref = _checkout_module()
globals().update({k: v for k, v in vars(_ref).items() if not k.startswith("__")})

PsychoacousticMasker = _psy.PsychoacousticMasker


class AudioAttack(_ref.AudioAttack):
    """The checkout's ``AudioAttack`` with the stage-2 threshold and hinge-loss hooks on the device."""

    def _stabilized_threshold_and_psd_maximum(self, x):
        return self.masker.threshold_and_psd_maximum(x)

    def _loss_gradient_masking_threshold(self, perturbation, x, masking_threshold_stabilized, psd_maximum_stabilized):
        return _psy.masking_threshold_loss_and_grad(perturbation, masking_threshold_stabilized, psd_maximum_stabilized,
                                                    hop_size=self.masker.hop_size)


class NativeStage1AudioAttack(AudioAttack):
    """``AudioAttack`` with stage 1's loop bookkeeping on the device too, where ``audiopure_amd.attacks.stage_1`` serves the call."""

    def stage_1(self, x, y):
        if _attacks.stage_1_served(self, x, y):
            return _attacks.stage_1(self, x, y)
        return super().stage_1(x, y)
