"""Device-side classifier front-end transforms."""
from .melspec import MelSpecDB, MelSpecDBHTK, ToMelSpectrogramDB  # noqa: F401
from .augment import AugmentDraws, SpeechCommandsAugment, draw_augment  # noqa: F401
from .defenses import AS, AT, BPF, DS, LPF, MS, FreqDomainDefense, TimeDomainDefense  # noqa: F401
