"""Counterparts of nerfstudio.engine: training callbacks, optimisers and schedulers.  Nothing is imported eagerly — the
optimisers load the HIP library's bindings."""

__all__ = ["ArenaAdam", "FusedAdamOptimizerConfig", "FusedRAdamOptimizerConfig", "Optimizers",
           "ExponentialDecaySchedulerConfig"]


def __getattr__(name: str):   # PEP 562
    if name in ("ArenaAdam", "FusedAdamOptimizerConfig", "FusedRAdamOptimizerConfig", "Optimizers"):
        from . import optimizers
        return getattr(optimizers, name)
    if name == "ExponentialDecaySchedulerConfig":
        from .schedulers import ExponentialDecaySchedulerConfig
        return ExponentialDecaySchedulerConfig
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
