"""Stand-in for nerfstudio.engine.schedulers: the one scheduler the method configs use."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
from torch.optim import Optimizer, lr_scheduler


@dataclass
class ExponentialDecaySchedulerConfig:
    """nerfstudio ExponentialDecaySchedulerConfig without warm-up (fruit_nerf_config.py:49,53): log-linear decay from the
    optimiser's initial learning rate to `lr_final` over `max_steps`, constant afterwards.  `setup()` returns the object
    that answers `get_scheduler`, as Nerfstudio's config does — here the config itself."""
    lr_final: Optional[float] = None
    max_steps: int = 100000

    def setup(self) -> "ExponentialDecaySchedulerConfig":
        return self

    def get_scheduler(self, optimizer: Optimizer, lr_init: float) -> lr_scheduler.LambdaLR:
        lr_final = lr_init if self.lr_final is None else self.lr_final
        max_steps = self.max_steps

        def factor(step: int) -> float:      # training.exponential_decay_lr(step, ...) / lr_init
            t = float(np.clip(step / max_steps, 0, 1))
            return float(np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)) / lr_init

        return lr_scheduler.LambdaLR(optimizer, lr_lambda=factor)
