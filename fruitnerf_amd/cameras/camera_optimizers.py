"""nerfstudio.cameras.camera_optimizers (0.3.2) as used by the reference's datamanager
(/root/reference/fruit_nerf/fruit_nerf_config.py:39-43: CameraOptimizerConfig(mode="SO3xR3",
optimizer=AdamOptimizerConfig(lr=6e-4, eps=1e-8, weight_decay=1e-2), scheduler=ExponentialDecay(lr_final=6e-6,
max_steps=200000))): a learnable [num_cameras, 6] tangent vector per training camera, applied to the camera-to-world
matrices before ray generation and trained from the ray gradients of the hot path.  The arithmetic runs in
libfruitnerf_hip.so (camera_opt.hip); there is no CPU path."""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor, nn

from .. import _kernels as K
from .. import _lib as L


_SERIALS = itertools.count(1)   # CameraAdam.serial


def _padded_rows(num_cameras: int, device) -> Tensor:
    """Zeros [num_cameras, 6] at the start of a storage padded to a multiple of 4 floats: the optimiser kernel of
    CameraAdam.step() works on float4 chunks, and an odd camera count ends in the middle of one."""
    n = 6 * num_cameras
    return torch.zeros((n + 3) // 4 * 4, device=device)[:n].view(num_cameras, 6)


def _padded_flat(rows: Tensor) -> Tensor:
    """The whole padded storage of a _padded_rows() tensor, flat (its padding lanes included)."""
    n = (rows.numel() + 3) // 4 * 4
    if n == rows.numel() and rows.is_contiguous():
        return rows.view(-1)
    if not rows.is_contiguous() or rows.untyped_storage().nbytes() < 4 * (rows.storage_offset() + n):
        raise RuntimeError("the pose table, its .grad or a moment was replaced by a tensor without the padding to a multiple "
                           "of 4 floats (copy into the tensors CameraOptimizer / CameraAdam allocated instead)")
    return rows.as_strided((n,), (1,), rows.storage_offset())


@dataclass
class CameraOptimizerConfig:
    mode: str = "off"                      # "off" | "SO3xR3" | "SE3"  (nerfstudio's three values)
    position_noise_std: float = 0.0        # nerfstudio fields kept for config compatibility; noise is not built
    orientation_noise_std: float = 0.0
    lr: float = 6e-4                       # AdamOptimizerConfig(lr=6e-4, eps=1e-8, weight_decay=1e-2)
    eps: float = 1e-8
    weight_decay: float = 1e-2
    lr_final: Optional[float] = 6e-6       # ExponentialDecaySchedulerConfig(lr_final=6e-6, max_steps=200000)
    max_steps: int = 200000
    param_group: str = "camera_opt"

    def setup(self, num_cameras: int, device) -> "CameraOptimizer":
        return CameraOptimizer(self, num_cameras, device)


class CameraOptimizer(nn.Module):
    """Layer that modifies camera poses to be optimized (nerfstudio CameraOptimizer)."""

    def __init__(self, config: CameraOptimizerConfig, num_cameras: int, device) -> None:
        super().__init__()
        if config.mode != "off" and config.mode not in L.POSE_MODES:
            raise ValueError(f"camera optimizer mode {config.mode!r} (off | SO3xR3 | SE3)")
        if config.position_noise_std != 0.0 or config.orientation_noise_std != 0.0:
            raise NotImplementedError("pose noise is not built")
        self.config = config
        self.num_cameras = num_cameras
        self.device = torch.device(device)
        # the exponential map of the pose rows: pose_mode of the fnr_*_mode entry points
        self.pose_mode = L.POSE_MODES.get(config.mode, L.FNR_POSE_SO3XR3)
        if config.mode != "off":
            # [num_cameras, 6] views of storages padded to a multiple of 4 floats for the float4 optimiser kernel (540
            # floats for 90 cameras already are); the padding lanes are zero and stay zero (p = g = 0 under L2 decay)
            self.pose_adjustment = nn.Parameter(_padded_rows(num_cameras, self.device))
            self.pose_adjustment.grad = _padded_rows(num_cameras, self.device)
        self._identity = None

    @property
    def enabled(self) -> bool:
        return self.config.mode != "off"

    def forward(self, indices: Tensor) -> Tensor:
        """[N,3,4] camera-to-camera corrections exp_map_SO3xR3 | exp_map_SE3 (pose_adjustment[indices]) (identity when
        off)."""
        n = indices.shape[0]
        if not self.enabled:
            return torch.eye(4, device=self.device)[None, :3, :4].tile(n, 1, 1)
        if self._identity is None:
            eye = torch.eye(4, device=self.device)[None, :3, :4].tile(self.num_cameras, 1, 1).contiguous()
            self._identity = K.ImageSetArg(torch.zeros(1, 1, 1, 3, dtype=torch.uint8, device=self.device),
                                           torch.zeros(1, 1, 1, dtype=torch.uint8, device=self.device), eye, 1, 1, 0, 0)
            self._all = torch.arange(self.num_cameras, device=self.device)
        return K.camera_adjust(self._identity, self._all, self.pose_adjustment.data, pose_mode=self.pose_mode)[indices.long()]

    def adjusted_cameras(self, image_set: "K.ImageSetArg", train_ids: Tensor) -> Optional[Tensor]:
        """c2w' [n_train,3,4] = pose_utils.multiply(c2w[train_ids], forward(arange(n_train))); None when off."""
        if not self.enabled:
            return None
        return K.camera_adjust(image_set, train_ids, self.pose_adjustment.data, pose_mode=self.pose_mode)

    def get_metrics_dict(self) -> dict:
        """nerfstudio's camera_opt_translation / camera_opt_rotation (fruit_pipeline.py:133-142): the norms of the two
        halves of the pose table, as device scalars; {} when off."""
        if not self.enabled:
            return {}
        pose = self.pose_adjustment.data
        return {"camera_opt_translation": pose[:, :3].norm(), "camera_opt_rotation": pose[:, 3:].norm()}

    def get_param_groups(self) -> dict:
        return {self.config.param_group: list(self.parameters())} if self.enabled else {}


class CameraAdam:
    """The camera optimiser's torch.optim.Adam(lr, eps, weight_decay) + ExponentialDecay schedule as one fused launch
    (same kernel as the model's optimiser: fnr_adam_step with the L2 weight_decay term)."""

    def __init__(self, camera_optimizer: CameraOptimizer, betas=(0.9, 0.999), algorithm: str = "adam"):
        # algorithm="radam": the big/huge configs' camera optimiser (RAdamOptimizerConfig(lr=6e-4, eps=1e-8,
        # weight_decay=1e-3), fruit_nerf_config.py:77-80,125-128)
        if algorithm not in ("adam", "radam"):
            raise ValueError(f"unknown optimiser algorithm {algorithm!r}")
        self.algorithm = algorithm
        self.opt = camera_optimizer
        self.cfg = camera_optimizer.config
        self.betas = betas
        self.step_count = 0
        p = camera_optimizer.pose_adjustment
        self.exp_avg = _padded_rows(p.shape[0], p.device)     # padded like the table: step() runs on the whole storages
        self.exp_avg_sq = _padded_rows(p.shape[0], p.device)
        self.serial = next(_SERIALS)                          # never reused, unlike id()

    def program_fingerprint(self) -> tuple:
        """Everything a recorded step program (training.TrainingSteps) captures from this object and its CameraOptimizer by
        value, the per-step scalars (learning rate, step count) aside: which optimiser this is, the addresses of the pose
        table, its gradient and the two moments, and the hyper-parameters.  Host-only; in-place edits leave it alone."""
        c = self.cfg
        p = self.opt.pose_adjustment
        return (self.serial, p.data_ptr(), None if p.grad is None else p.grad.data_ptr(), self.exp_avg.data_ptr(),
                self.exp_avg_sq.data_ptr(), self.betas[0], self.betas[1], c.eps, c.weight_decay, self.algorithm)

    def fused_step_args(self, grad_scale: float = 1.0):
        """Advance the step count and return the fnr_table_adam of THIS update for a kernel that applies it itself
        (fnr_camera_pose_grad_adam) — same learning rate / step as step() would use."""
        from ..training import exponential_decay_lr
        from .. import _lib as L
        lr, step = self.advance()
        c = self.cfg
        p = self.opt.pose_adjustment
        return L.table_adam(0 if self.algorithm == "adam" else 1, lr, self.betas[0], self.betas[1], c.eps,
                            step, grad_scale, c.weight_decay, L.ptr(p.data), L.ptr(self.exp_avg),
                            L.ptr(self.exp_avg_sq), None, slot=L.ADAM_SLOTS["camera_opt"])

    def advance(self):
        """Count one optimiser step -> (its learning rate, its 1-based step number): the host bookkeeping of
        fused_step_args() (a replayed step program patches these two into the recorded call)."""
        from ..training import exponential_decay_lr
        self.step_count += 1
        c = self.cfg
        lr = c.lr if c.lr_final is None else exponential_decay_lr(self.step_count - 1, c.lr, c.lr_final, c.max_steps)
        return lr, self.step_count

    def step(self, grad_scale: float = 1.0) -> None:
        from ..training import exponential_decay_lr
        self.step_count += 1
        c = self.cfg
        lr = c.lr if c.lr_final is None else exponential_decay_lr(self.step_count - 1, c.lr, c.lr_final, c.max_steps)
        p = self.opt.pose_adjustment
        fn = K.adam_step if self.algorithm == "adam" else K.radam_step
        fn(_padded_flat(p.data), _padded_flat(p.grad), _padded_flat(self.exp_avg), _padded_flat(self.exp_avg_sq), lr,
           self.betas[0], self.betas[1], c.eps, self.step_count, grad_scale, True, weight_decay=c.weight_decay)
