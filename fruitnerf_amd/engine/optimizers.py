"""The fused Adam / RAdam step as a `torch.optim.Optimizer`, and stand-ins for Nerfstudio's optimiser plumbing.

An unmodified Nerfstudio Trainer builds one optimiser per parameter group from `config.setup(params)`, steps it
through `GradScaler.step(optimizer)` (the method configs set mixed_precision=True), drives its learning rate with a
`torch.optim.lr_scheduler` and checkpoints `optimizer.state_dict()`.  `ArenaAdam` is that optimiser for this package:

  * parameters that live in a `ParamArena` are stepped through spans of the arena — contiguous parameters of one
    param group are ONE span, a group is one launch of `fnr_adam_step_spans_dev` — with flat moment buffers parallel
    to the span; any other contiguous fp32 device parameter (Nerfstudio's camera pose table) gets a launch of its own;
  * `_step_supports_amp_scaling`: `GradScaler.step` hands the loss scale and its inf flag over as device tensors and the
    kernel unscales / skips on the device.  The step path reads no device value on the host;
  * zeroing the gradients is fused into the step, and `zero_grad()` never detaches an arena parameter's `.grad` from the
    gradient arena (the backward kernels hold raw pointers into it);
  * arena gradients are always attached, so "this group received no gradient" is read from `ParamArena.grad_marks`
    instead of `.grad is None`: an optimiser none of whose arena groups was written since its last step does nothing,
    as `torch.optim` does for parameters without a gradient (the proposal networks on the iterations that evaluate them
    under no_grad);
  * `state_dict()` / `load_state_dict()` use `torch.optim.Adam`'s / `RAdam`'s layout, in both directions.

There is no CPU path: a parameter that is not a contiguous fp32 tensor on a HIP device makes `step()` raise.

`Optimizers`, `FusedAdamOptimizerConfig`, `FusedRAdamOptimizerConfig` mirror `nerfstudio.engine.optimizers` (0.3.2) so
that the path can be driven and tested without Nerfstudio; the real `Optimizers` needs only `setup`, `lr` and `max_norm`
of the configs.
"""
from __future__ import annotations

import weakref
from dataclasses import dataclass
from typing import Any, ClassVar, Dict, List, Optional

import torch
from torch import Tensor

from .. import _kernels as K
from .. import _lib as L
from ..params import arena_of

_ALGORITHMS = {"adam": torch.optim.Adam, "radam": torch.optim.RAdam}
_torch_defaults: Dict[str, dict] = {}
# one launch covers at most this many floats of gap between its spans (its moment buffers span the gaps too)
_MAX_GAP_FLOATS = 1 << 20


def _defaults_of(algorithm: str) -> dict:
    """The param-group keys (and default values) this build's torch.optim.Adam / RAdam emit: a checkpoint written here
    must carry the keys theirs expects."""
    if algorithm not in _torch_defaults:
        probe = _ALGORITHMS[algorithm]([torch.zeros(1, requires_grad=True)])
        _torch_defaults[algorithm] = dict(probe.defaults)
    return dict(_torch_defaults[algorithm])


class _Unit:
    """One launch of fnr_adam_step_spans_dev: spans of one arena that belong to one param group, or one free parameter."""

    def __init__(self, group_index: int, arena, members, device):
        # members: [(param, offset, numel)] sorted by offset (a free parameter: one member at offset 0)
        self.gi, self.arena, self.device = group_index, arena, device
        self.spans: List[List[int]] = []          # [begin, end) in arena elements, ends padded to 4
        self.members = []                         # (param, span index, offset, numel)
        for p, o, n in members:
            end = o + (n + 3) // 4 * 4
            if self.spans and self.spans[-1][1] == o:
                self.spans[-1][1] = end
            else:
                self.spans.append([o, end])
            self.members.append((p, len(self.spans) - 1, o, n))
        self.lo, self.hi = self.spans[0][0], self.spans[-1][1]
        self.ptrs = [p.data_ptr() for p, _, _, _ in self.members]
        self.exp_avg = torch.zeros(self.hi - self.lo, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(self.hi - self.lo, dtype=torch.float32, device=device)
        self.scalars = torch.zeros(L.FNR_ADAM_DEV_SCALAR_FLOATS, dtype=torch.float32, device=device)
        self.steps: Optional[Tensor] = None       # int64 [n spans], device
        if arena is not None:
            self.params_view, self.grads_view = arena.params[self.lo:self.hi], arena.grads[self.lo:self.hi]
            # the arena groups whose "received gradient" marks decide whether this launch has anything to do
            self.mark_names = tuple(sorted(g for g, (a, b) in arena.group_ranges.items()
                                           if any(a <= o < b for _, _, o, _ in self.members)))
        else:
            n = self.members[0][3]
            self.stage = None
            if n % 4 != 0:                        # the kernel works on float4 chunks: step a padded copy
                self.stage = torch.zeros(2, self.hi, dtype=torch.float32, device=device)

    def moment_views(self, member):
        p, _, o, n = member
        a = o - self.lo
        return self.exp_avg[a:a + n].view(p.shape), self.exp_avg_sq[a:a + n].view(p.shape)


class ArenaAdam(torch.optim.Optimizer):
    """torch.optim.Adam / RAdam (algorithm "adam" / "radam"; no amsgrad, L2 weight decay) on the fused HIP step."""

    _step_supports_amp_scaling = True     # GradScaler.step sets self.grad_scale / self.found_inf (device tensors)

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 algorithm: str = "adam"):
        if algorithm not in _ALGORITHMS:
            raise ValueError(f"unknown optimiser algorithm {algorithm!r}")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid hyper-parameters: lr {lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        self.algorithm = algorithm
        defaults = _defaults_of(algorithm)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self._plan: Optional[List[_Unit]] = None
        # arena -> {group: the ParamArena.grad_marks count this optimiser has consumed}; an arena starts at 0 = "no
        # backward yet", and so does this
        self._seen: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()
        super().__init__(params, defaults)

    def __getstate__(self) -> dict:
        self._refresh_steps()
        state = super().__getstate__()
        state["algorithm"] = self.algorithm
        return state

    def __setstate__(self, state: dict) -> None:
        super().__setstate__(state)
        self.__dict__.setdefault("_plan", None)   # (unpickled: the state is placed again at the next step)
        self.__dict__.setdefault("_seen", weakref.WeakKeyDictionary())

    def _fresh_gradients(self, plan) -> Dict[int, bool]:
        """id(unit) -> "a backward has written this launch's gradient spans since this optimiser last consumed them";
        consumes the marks of every arena group the plan covers."""
        fresh: Dict[int, bool] = {}
        taken = []
        for u in plan:
            if u.arena is None:
                continue
            seen, marks = self._seen.setdefault(u.arena, {}), u.arena.grad_marks
            fresh[id(u)] = any(seen.get(g, 0) != marks[g] for g in u.mark_names)
            taken.append((seen, marks, u.mark_names))
        for seen, marks, names in taken:          # (after the loop: several launches may share a group)
            for g in names:
                seen[g] = marks[g]
        return fresh

    # ---- launch plan -----------------------------------------------------------------------------------------------
    def _plan_is_current(self) -> bool:
        if self._plan is None:
            return False
        for u in self._plan:
            for (p, _, _, _), ptr in zip(u.members, u.ptrs):
                if p.data_ptr() != ptr:          # re-homed into an arena, or moved by module.to(...)
                    return False
        return True

    def _make_plan(self) -> List[_Unit]:
        """Resolve every parameter (lazily, at the first step: a Trainer builds its optimisers before the model's arena
        exists) and place the optimiser state — loaded, carried over from the previous plan, or zero — in flat buffers."""
        if self._plan is not None:
            self._refresh_steps()                 # the old counters -> state[p]["step"], before they are replaced
        plan: List[_Unit] = []
        for gi, group in enumerate(self.param_groups):
            by_arena: Dict[tuple, list] = {}
            for p in group["params"]:
                if not p.is_cuda:
                    raise RuntimeError(f"ArenaAdam: a parameter of shape {tuple(p.shape)} is on {p.device}; it steps "
                                       "only parameters on a HIP device (no CPU path)")
                if p.dtype != torch.float32 or not p.is_contiguous() or p.layout != torch.strided:
                    raise RuntimeError(f"ArenaAdam: a parameter of shape {tuple(p.shape)} is {p.dtype}, "
                                       f"contiguous={p.is_contiguous()}; it steps contiguous fp32 tensors only")
                if p.numel() == 0:
                    continue
                slot = arena_of(p)
                if slot is None:
                    plan.append(_Unit(gi, None, [(p, 0, p.numel())], p.device))
                else:
                    arena, gname, o, n = slot   # (per arena group: a launch steps or rests with its group's mark)
                    by_arena.setdefault((id(arena), gname), [arena, []])[1].append((p, o, n))
            for arena, members in by_arena.values():
                members.sort(key=lambda m: m[1])
                run: list = []
                n_spans = 0
                for m in members:
                    end = run[-1][1] + (run[-1][2] + 3) // 4 * 4 if run else None
                    new_span = end is None or end != m[1]
                    if run and new_span and (n_spans == L.FNR_MAX_ADAM_SPANS or m[1] - end > _MAX_GAP_FLOATS):
                        plan.append(_Unit(gi, arena, run, arena.params.device))
                        run, n_spans = [], 0
                    n_spans += 1 if new_span else 0
                    run.append(m)
                if run:
                    plan.append(_Unit(gi, arena, run, arena.params.device))
        for u in plan:
            span_step: List[Optional[int]] = [None] * len(u.spans)
            for member in u.members:
                p, k = member[0], member[1]
                m, v = u.moment_views(member)
                st = self.state.get(p)
                step = 0
                if st:
                    step = int(round(float(st["step"]))) if "step" in st else 0
                    if "exp_avg" in st:
                        m.copy_(st["exp_avg"].reshape(p.shape))
                        v.copy_(st["exp_avg_sq"].reshape(p.shape))
                if span_step[k] is not None and span_step[k] != step:
                    raise ValueError(f"ArenaAdam: the parameters of one span share one step counter, but the state holds "
                                     f"step {span_step[k]} and step {step} for them")
                span_step[k] = step
                self.state[p] = {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
            if any(span_step):
                u.steps = torch.tensor(span_step, dtype=torch.int64).to(u.device)
            else:
                u.steps = torch.zeros(len(u.spans), dtype=torch.int64, device=u.device)
        self._plan = plan
        return plan

    def _refresh_steps(self) -> None:
        """Device counters -> state[p]["step"] (synchronises)."""
        for u in self._plan or ():
            steps = u.steps.tolist()
            for p, k, _, _ in u.members:
                if p in self.state:
                    self.state[p]["step"] = torch.tensor(float(steps[k]), dtype=torch.float32)

    # ---- torch.optim.Optimizer -------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._plan if self._plan_is_current() else self._make_plan()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        grad_scale = grad_scale if isinstance(grad_scale, Tensor) else None     # (absent, or None after unscale_())
        found_inf = found_inf if isinstance(found_inf, Tensor) else None
        fresh = self._fresh_gradients(plan)
        for u in plan:
            group = self.param_groups[u.gi]
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay") or \
                    group.get("differentiable"):
                raise RuntimeError("ArenaAdam: amsgrad, maximize, decoupled_weight_decay and differentiable are not built")
            lr, (b1, b2) = group["lr"], group["betas"]
            if isinstance(lr, Tensor):
                raise RuntimeError("ArenaAdam: a tensor learning rate would have to be read on the host; pass a float")
            if u.arena is not None:
                if not fresh[id(u)]:              # no backward wrote these gradients since the last step: .grad is None
                    continue
                params, grads = u.params_view, u.grads_view
            else:
                p = u.members[0][0]
                g = p.grad
                if g is None:
                    continue
                if not g.is_cuda or g.dtype != torch.float32 or g.layout != torch.strided or not g.is_contiguous():
                    raise RuntimeError(f"ArenaAdam: the gradient of a parameter of shape {tuple(p.shape)} is not a "
                                       "contiguous fp32 tensor on the HIP device (no CPU path, no sparse gradients)")
                params, grads = p.data.view(-1), g.view(-1)
                if u.stage is None and (params.data_ptr() % 16 or grads.data_ptr() % 16):
                    u.stage = torch.zeros(2, u.hi, dtype=torch.float32, device=u.device)
                if u.stage is not None:
                    n = params.numel()
                    u.stage[0, :n].copy_(params)
                    u.stage[1, :n].copy_(grads)
                    params, grads = u.stage[0], u.stage[1]
            K.adam_step_spans_dev(params, grads, u.exp_avg, u.exp_avg_sq,
                                  [(a - u.lo, b - a, lr) for a, b in u.spans], u.steps, self.algorithm, b1, b2,
                                  group["eps"], u.scalars, grad_scale=grad_scale, found_inf=found_inf, zero_grad=True,
                                  weight_decay=group["weight_decay"])
            if u.arena is None and u.stage is not None:
                n = p.numel()
                p.data.view(-1).copy_(u.stage[0, :n])
                g.view(-1).zero_()
        return loss

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Arena parameters keep their `.grad` (a view of the gradient arena the kernels write through raw pointers);
        their spans are zero after every step, and are zeroed here only when a backward has written them since.  Other
        parameters: torch.optim's behaviour."""
        if self._plan_is_current():
            fresh = self._fresh_gradients(self._plan)
            for u in self._plan:
                if u.arena is not None:
                    if fresh[id(u)]:
                        for a, b in u.spans:
                            u.arena.grads[a:b].zero_()
                else:
                    self._zero_free(u.members[0][0], set_to_none)
            return
        for group in self.param_groups:
            for p in group["params"]:
                slot = arena_of(p)
                if slot is None:
                    self._zero_free(p, set_to_none)
                else:
                    arena, _, o, n = slot
                    arena.grads[o:o + n].zero_()
                    if p.grad is None or p.grad.data_ptr() != arena.grads.data_ptr() + 4 * o:
                        p.grad = arena.grads[o:o + n].view(p.shape)

    @staticmethod
    def _zero_free(p, set_to_none: bool) -> None:
        if p.grad is not None:
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.requires_grad_(False)
                p.grad.zero_()

    def state_dict(self) -> dict:
        """torch.optim.Adam's / RAdam's layout: state[i] = {"step" (float32 scalar), "exp_avg", "exp_avg_sq"} with the
        parameters' shapes (views of the flat moment buffers).  Reads the step counters from the device."""
        self._refresh_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict: dict) -> None:
        """Accepts a torch.optim.Adam / RAdam (or ArenaAdam) checkpoint, also before the parameters have found their
        arena: the state is held per parameter and placed in the flat buffers at the next step.  Parameters that share a
        span share its step counter — their `step` values must agree (checked when the state is placed)."""
        self._plan = None                         # (nothing of the old plan survives: no counters to carry over)
        super().load_state_dict(state_dict)


# ---- stand-ins for nerfstudio.engine.optimizers ---------------------------------------------------------------------


@dataclass
class FusedAdamOptimizerConfig:
    """nerfstudio AdamOptimizerConfig whose setup() builds ArenaAdam."""
    lr: float = 0.0005
    eps: float = 1e-08
    max_norm: Optional[float] = None
    weight_decay: float = 0
    algorithm: ClassVar[str] = "adam"

    def setup(self, params) -> ArenaAdam:
        return ArenaAdam(params, lr=self.lr, eps=self.eps, weight_decay=self.weight_decay, algorithm=self.algorithm)


@dataclass
class FusedRAdamOptimizerConfig(FusedAdamOptimizerConfig):
    """nerfstudio RAdamOptimizerConfig whose setup() builds ArenaAdam(algorithm="radam")."""
    algorithm: ClassVar[str] = "radam"


class Optimizers:
    """nerfstudio.engine.optimizers.Optimizers (0.3.2): one optimiser (+ optional scheduler) per parameter group.
    config = {group: {"optimizer": cfg, "scheduler": cfg | None}}, param_groups = model.get_param_groups()."""

    def __init__(self, config: Dict[str, Any], param_groups: Dict[str, List[torch.nn.Parameter]]) -> None:
        self.config = config
        self.optimizers: Dict[str, torch.optim.Optimizer] = {}
        self.schedulers: Dict[str, Any] = {}
        self.parameters: Dict[str, List[torch.nn.Parameter]] = {}
        for name, params in param_groups.items():
            lr_init = config[name]["optimizer"].lr
            self.optimizers[name] = config[name]["optimizer"].setup(params=params)
            self.parameters[name] = params
            sched = config[name].get("scheduler")
            if sched:
                sched = sched.setup() if hasattr(sched, "setup") else sched
                self.schedulers[name] = sched.get_scheduler(optimizer=self.optimizers[name], lr_init=lr_init)

    def optimizer_step(self, param_group_name: str) -> None:
        self.optimizers[param_group_name].step()

    def scheduler_step(self, param_group_name: str) -> None:
        if param_group_name in self.schedulers:
            self.schedulers[param_group_name].step()

    def zero_grad_all(self) -> None:
        for optimizer in self.optimizers.values():
            optimizer.zero_grad()

    def optimizer_scaler_step_all(self, grad_scaler) -> None:
        for name, optimizer in self.optimizers.items():
            max_norm = self.config[name]["optimizer"].max_norm
            if max_norm is not None:
                grad_scaler.unscale_(optimizer)
                torch.nn.utils.clip_grad_norm_(self.parameters[name], max_norm)
            if any(p.grad is not None for p in self.parameters[name]):
                grad_scaler.step(optimizer)

    def optimizer_step_all(self) -> None:
        for name, optimizer in self.optimizers.items():
            max_norm = self.config[name]["optimizer"].max_norm
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(self.parameters[name], max_norm)
            optimizer.step()

    def scheduler_step_all(self, step: int) -> None:
        for scheduler in self.schedulers.values():
            scheduler.step()

    def load_optimizers(self, loaded_state: Dict[str, Any]) -> None:
        for name, state in loaded_state.items():
            self.optimizers[name].load_state_dict(state)

    def load_schedulers(self, loaded_state: Dict[str, Any]) -> None:
        for name, state in loaded_state.items():
            self.schedulers[name].load_state_dict(state)
