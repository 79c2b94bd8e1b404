"""Shared body of the ZeRO-1 / ZeRO-2 ``ShardedOptimizer`` drop-ins.

The public surface is the reference's: ``ShardedOptimizer(optimizer)``,
``.step(closure=None)``, ``.zero_grad()``, attributes ``optimizer``, ``original_param_groups``,
``params``, ``local_param_indices``, ``local_params``, ``step_time``, ``communication_time``,
``broadcast_count``; the inner optimizer's ``param_groups`` are filtered to the owned parameters
(zero1.py:71-74) and ``optimizer.state[p]`` holds ``step`` / ``exp_avg`` / ``exp_avg_sq`` for
every owned parameter (read by memory.py:15-24); with a ``torch.optim.SGD`` it holds
``momentum_buffer`` once the parameter has stepped, as torch's does.  Everything below ``step()`` is the native
engine (engine.py → libzero_amd.so); the inner torch optimizer's own ``step`` is never called.
"""
from __future__ import annotations

import contextlib
import time
import weakref

import torch
import torch.distributed as dist
from torch.optim import Optimizer

from . import checkpoint as ckpt
from ._hooks import on_param_device
from ._update import (check_bf16_state_group, check_bf16_state_lion_group, check_ema, check_ema_decay, check_ema_group,
                      check_max_grad_norm, check_param_grad_norms, check_update_norms,
                      check_update_norms_group,
                      check_skip_nonfinite, check_master_free, check_master_free_group,
                      check_state_dtype, check_state_rounding, owner_range, KIND_NAMES)
from .engine import ShardEngine
from .training_utils.utils import get


def adam_group_hparams(group: dict, optimizer: Optimizer) -> dict:
    """Hyper-parameters of one torch.optim.Adam / AdamW param group (adam.py:38-90)."""
    lr = group["lr"]
    lr = float(lr.item()) if torch.is_tensor(lr) else float(lr)
    beta1, beta2 = group["betas"]
    decoupled = bool(group.get("decoupled_weight_decay", False)) or isinstance(
        optimizer, torch.optim.AdamW)
    return dict(lr=lr, beta1=float(beta1), beta2=float(beta2), eps=float(group["eps"]),
                weight_decay=float(group["weight_decay"]), amsgrad=bool(group.get("amsgrad", False)),
                maximize=bool(group.get("maximize", False)), decoupled=decoupled)


def sgd_group_hparams(group: dict) -> dict:
    """Hyper-parameters of one torch.optim.SGD param group (sgd.py SGD.__init__); ``foreach`` and
    ``fused`` only pick torch's implementation and are ignored, ``differentiable`` is refused."""
    if group.get("differentiable", False):
        raise ValueError("zero_amd: torch.optim.SGD(differentiable=True) is not supported (the "
                         "update runs in a HIP kernel outside autograd)")
    lr = group["lr"]
    lr = float(lr.item()) if torch.is_tensor(lr) else float(lr)
    return dict(lr=lr, momentum=float(group.get("momentum", 0.0)),
                dampening=float(group.get("dampening", 0.0)),
                weight_decay=float(group.get("weight_decay", 0.0)),
                nesterov=bool(group.get("nesterov", False)),
                maximize=bool(group.get("maximize", False)), amsgrad=False)


def lion_group_hparams(group: dict) -> dict:
    """Hyper-parameters of one zero_amd.optim.Lion param group."""
    lr = group["lr"]
    lr = float(lr.item()) if torch.is_tensor(lr) else float(lr)
    beta1, beta2 = group["betas"]
    return dict(lr=lr, beta1=float(beta1), beta2=float(beta2),
                weight_decay=float(group.get("weight_decay", 0.0)),
                maximize=bool(group.get("maximize", False)), amsgrad=False)


def group_hparams(kind: str, group: dict, optimizer: Optimizer) -> dict:
    """One param group's hyper-parameters for the ``kind`` ("adam" / "sgd" / "lion") update."""
    if kind == "lion":
        return lion_group_hparams(group)
    return sgd_group_hparams(group) if kind == "sgd" else adam_group_hparams(group, optimizer)


def optimizer_kind(optimizer: Optimizer) -> str:
    """"adam" (torch.optim.Adam / AdamW), "sgd" (torch.optim.SGD) or "lion"
    (zero_amd.optim.Lion); TypeError for anything else."""
    from .optim import Lion

    if isinstance(optimizer, torch.optim.Adam):
        return "adam"
    if isinstance(optimizer, torch.optim.SGD):
        return "sgd"
    if isinstance(optimizer, Lion):
        return "lion"
    raise TypeError("zero_amd ShardedOptimizer wraps torch.optim.Adam / AdamW / SGD or "
                    f"zero_amd.optim.Lion (got {type(optimizer).__name__})")


class ShardedOptimizerBase:
    """ZeRO-1/2 wrapper; subclasses set ``_carry`` (ZeRO-1 gradient carry) and ``_variant``."""

    _carry = False
    _variant = 2

    @on_param_device
    def __init__(self, optimizer: Optimizer, *, layout: str = "reference",
                 bucket_mb: float | None = None, comm=None, sync: bool = True, buckets: str = "ragged",
                 overlap: bool = False, overlap_bucket_mb: float = 64.0, master: str = "split",
                 arena: str = "flat", grad_comm: str | None = None,
                 max_grad_norm: float | None = None, state_dtype=None,
                 state_rounding: str | None = None, state_seed: int = 0,
                 skip_nonfinite: bool = False, param_grad_norms: bool = False,
                 ema_decay: float | None = None, param_update_norms: bool = False):
        if arena not in ("flat", "buckets", "auto"):
            raise ValueError(f"arena must be 'flat', 'buckets' or 'auto' (got {arena!r})")
        # the moments' dtype: None / torch.float32, or torch.bfloat16 (opt-in: exp_avg and
        # exp_avg_sq stored in bf16, the arithmetic in fp32 as before).  What it
        # cannot be combined with is refused below, on every rank and before anything collective
        self.state_dtype = check_state_dtype(state_dtype)
        bf16_state = self.state_dtype == torch.bfloat16
        # how bf16 moments are rounded when stored: None / "nearest", or "stochastic" (opt-in: the
        # fused update rounds them from a counter-based generator keyed by state_seed, the step
        # and the element's index in its shard, which lifts the bound on the betas)
        self.state_rounding, self.state_seed = check_state_rounding(state_rounding, state_seed,
                                                                    self.state_dtype)
        # global gradient-norm clipping inside step() (None = off); a plain attribute, it may be
        # changed between steps.  What it cannot be combined with is refused here, on every rank
        # and before anything collective
        self.max_grad_norm = max_grad_norm
        self.engine = None
        self._clip_unsupported = None
        if self._carry and get("ws") > 1:
            self._clip_unsupported = ("ZeRO-1 at world size > 1 (what the gradient carry should "
                                      "hold under clipping is undecided)")
        elif overlap:
            self._clip_unsupported = "overlap=True (the backward-overlapped reduction)"
        elif arena == "buckets":
            self._clip_unsupported = "arena='buckets' (the bucket arena)"
        elif layout != "reference" and (layout != "flat" or self._carry):
            self._clip_unsupported = f"layout={layout!r} (it runs on the bucket arena)"
        self._check_clip()
        self._kind = optimizer_kind(optimizer)
        # skip_nonfinite (with max_grad_norm; Adam): a step whose gradient norm is not finite is
        # skipped on the device — nothing in device memory changes, the host proceeds as for any
        # step; refused here, on every rank and before anything collective
        self.skip_nonfinite = check_skip_nonfinite(skip_nonfinite, max_grad_norm, self._kind)
        # param_grad_norms (with max_grad_norm): the norm pass also reports the L2 norm of every
        # parameter's averaged gradient, last_param_grad_norms; a reporting switch,
        # fixed at construction and not checkpointed
        self.param_grad_norms = check_param_grad_norms(param_grad_norms, max_grad_norm)
        # master="none": bf16 parameters without any master, updated in place and rounded
        # stochastically from the same generator (state_seed).  What it cannot be
        # combined with is refused here, on every rank and before anything collective
        if master not in ("split", "fp32", "none"):
            raise ValueError(f"master must be 'split', 'fp32' or 'none' (got {master!r})")
        master_free = master == "none"
        if master_free:
            check_master_free(self._kind, self._carry and get("ws") > 1,
                              all(p.dtype == torch.bfloat16 for g in optimizer.param_groups
                                  for p in g["params"]))
            if arena == "buckets" or overlap or \
                    (layout != "reference" and (layout != "flat" or self._carry)):
                raise ValueError("zero_amd: master='none' is not supported with the bucket arena "
                                 f"or overlap=True (arena={arena!r}, layout={layout!r}, "
                                 f"overlap={bool(overlap)}); use the flat arena")
        # ema_decay: an fp32 EMA of the master weights, sharded like exp_avg and updated inside
        # the fused Adam step ("Sharded EMA"); None: off.  What it cannot be combined
        # with is refused here, on every rank and before anything collective
        self._ema_decay = check_ema_decay(ema_decay)
        self._ema_swapped = False  # inside ema_parameters()
        has_ema = self._ema_decay is not None
        if has_ema:
            check_ema(self._kind, self._carry and get("ws") > 1, self.state_dtype, master)
            if arena == "buckets" or overlap or \
                    (layout != "reference" and (layout != "flat" or self._carry)):
                raise ValueError("zero_amd: ema_decay is not supported with the bucket arena or "
                                 f"overlap=True (arena={arena!r}, layout={layout!r}, "
                                 f"overlap={bool(overlap)}); use the flat arena")
        # param_update_norms: the fused update also reports the L2 norm of every parameter's
        # update and of its weights, on the fp32 master (last_param_update_norms,
        # last_param_weight_norms); a reporting switch, fixed at construction and not
        # checkpointed.  Refused here where it does not apply, before anything collective
        self.param_update_norms = bool(param_update_norms)
        if self.param_update_norms:
            check_update_norms(self._kind, self._carry and get("ws") > 1, self.state_dtype, master,
                               ema=has_ema)
            if arena == "buckets" or overlap or \
                    (layout != "reference" and (layout != "flat" or self._carry)):
                raise ValueError("zero_amd: param_update_norms is not supported with the bucket "
                                 f"arena or overlap=True (arena={arena!r}, layout={layout!r}, "
                                 f"overlap={bool(overlap)}); use the flat arena")
        for group in optimizer.param_groups:  # (what a group cannot ask for is refused here)
            hpd = group_hparams(self._kind, group, optimizer)
            if bf16_state and self._kind == "adam":
                check_bf16_state_group(hpd, self.state_rounding)
            if bf16_state and self._kind == "lion":
                check_bf16_state_lion_group(hpd, self.state_rounding)
            if master_free:
                check_master_free_group(hpd)
            if has_ema:
                check_ema_group(hpd)
            if self.param_update_norms:
                check_update_norms_group(hpd)
        if bf16_state:
            if self._kind == "sgd":
                raise ValueError("zero_amd: state_dtype=torch.bfloat16 is not supported with "
                                 "torch.optim.SGD (bf16 moments are Adam's)")
            if self._carry and get("ws") > 1:
                raise ValueError("zero_amd: state_dtype=torch.bfloat16 is not supported with "
                                 "ZeRO-1 at world size > 1 (the gradient carry stays fp32)")
            if arena == "buckets" or (layout != "reference" and (layout != "flat" or self._carry)):
                raise ValueError("zero_amd: state_dtype=torch.bfloat16 is not supported with the "
                                 f"bucket arena (arena={arena!r}, layout={layout!r}); use the "
                                 "flat arena")
        if self._kind in ("sgd", "lion"):
            # the SGD and Lion updates run on the flat arena (and its rounds) only
            name = KIND_NAMES[self._kind]
            if arena == "buckets":
                raise ValueError(f"zero_amd: {name} is not supported with arena='buckets' "
                                 "(the bucket arena); use the flat arena")
            if layout != "reference" and (layout != "flat" or self._carry):
                raise ValueError(f"zero_amd: {name} is not supported with layout={layout!r} "
                                 "(it runs on the bucket arena, arena='buckets')")
            arena = "flat"  # arena='auto' would time the bucket arena as a candidate
        self.optimizer = optimizer
        self.original_param_groups = optimizer.param_groups
        self.params = [p for group in self.original_param_groups for p in group["params"]]
        self._param_device = self.params[0].device if self.params else None  # (on_param_device)
        self._group_of = [gi for gi, group in enumerate(self.original_param_groups)
                          for _ in group["params"]]
        # references to the unfiltered groups' hyper-parameter dicts (lr schedulers mutate these)
        self._groups = list(self.original_param_groups)

        world_size = get("ws")
        rank = get("rank")
        # zero1.py:55-62 / zero2.py:51-58 (the planner computes the same ranges natively)
        self.local_param_indices = list(range(*owner_range(len(self.params), world_size, rank)))
        self.local_params = set(self.params[i] for i in self.local_param_indices)
        self._shard_optimizer_params()
        ckpt.bind_inner_load(self)  # opt.optimizer.load_state_dict fills the flat state

        self.broadcast_count = 0
        self.communication_time = 0.0
        self.step_time = 0.0
        self.world_size, self.rank = world_size, rank
        self._layout = layout
        self._buckets = buckets
        self._comm = comm
        self.arena_calibration = None
        if arena == "auto":
            # measured on this job's interconnect at construction (a collective call): the flat
            # arena's grouped reduce / broadcast against the bucket arena's reduce-scatter /
            # all-gather plus its pack / unpack copies (calibrate_arena)
            arena = "flat"
            if world_size > 1 and layout == "reference" and grad_comm is None:
                self.arena_calibration = calibrate_arena(self)
                arena = self.arena_calibration["chosen"]
                if arena == "buckets":  # (rank 0's choice, broadcast: every rank raises alike)
                    self._clip_unsupported = "arena='auto' that resolved to the bucket arena"
                    self._check_clip()
                    if bf16_state:
                        raise ValueError("zero_amd: state_dtype=torch.bfloat16 is not supported "
                                         "with arena='auto' that resolved to the bucket arena")
                    if master_free:
                        raise ValueError("zero_amd: master='none' is not supported with "
                                         "arena='auto' that resolved to the bucket arena")
                    if has_ema:
                        raise ValueError("zero_amd: ema_decay is not supported with "
                                         "arena='auto' that resolved to the bucket arena")
                    if self.param_update_norms:
                        raise ValueError("zero_amd: param_update_norms is not supported with "
                                         "arena='auto' that resolved to the bucket arena")
        # bytes per bucket (bucket arena) / per round (flat arena, all owners' windows together);
        # default 256 MiB / 1 GiB: a flat round has no pack to pipeline, so fewer, larger rounds
        # cost only the last round's Adam as exposed tail and cut the launches per step
        if bucket_mb is None:
            bucket_mb = 1024.0 if arena == "flat" else 256.0
        self._bucket_bytes = int(bucket_mb * (1 << 20))
        self._sync = sync
        # bf16 params: "split" (bf16 param + int16 residual), "fp32", or "none" (no master)
        self._master = master
        # ws > 1 exchange: "flat" = params and grads are views of one owner-major arena, rounds of
        # grouped reduce / broadcast, no pack / unpack (flat.py); "buckets" = the rank-major
        # bucket arena with pack / reduce-scatter / all-gather / unpack (engine.py)
        self._arena = arena
        # grad_comm="bf16": fp32 grads cross the interconnect as bf16 (flat
        # arena only); opt-in, since the sum is then rounded to bf16 before Adam sees it
        self._grad_comm = grad_comm
        if grad_comm is not None and arena != "flat":
            raise ValueError("grad_comm='bf16' needs the flat arena")
        self.engine: ShardEngine | None = None
        self._step_tensors = {}
        self._validated = [None] * len(self.params)
        self._overlap = bool(overlap)
        self._overlap_hooks = []
        if self._overlap:
            # hooks must exist before the first backward: build the engine (and the communicator,
            # a collective call every rank makes here) now.  Flat arena: per-owner reduces of G
            # stretches from the hooks (flat.py); bucket arena: GradBuckets views (overlap.py)
            self._build_engine()
            gb = self.engine.enable_overlap(int(overlap_bucket_mb * (1 << 20)))
            self._overlap_hooks = gb.register_hooks()
        elif self._flat():
            # params become views of the arena now, so zero_grad() can hand out grad views
            # before the first step (every rank builds it: the communicator is a collective)
            self._build_engine()
            self._overlap_hooks = self.engine.register_marks()

    @property
    def ema_decay(self):
        """The EMA's decay (None: the optimizer keeps no EMA): ``ema = lerp(ema, master, 1 - d)``
        after every update.  It may be changed between steps (a warm-up schedule) and is checked
        when set and at every step; whether there is an EMA is fixed at construction.  Not
        checkpointed."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, d):
        if (d is None) != (self._ema_decay is None):
            raise ValueError("zero_amd: whether the optimizer keeps an EMA is fixed at construction "
                             "(ShardedOptimizer(..., ema_decay=d))")
        self._ema_decay = check_ema_decay(d)

    def _check_not_swapped(self, what: str):
        if self._ema_swapped:
            raise RuntimeError(f"zero_amd: {what} inside ema_parameters(): the parameters hold the "
                               "EMA, not the weights training continues from")

    @contextlib.contextmanager
    def ema_parameters(self):
        """Inside the ``with`` block every rank's parameters hold the EMA rounded to the parameter
        dtype (to nearest even); on exit they are restored bit for bit.  Collective at world size
        > 1: each rank stashes its own window of the parameter arena (in the parameter dtype,
        freed on exit), writes its EMA there and the step's broadcast groups send every owner's
        window round; exit copies the stash back and broadcasts again.  ``step()``,
        ``state_dict()``, ``load_state_dict()`` and a nested entry raise RuntimeError inside."""
        if self._ema_decay is None:
            raise RuntimeError("zero_amd: ema_parameters() needs ShardedOptimizer(..., ema_decay=d)")
        self._check_not_swapped("ema_parameters()")
        with contextlib.ExitStack() as es:
            dev = self._param_device
            if dev is not None and dev.type == "cuda" and dev.index is not None:
                es.enter_context(torch.cuda.device(dev))
            if self.engine is None:
                self._build_engine()
            eng = self.engine
            stream = torch.cuda.current_stream(eng.device)
            win = eng.own_window()
            with torch.no_grad():
                stash = win.clone()
                if win.numel():
                    if win.dtype == torch.float32:
                        win.copy_(eng.ema)
                    else:
                        from .kernels import convert

                        convert(eng.ema, win, stream)
                eng.broadcast_params(stream)
            self._ema_swapped = True
            try:
                yield self
            finally:
                stream = torch.cuda.current_stream(eng.device)
                with torch.no_grad():
                    win.copy_(stash)
                    eng.broadcast_params(stream)
                self._ema_swapped = False
                del stash

    def _check_clip(self):
        """``max_grad_norm`` is None or a limit >= 0 (infinity: report the norm, clip nothing) on
        a configuration that supports clipping; ValueError otherwise."""
        m = self.max_grad_norm
        check_max_grad_norm(m)
        if m is None:
            if getattr(self, "skip_nonfinite", False):
                raise ValueError("zero_amd: skip_nonfinite=True needs max_grad_norm")
            check_param_grad_norms(getattr(self, "param_grad_norms", False), m)
            return
        if self._clip_unsupported is not None:
            raise ValueError("zero_amd: max_grad_norm is not supported with "
                             + self._clip_unsupported)

    @property
    def last_grad_norm(self):
        """0-d fp32 device tensor: the L2 norm of the averaged gradient the last clipped step
        saw (clip_grad_norm_'s return value); valid in stream order after step(), overwritten by
        the next step; None before the first clipped step."""
        out = None if self.engine is None else self.engine.clip_out
        return None if out is None else out[0]

    @property
    def last_clip_coef(self):
        """0-d fp32 device tensor: min(1, max_grad_norm / (last_grad_norm + 1e-6)), as above."""
        out = None if self.engine is None else self.engine.clip_out
        return None if out is None else out[1]

    @property
    def last_param_grad_norms(self):
        """1-D fp32 device tensor of ``len(params)`` (``param_grad_norms``): entry i is the L2 norm
        of parameter i's averaged gradient in the last clipped step, +0.0 for a parameter without
        a gradient; the same bits on every rank, valid in stream order after step(), overwritten
        (the same tensor) by the next step; None before the first such step and without the
        option."""
        clip = None if self.engine is None else self.engine.clip
        return None if clip is None else clip.param_norms

    @property
    def last_param_update_norms(self):
        """1-D fp32 device tensor of ``len(params)`` (``param_update_norms``): entry i is the L2
        norm of (fp32 master after - fp32 master before) of parameter i in the last step; +0.0 for
        a parameter that step did not update and for a step ``skip_nonfinite`` skipped; NaN before
        the first step.  The same bits on every rank, valid in stream order after step(),
        overwritten (the same tensor) by the next step; None without the option."""
        un = None if self.engine is None else getattr(self.engine, "stats", None)
        return None if un is None else un.update

    @property
    def last_param_weight_norms(self):
        """As ``last_param_update_norms``: entry i is the L2 norm of parameter i's fp32 master
        after the last step that updated it (a parameter not updated and a skipped step keep the
        entry); NaN until then."""
        un = None if self.engine is None else getattr(self.engine, "stats", None)
        return None if un is None else un.weight

    @property
    def last_norm_bytes(self) -> int:
        """Gradient bytes the last step's norm pass read (0 without clipping)."""
        return 0 if self.engine is None else self.engine.last_norm_bytes

    @property
    def skipped_steps(self):
        """0-d int64 device tensor (``skip_nonfinite``): the steps skipped so far for a non-finite
        gradient norm; valid in stream order after step(), not checkpointed; None before the
        first step and without ``skip_nonfinite``."""
        clip = None if self.engine is None else self.engine.clip
        return None if clip is None or clip.skipped is None else clip.skipped[0]

    def _flat(self) -> bool:
        """The flat parameter arena: the reference layout (the drop-in), or the balanced Layout F
        ablation for ZeRO-2 (the ZeRO-1 carry is per whole parameter: bucket arena there)."""
        return self._arena == "flat" and (self._layout == "reference" or
                                          (self._layout == "flat" and not self._carry))

    def _shard_optimizer_params(self):
        """zero1.py:71-74: drop non-owned params from the inner optimizer's groups."""
        for group in self.optimizer.param_groups:
            group["params"] = [p for p in group["params"] if p in self.local_params]

    # ------------------------------------------------------------------------------------------
    def _build_engine(self):
        comm = self._comm
        if self.world_size > 1 and comm is None:
            from .comm import RcclComm
            comm = RcclComm()
            self._comm = comm
        # ws=1 owns every param, so zero_grad clears them all and there is no carry
        # (zero1.py:107-108): no buffer, no 0·A term
        carry = self._carry and self.world_size > 1
        if self._flat():
            from .flat import FlatEngine

            self.engine = FlatEngine(self.params, self._group_of, self.world_size, self.rank,
                                     carry=carry, comm=comm, bucket_bytes=self._bucket_bytes,
                                     master=self._master, grad_comm=self._grad_comm,
                                     layout=self._layout, kind=self._kind,
                                     state_dtype=self.state_dtype,
                                     state_rounding=self.state_rounding,
                                     state_seed=self.state_seed,
                                     ema=self._ema_decay is not None,
                                     update_norms=self.param_update_norms,
                                     momentum=self._kind == "sgd" and any(
                                         g.get("momentum", 0) != 0 for g in self._groups))
        else:
            self.engine = ShardEngine(self.params, self._group_of, self.world_size, self.rank,
                                      layout=self._layout, carry=carry, comm=comm,
                                      bucket_bytes=self._bucket_bytes, buckets=self._buckets,
                                      master=self._master)
        if self.engine.plan.layout != 0:
            return
        self._expose_state()

    def _expose_state(self):
        """optimizer.state[p] = {'step', 'exp_avg', 'exp_avg_sq'} as views of the flat shard."""
        eng = self.engine
        if self._kind == "sgd":
            self._update_step_state()
            return
        for i in eng.owned_param_indices():
            views = eng.state_views(i)
            if views is not None:
                self.optimizer.state[self.params[i]].update(views)

    def _hparams_of(self, gi: int) -> dict:
        return group_hparams(self._kind, self._groups[gi], self.optimizer)

    def _update_step_state(self):
        eng = self.engine
        if self._kind == "sgd":
            eng.expose_sgd(self.optimizer, self.params, self._groups, eng.owned_param_indices(),
                           eng.state_views)
            return
        for i in eng.owned_param_indices():
            s = int(eng.steps[i])
            if s == 0:
                continue
            t = self._step_tensors.get(s)
            if t is None:
                self._step_tensors.clear()
                t = self._step_tensors[s] = torch.tensor(float(s), dtype=torch.float32)
            st = self.optimizer.state[self.params[i]]
            if st.get("step") is not t:
                st["step"] = t

    # ------------------------------------------------------------------------------------------
    @on_param_device
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        step_start = time.perf_counter()
        self._check_not_swapped("step()")
        if self.engine is None:
            self._build_engine()
        self._check_clip()
        if self._ema_decay is not None:  # (the decay and the groups are mutable between steps)
            check_ema_decay(self._ema_decay)
            for gi in range(len(self._groups)):
                check_ema_group(self._hparams_of(gi))
            self.engine.ema_decay = self._ema_decay
        if self.param_update_norms:  # (groups are mutable between steps)
            for gi in range(len(self._groups)):
                check_update_norms_group(self._hparams_of(gi))
        if self.state_dtype == torch.bfloat16:  # (groups are mutable between steps)
            check = check_bf16_state_lion_group if self._kind == "lion" else check_bf16_state_group
            for gi in range(len(self._groups)):
                check(self._hparams_of(gi), self.state_rounding)
        if self._master == "none":
            for gi in range(len(self._groups)):
                check_master_free_group(self._hparams_of(gi))
        self.engine.max_grad_norm = self.max_grad_norm
        self.engine.skip_nonfinite = self.skip_nonfinite
        self.engine.param_grad_norms = self.param_grad_norms
        had_vmax = self.engine.vmax is not None
        grads = [p.grad for p in self.params]
        seen = self._validated
        for i, (g, p) in enumerate(zip(grads, self.params)):
            # the same grad tensor as last step: already checked (a weak reference, so a grad the
            # step releases is not kept alive by the check)
            if g is None or (seen[i] is not None and seen[i]() is g):
                continue
            # (the flat arena copies a strided / expanded gradient into its slot through torch,
            # as torch's Adam would read it; the bucket arena packs raw runs: dense only)
            if g.dtype != p.dtype or g.shape != p.shape or not (g.is_contiguous() or self._flat()):
                raise ValueError("zero_amd: grads must match their param's dtype and shape (and "
                                 "be contiguous outside the flat arena)")
            seen[i] = weakref.ref(g)
        with torch.no_grad():
            self.engine.step(grads, self._hparams_of)
        if not had_vmax and self.engine.vmax is not None:
            self._expose_state()
        self._update_step_state()
        self._release_grads()
        if self._sync:
            torch.cuda.synchronize(self.engine.device)
            if self._variant != 1:  # zero1.py:67-68: ZeRO-1 never counts communication time
                self.communication_time += self.engine.comm_time_s()
            self.engine.release_retired()
        elif self.engine.n_retired() > 64:
            torch.cuda.synchronize(self.engine.device)
            self.engine.release_retired()
        self.step_time += time.perf_counter() - step_start
        return loss

    def _release_grads(self):
        # zero2.py:113 frees non-owned grads; the reduced grads live in the bucket arena, so
        # every grad is released (the next backward allocates fresh ones).  The flat arena keeps
        # every p.grad as its view of G (this rank's local gradient).
        if self._flat():
            return
        if self._overlap:
            self.engine.gb.release()
            return
        for p in self.params:
            p.grad = None

    @on_param_device
    def zero_grad(self, set_to_none: bool = True):
        if self._flat():
            # ZeRO-2 (and ZeRO-1 at ws = 1, which has no carry): None, as the reference's —
            # backward's fresh grads are then read in place (ws = 1) or landed in the arena;
            # ZeRO-1 at ws > 1: zeroed views of the grad arena (its carry follows the views)
            self.engine.zero_grad(set_to_none=set_to_none and not (self._carry and self.world_size > 1))
            return
        if self._overlap:  # grads become zeroed views of the overlap buckets (no pack copy)
            self.engine.gb.install_views()
            return
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.zero_()

    # convenience --------------------------------------------------------------------------------
    @property
    def param_groups(self):
        return self.optimizer.param_groups

    # checkpointing (zero_amd/checkpoint.py) -------------------------------------------------------
    def _ckpt_header(self):
        keyed = self.state_rounding == "stochastic" or self._master == "none"
        return ckpt.header(self._variant, self.world_size, self.rank, self.local_param_indices,
                           state_seed=self.state_seed if keyed else None, master=self._master)

    def _ckpt_views(self, i: int) -> dict:
        """name -> live view of param i's flat state (the owned params of Layout R)."""
        views = self.engine.state_views(i, ckpt=True)
        if views is None:
            raise NotImplementedError("zero_amd: state_dict() needs the reference (whole-param) layout")
        return views

    @on_param_device
    def state_dict(self):
        """The inner optimizer's state dict in torch's format (indices over the owned parameters,
        as the reference's ``opt.optimizer.state_dict()``), every tensor a copy of the engine's
        flat state, plus the split master's residual / fp32 master and ZeRO-1's carry
        (zero_amd/checkpoint.py)."""
        self._check_not_swapped("state_dict()")
        torch.cuda.synchronize(self.params[0].device)  # the state of every enqueued step
        sd = Optimizer.state_dict(self.optimizer)
        index = {id(p): k for k, p in enumerate(ckpt.inner_params(self.optimizer))}
        state = {}
        if self.engine is not None:
            for i in self.engine.owned_param_indices():
                p = self.params[i]
                if id(p) not in index:
                    continue
                state[index[id(p)]] = self.engine.save_entry(i, self._ckpt_views(i),
                                                             self.optimizer.state[p])
        sd["state"] = state
        sd["zero_amd"] = self._ckpt_header()
        return sd

    @on_param_device
    def load_state_dict(self, state_dict):
        """Restore a ``state_dict()`` of this rank (or a plain torch Adam state dict over the same
        owned parameters): hyper-parameters through torch's loader, state copied into the flat
        buffers.  Parameters are the model's (load them with the model's own state dict)."""
        self._check_not_swapped("load_state_dict()")
        ckpt.check_header(state_dict, self._ckpt_header())
        if self._ema_decay is None:
            ckpt.check_ema_load(state_dict.get("state", {}))
        if self._master == "none":
            ckpt.check_master_free_load(state_dict.get("state", {}))
        if self.engine is None:
            self._build_engine()
        eng = self.engine
        torch.cuda.synchronize(eng.device)
        seed = ckpt.saved_state_seed(state_dict)
        if seed is not None and (self.state_rounding == "stochastic" or self._master == "none"):
            self.state_seed = eng.state_seed = seed  # the saved run's bits continue
        ckpt.load_param_groups(self.optimizer, state_dict)
        self.original_param_groups = self.optimizer.param_groups
        self._groups = list(self.optimizer.param_groups)
        saved = state_dict.get("state", {})
        params = ckpt.inner_params(self.optimizer)
        if any("max_exp_avg_sq" in saved.get(k, {}) for k in range(len(params))) and eng.vmax is None:
            eng.ensure_vmax()
            if hasattr(eng, "rebuild_rows"):
                eng.rebuild_rows()
        index = {id(p): k for k, p in enumerate(params)}
        with torch.no_grad():
            for i in eng.owned_param_indices():
                p = self.params[i]
                entry = saved.get(index.get(id(p), -1), {})
                eng.load_entry(i, self._ckpt_views(i), entry, p)
        self.optimizer.state.clear()
        self._expose_state()
        self._update_step_state()
        ckpt.bind_inner_load(self)

    def __repr__(self):
        return (f"{type(self).__name__}(zero={self._variant}, ws={self.world_size}, rank={self.rank}, "
                f"owned={self.local_param_indices[:1]}..{self.local_param_indices[-1:]})")


CALIBRATION_BYTES = 256 << 20  # gradient bytes per calibration exchange (capped by the model's)


def _owner_bytes(opt) -> list:
    """Gradient bytes each rank owns under the reference's index ranges (zero1.py:55-62)."""
    ws, n = opt.world_size, len(opt.params)
    return [sum(p.numel() * p.element_size() for p in opt.params[slice(*owner_range(n, ws, r))])
            for r in range(ws)]


def calibrate_arena(opt, iters: int = 3) -> dict:
    """``arena="auto"``: time both exchanges on this job's interconnect, at construction.

    A ``CALIBRATION_BYTES`` sample of the gradient (the model's own size if smaller) is exchanged
    the flat arena's way — one RCCL group of per-owner reduces then one of per-owner broadcasts,
    windows in proportion to what each rank owns (uneven under the reference's index ranges) — and
    the bucket arena's way — equal-chunk reduce-scatter then all-gather, plus the pack and unpack
    copies it needs (two copies of the sample through the gfx950 copy kernel) — each ``iters``
    times after one warm-up, on the collective stream.  Rank 0's times decide (a collective
    finishes on every rank together) and its choice is broadcast, so every rank builds the same
    arena.  Per-step estimates scale the sample to the model's gradient bytes; the bucket arena is
    chosen only when it is at least 5 % faster (no overlap credit to either side)."""
    import numpy as np

    from .comm import RcclComm, comm_stream
    from .kernels import CopySet

    if opt._comm is None:
        opt._comm = RcclComm()
    comm, ws = opt._comm, opt.world_size
    p0 = opt.params[0]
    dev, dt = p0.device, p0.dtype
    es = p0.element_size()
    total = sum(p.numel() for p in opt.params) * es
    align = ws * 64
    n = max(align, min(total, CALIBRATION_BYTES) // es // align * align)  # elements in the sample
    own = np.asarray(_owner_bytes(opt), np.float64)
    share = own / own.sum() if own.sum() > 0 else np.full(ws, 1.0 / ws)
    win_len = np.floor(share * n).astype(np.int64)
    win_len[-1] += n - int(win_len.sum())
    win_off = np.concatenate([[0], np.cumsum(win_len)[:-1]]).astype(np.int64)
    stream = comm_stream(dev)
    buf = torch.zeros(n, dtype=dt, device=dev)
    chunk = torch.zeros(n // ws, dtype=dt, device=dev)
    scratch = torch.empty_like(buf)
    nb = n * es
    copy = CopySet([buf.data_ptr()], [scratch.data_ptr()], [nb])

    def flat():
        comm.reduce_v(buf, win_off, win_len, stream)
        comm.broadcast_v(buf, win_off, win_len, stream)

    def buckets():
        copy.run(stream)  # pack
        comm.reduce_scatter(buf, chunk, stream)
        comm.all_gather(chunk, buf, stream)
        copy.run(stream)  # unpack

    def timed(fn):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(iters):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    torch.cuda.synchronize(dev)
    t_flat, t_buck = timed(flat), timed(buckets)
    scale = total / nb
    est = {"flat": t_flat * scale, "buckets": t_buck * scale}
    chosen = "buckets" if est["buckets"] < 0.95 * est["flat"] else "flat"
    obj = [chosen]
    dist.broadcast_object_list(obj, src=0)
    del buf, chunk, scratch, copy
    return {"chosen": obj[0], "sample_bytes": nb, "grad_bytes": total,
            "sample_ms": {"flat": t_flat, "buckets": t_buck},
            "est_ms_per_step": est, "decided_by": "rank 0"}


def is_initialized() -> bool:
    return dist.is_available() and dist.is_initialized()
