"""The fused update over one flat shard: what ZeRO-1/2's engines and ZeRO-3's update mode share.

``UpdateCore`` owns, for a shard of ``L`` elements, the flat fp32 optimizer state (one placed
allocation: ``[m][v][carry][master]`` + the split master's int16 residuals), the per-parameter step
counts, the cache of kernel sets with its retire list, and the one timed launch.  It knows nothing
of how gradients reach the shard: ``ShardEngine`` (engine.py, flat.py) is a core plus an exchange,
``zero3.ShardedOptimizer`` holds one over its chunk arena.  Callers hand it ``zs_adam_seg`` rows
(include/zero_amd.h) whose pointer columns they filled; the core fills the state columns, cuts the
rows into (group, step key, carry multiplier) parts and launches one AdamSet / SgdSet per part.
``GradClip`` is global gradient-norm clipping around those launches (and the skip of a step whose
norm is not finite), shared by the same two callers.
"""
from __future__ import annotations

import numpy as np
import torch

from .checkpoint import step_of
from .kernels import adam_hparams, lion_hparams, sgd_hparams, sr_keys

# master="none": bf16 parameters without any master — the fused update reads the bf16 parameter,
# runs the fp32 rule and stores it back rounded stochastically ("Master-free bf16
# parameters").  Adam without amsgrad or the ZeRO-1 carry only.
MASTERS = ("split", "fp32", "none")


def owner_range(n: int, ws: int, rank: int):
    """(start, end) of the parameter indices ``rank`` owns out of ``n`` (zero1.py:55-62: equal
    runs, the first ``n % ws`` ranks one longer)."""
    per, rem = n // ws, n % ws
    start = rank * per + min(rank, rem)
    return start, start + per + (1 if rank < rem else 0)


def check_params(params):
    """(device, dtype) shared by ``params``; they must live on one GPU in one dtype."""
    dev, dtype = params[0].device, params[0].dtype
    if dev.type != "cuda":
        raise RuntimeError(f"zero_amd: parameters must live on a GPU (got {dev}); "
                           "there is no CPU path")
    for p in params:
        if p.device != dev or p.dtype != dtype:
            raise TypeError("zero_amd: all parameters must share one device and dtype")
    return dev, dtype


# bf16 moments keep 8 significant bits: a pure decay x <- beta * x moves every stored value only
# while 1 - beta >= 2^-8 ("bf16 moments"); below that exp_avg_sq could never shrink
BF16_STATE_MIN_ONE_MINUS_BETA = 2.0 ** -8


KINDS = ("adam", "sgd", "lion")
# what the messages call the optimizer of a kind that an option does not support
KIND_NAMES = {"sgd": "torch.optim.SGD", "lion": "zero_amd.optim.Lion"}


def check_state_dtype(state_dtype):
    """``state_dtype`` of an optimizer as torch.float32 (None: the default) or torch.bfloat16;
    ValueError for anything else."""
    if state_dtype is None or state_dtype == torch.float32:
        return torch.float32
    if state_dtype == torch.bfloat16:
        return torch.bfloat16
    raise ValueError("zero_amd: state_dtype must be None, torch.float32 or torch.bfloat16 "
                     f"(got {state_dtype!r})")


def check_state_rounding(state_rounding, state_seed, state_dtype):
    """(``state_rounding`` as "nearest" (None: the default) or "stochastic", ``state_seed`` as an
    int); ValueError for another rounding, a seed outside [0, 2^64) or stochastic rounding of
    anything but bf16 moments (``state_dtype`` as ``check_state_dtype`` returns it)."""
    rounding = "nearest" if state_rounding is None else state_rounding
    if rounding not in ("nearest", "stochastic"):
        raise ValueError("zero_amd: state_rounding must be None, 'nearest' or 'stochastic' "
                         f"(got {state_rounding!r})")
    if isinstance(state_seed, bool) or not isinstance(state_seed, (int, np.integer)) or \
            not 0 <= int(state_seed) < 1 << 64:
        raise ValueError(f"zero_amd: state_seed must be an int in [0, 2^64) (got {state_seed!r})")
    if rounding == "stochastic" and state_dtype != torch.bfloat16:
        raise ValueError("zero_amd: state_rounding='stochastic' rounds bf16 moments: it needs "
                         "state_dtype=torch.bfloat16")
    return rounding, int(state_seed)


def check_bf16_state_group(hpd: dict, state_rounding=None) -> None:
    """What a param group may ask of bf16 moments: no amsgrad, and — rounded to nearest — both
    betas at or below 1 - 2^-8 = 0.99609375, so that every bf16 value moves under the decay;
    ValueError otherwise.  ``state_rounding`` "stochastic": any beta (the rounding is unbiased, so
    the decay acts in expectation)."""
    if hpd.get("amsgrad"):
        raise ValueError("zero_amd: state_dtype=torch.bfloat16 does not support amsgrad")
    if state_rounding == "stochastic":
        return
    for name in ("beta1", "beta2"):
        if 1.0 - float(hpd[name]) < BF16_STATE_MIN_ONE_MINUS_BETA:
            raise ValueError(
                f"zero_amd: state_dtype=torch.bfloat16 needs 1 - {name} >= 2^-8 = 0.00390625, that "
                f"is {name} <= 0.99609375 (got {name} = {hpd[name]!r}): bf16 keeps 8 significant "
                "bits and a smaller decay is rounded away, so the moment could never shrink")


def check_bf16_state_lion_group(hpd: dict, state_rounding=None) -> None:
    """Lion's bf16 momentum rounded to nearest: only beta2 is bounded (beta2 <= 0.99609375), since
    beta1 never reaches a stored value; ValueError otherwise.  "stochastic": any beta."""
    if state_rounding != "stochastic" and 1.0 - float(hpd["beta2"]) < BF16_STATE_MIN_ONE_MINUS_BETA:
        raise ValueError(
            "zero_amd: state_dtype=torch.bfloat16 needs 1 - beta2 >= 2^-8 = 0.00390625, that is "
            f"beta2 <= 0.99609375 (got beta2 = {hpd['beta2']!r}): bf16 keeps 8 significant bits and "
            "a smaller decay is rounded away, so the momentum could never shrink")


def check_master_free(kind: str, carry: bool, bf16_params: bool = True) -> None:
    """What ``master="none"`` cannot be combined with, as ValueError."""
    if kind != "adam":
        raise ValueError(f"zero_amd: master='none' is not supported with {KIND_NAMES[kind]}")
    if not bf16_params:
        raise ValueError("zero_amd: master='none' rounds bf16 parameters stochastically: it needs "
                         "bf16 parameters (fp32 parameters are their own master)")
    if carry:
        raise ValueError("zero_amd: master='none' is not supported with the ZeRO-1 gradient carry")


def check_master_free_group(hpd: dict) -> None:
    if hpd.get("amsgrad"):
        raise ValueError("zero_amd: master='none' does not support amsgrad")


def check_ema_decay(ema_decay):
    """``ema_decay`` as None (no EMA) or a float in [0, 1]; ValueError for anything else, a bool
    included (torch's ``get_ema_multi_avg_fn`` refuses a decay outside that range alike)."""
    if ema_decay is None:
        return None
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float, np.integer, np.floating)) \
            or not 0.0 <= float(ema_decay) <= 1.0:
        raise ValueError(f"zero_amd: ema_decay must be None or a number in [0, 1] (got {ema_decay!r})")
    return float(ema_decay)


def ema_weight(ema_decay) -> float:
    """The lerp weight of one EMA step: 1 - decay in double, rounded to fp32 once (torch's
    ``lerp_(p, 1 - decay)`` hands its kernels the same number)."""
    return float(np.float32(1.0 - check_ema_decay(ema_decay)))


def check_ema(kind: str, carry: bool, state_dtype=None, master=None) -> None:
    """What ``ema_decay`` cannot be combined with on an update core, as ValueError."""
    if kind != "adam":
        raise ValueError(f"zero_amd: ema_decay is not supported with {KIND_NAMES[kind]} (the EMA "
                         "is fused into the Adam update)")
    if check_state_dtype(state_dtype) == torch.bfloat16:
        raise ValueError("zero_amd: ema_decay is not supported with state_dtype=torch.bfloat16 (the "
                         "fp32 EMA would add back the bytes the bf16 moments save)")
    if master == "none":
        raise ValueError("zero_amd: ema_decay is not supported with master='none' (there is no "
                         "master to average)")
    if carry:
        raise ValueError("zero_amd: ema_decay is not supported with the ZeRO-1 gradient carry "
                         "(ZeRO-1 at world size > 1)")


def check_ema_group(hpd: dict) -> None:
    if hpd.get("amsgrad"):
        raise ValueError("zero_amd: ema_decay is not supported with amsgrad (the EMA streams "
                         "through the slot of max_exp_avg_sq)")


def check_update_norms(kind: str, carry: bool, state_dtype=None, master=None, ema=False) -> None:
    """What ``param_update_norms`` cannot be combined with on an update core, as ValueError."""
    if kind != "adam":
        raise ValueError(f"zero_amd: param_update_norms is not supported with {KIND_NAMES[kind]} "
                         "(the norms are summed inside the fused Adam update)")
    if check_state_dtype(state_dtype) == torch.bfloat16:
        raise ValueError("zero_amd: param_update_norms is not supported with "
                         "state_dtype=torch.bfloat16 (the stats instances keep fp32 moments)")
    if master == "none":
        raise ValueError("zero_amd: param_update_norms is not supported with master='none' (there "
                         "is no master to measure)")
    if ema:
        raise ValueError("zero_amd: param_update_norms is not supported with ema_decay (the EMA "
                         "has a rule family of its own)")
    if carry:
        raise ValueError("zero_amd: param_update_norms is not supported with the ZeRO-1 gradient "
                         "carry (ZeRO-1 at world size > 1)")


def check_update_norms_group(hpd: dict) -> None:
    if hpd.get("amsgrad"):
        raise ValueError("zero_amd: param_update_norms is not supported with amsgrad (the stats "
                         "instances have no max_exp_avg_sq stream)")


def join_split_master(param: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """The fp32 split master of bf16 ``param`` and its int16 ``residual``:
    (bits << 16) + sext(residual), as the kernel joins them."""
    hi = param.detach().contiguous().view(torch.int16).to(torch.int32) << 16
    return (hi + residual.reshape(hi.shape).to(torch.int32)).view(torch.float32)


def state_layout(kind: str, L: int, *, split: bool = False, fp32_master: bool = False,
                 carry: bool = False, momentum: bool = True, state_dtype=None, master=None):
    """(total fp32 words, {name: (word offset, dtype)}) of the flat state of an ``L``-element
    shard: ``m``, ``v`` (Adam; SGD: ``m`` alone, the momentum buffer, and only with ``momentum``;
    Lion: ``m`` alone, always),
    ``carry`` (ZeRO-1), ``master`` (fp32 master of bf16 params), each ``L`` fp32, then ``lo``:
    ``L`` int16 residuals of the split master in ``(L + 1) // 2`` words.  ``state_dtype``
    torch.bfloat16 (Adam or Lion, without carry): ``m`` and ``v`` (Lion: ``m`` alone) are ``L``
    bf16 each, every array from ``v`` on starting at a multiple of 4 words (16 bytes).  ``master="none"`` (Adam without
    carry): the moments alone, neither ``master`` nor ``lo``."""
    if master == "none":
        check_master_free(kind, carry)
        if split or fp32_master:
            raise ValueError("state_layout: master='none' has neither a split nor an fp32 master")
    elif master is not None and master not in MASTERS:
        raise ValueError(f"state_layout: master must be one of {MASTERS} (got {master!r})")
    if check_state_dtype(state_dtype) == torch.bfloat16:
        if kind not in ("adam", "lion") or carry:
            raise ValueError("state_layout: bf16 state is Adam's or Lion's, without the ZeRO-1 "
                             "carry")
        words = (L + 1) // 2  # of one bf16 array
        pad = lambda w: (w + 3) // 4 * 4  # noqa: E731
        lay, total = {"m": (0, torch.bfloat16)}, words
        if kind == "adam":
            lay["v"] = (pad(words), torch.bfloat16)
            total = pad(words) + words
        if fp32_master:
            lay["master"] = (pad(total), torch.float32)
            total = pad(total) + L
        if split:
            lay["lo"] = (pad(total), torch.int16)
            total = pad(total) + words
        return total, lay
    names = ["m", "v"][:2 if kind == "adam" else 1 if kind == "lion" else int(bool(momentum))]
    names += ["carry"] * bool(carry) + ["master"] * bool(fp32_master)
    lay = {name: (k * L, torch.float32) for k, name in enumerate(names)}
    total = len(names) * L
    if split:
        lay["lo"] = (total, torch.int16)
        total += (L + 1) // 2
    return total, lay


class UpdateCore:
    update_norms = False  # (param_update_norms; set by the constructor)

    def __init__(self, kind: str, L: int, device, ws: int, group_of, n_params: int, *,
                 split: bool = False, fp32_master: bool = False, carry: bool = False,
                 momentum: bool = True, placement_tries: int = 8, state_dtype=None,
                 state_rounding=None, state_seed: int = 0, master=None, ema: bool = False,
                 update_norms: bool = False):
        from .engine import probed_zeros  # (engine.py builds on this module)

        if kind not in KINDS:
            raise ValueError(f"UpdateCore: kind must be 'adam', 'sgd' or 'lion' (got {kind!r})")
        # the update: torch.optim.Adam's, torch.optim.SGD's (`momentum`: some group has a
        # momentum, so the shard holds a momentum buffer; none of them: no optimizer state at all)
        # or zero_amd.optim.Lion's (one moment, exp_avg, always)
        self.kind, self.L, self.device, self.ws = kind, int(L), device, ws
        self.group_of = list(group_of)
        # the moments' dtype: torch.float32, or torch.bfloat16 (Adam without amsgrad or carry; one
        # step widens them, runs the fp32 update and stores them rounded to nearest even, or
        # stochastically: state_rounding below)
        self.state_dtype = check_state_dtype(state_dtype)
        if self.state_dtype == torch.bfloat16 and (kind == "sgd" or carry):
            raise ValueError("zero_amd: state_dtype=torch.bfloat16 is not supported with " +
                             ("torch.optim.SGD" if kind == "sgd" else "the ZeRO-1 gradient carry"))
        # how the bf16 moments are rounded when stored: "nearest", or "stochastic" from the
        # counter-based generator keyed by (state_seed, the part's step, the element's shard index)
        self.state_rounding, self.state_seed = check_state_rounding(state_rounding, state_seed,
                                                                    self.state_dtype)
        # master="none": no master and no residual; the launches go through run_psr and every one
        # is keyed by (state_seed, step), whatever the moments' dtype
        self.master_free = master == "none"
        total, lay = state_layout(kind, self.L, split=split, fp32_master=fp32_master, carry=carry,
                                  momentum=momentum, state_dtype=self.state_dtype, master=master)
        self.state, self.placement = probed_zeros(total, torch.float32, device, placement_tries)
        for name in ("m", "v", "carry", "master", "lo"):  # residual 0: master = the bf16 param
            off, dt = lay.get(name, (0, None))
            setattr(self, name, None if dt is None else self.state[off:].view(dt)[:self.L])
        self.vmax = None
        # ema (ema_decay): an fp32 EMA of the master per element, sharded like m, allocated like
        # vmax, whose column of the rows it takes; every launch then goes through run_ema with the
        # weight of the decay as it is at that step (the owner initialises the array from the
        # master once the parameters are in place)
        self.ema, self.ema_decay = None, None
        if ema:
            check_ema(kind, bool(carry), self.state_dtype, master)
            self.ema = torch.zeros(self.L, dtype=torch.float32, device=device)
        # update_norms (param_update_norms): every launch goes through run_stats, which also sums
        # each chunk's (master after - master before)^2 and master after^2 (UpdateNorms below)
        self.update_norms = bool(update_norms)
        if self.update_norms:
            check_update_norms(kind, bool(carry), self.state_dtype, master, ema=bool(ema))
        self.steps = np.zeros(n_params, np.int64)  # torch's per-param state['step']
        self._cache = {}
        self.retired = []
        self.timing_events = None  # optional list of (start, end, bytes) per update launch
        self.last_adam_bytes = 0

    # state ------------------------------------------------------------------------------------
    def views(self, so: int, n: int, shape, *, ckpt: bool = False) -> dict:
        """name -> live view of the state of the parameter at [so, so + n) of the shard, under
        torch's names (what ``optimizer.state[p]`` holds); ``ckpt``: also what only a checkpoint
        carries (ZeRO-1's carry)."""
        cut = lambda t: t[so:so + n].view(shape)  # noqa: E731
        if self.kind == "sgd":  # torch's SGD state: the buffer alone (absent without momentum)
            views = {} if self.m is None else {"momentum_buffer": cut(self.m)}
        elif self.kind == "lion":
            views = {"exp_avg": cut(self.m)}
        else:
            views = {"exp_avg": cut(self.m), "exp_avg_sq": cut(self.v)}
        if self.master is not None:
            views["master_param"] = cut(self.master)
        if self.lo is not None:  # the fp32 master = the bf16 param's bits << 16 + this residual
            views["master_residual"] = cut(self.lo)
        if self.vmax is not None:
            views["max_exp_avg_sq"] = cut(self.vmax)
        if self.ema is not None:
            views["ema_param"] = cut(self.ema)
        if ckpt and self.carry is not None:
            views["zero1_carry"] = cut(self.carry)
        return views

    def ensure_vmax(self):
        if self.update_norms:
            check_update_norms_group({"amsgrad": True})
        if self.ema is not None:
            raise ValueError("zero_amd: ema_decay is not supported with amsgrad (the EMA streams "
                             "through the slot of max_exp_avg_sq)")
        if self.master_free:
            raise ValueError("zero_amd: master='none' does not support amsgrad")
        if self.state_dtype == torch.bfloat16:
            raise ValueError("zero_amd: state_dtype=torch.bfloat16 does not support amsgrad")
        if self.vmax is None:
            self.vmax = torch.zeros(self.L, dtype=torch.float32, device=self.device)
        return self.vmax

    def state_cols(self, rows, so) -> None:
        """Columns 4-7 (m, v, vmax -- an EMA core: the EMA array --, carry) of zs_adam_seg ``rows``
        at shard offsets ``so``."""
        so = np.asarray(so).astype(np.uint64)
        x = self.vmax if self.ema is None else self.ema
        for col, t in ((4, self.m), (5, self.v), (6, x), (7, self.carry)):
            if t is not None:
                rows[:, col] = np.uint64(t.data_ptr()) + so * np.uint64(t.element_size())

    def expose_sgd(self, optimizer, params, groups, idx, views_of) -> None:
        """torch's SGD state for the parameters ``idx``: {} until a parameter's first step, then
        its momentum buffer alone (its presence is torch's "not the first step"); nothing at all
        without momentum.  ``views_of(i)``: parameter i's views (None: not whole in this shard)."""
        for i in idx:
            i = int(i)
            if self.steps[i] == 0 or self.m is None:
                continue
            st = optimizer.state[params[i]]
            if "momentum_buffer" not in st and groups[self.group_of[i]].get("momentum", 0) != 0:
                buf = (views_of(i) or {}).get("momentum_buffer")
                if buf is not None:
                    st["momentum_buffer"] = buf

    def save_entry(self, i: int, views: dict, torch_state: dict) -> dict:
        """Parameter i's checkpoint entry: copies of ``views``, in torch's format."""
        entry = {k: v.detach().clone() for k, v in views.items()}
        if self.kind == "sgd":  # torch's SGD entry: the buffer once it exists, no step
            if self.steps[i] == 0 or "momentum_buffer" not in torch_state:
                entry.pop("momentum_buffer", None)
        else:
            entry["step"] = torch.tensor(float(self.steps[i]), dtype=torch.float32)
        return entry

    def load_entry(self, i: int, views: dict, entry: dict, param) -> None:
        """``entry`` into parameter i's ``views`` and step count.  What it lacks starts fresh:
        moments and carry 0 (torch's new Adam), the master = ``param`` as it is (residual 0), the
        EMA = the master as loaded."""
        for name, view in views.items():
            src = entry.get(name)
            if src is not None:
                view.copy_(src.reshape(view.shape))
            elif name == "master_param":
                view.copy_(param.detach().reshape(view.shape))
            elif name != "ema_param":
                view.zero_()
        if "ema_param" in views and entry.get("ema_param") is None:
            view = views["ema_param"]
            if "master_param" in views:
                view.copy_(views["master_param"])
            elif "master_residual" in views:
                view.copy_(join_split_master(param.detach().reshape(view.shape),
                                             views["master_residual"]))
            else:
                view.copy_(param.detach().reshape(view.shape))
        if self.kind == "sgd":  # no buffer saved: the parameter's next step is its first
            self.steps[i] = int(entry.get("momentum_buffer") is not None)
        else:
            self.steps[i] = step_of(entry)

    # hyper-parameters ---------------------------------------------------------------------------
    def hp_key(self, steps):
        """What of a parameter's step count the hyper-parameter struct depends on: the count
        itself (Adam's bias correction), only whether this is its first step (SGD's buffer), or
        nothing (Lion; the count itself under stochastic rounding, which is keyed by it)."""
        steps = np.asarray(steps, np.int64)
        if self.kind == "lion":  # no bias correction: only the rounding keys depend on the step
            return steps if self.state_rounding == "stochastic" else np.zeros_like(steps)
        return (steps == 1).astype(np.int64) if self.kind == "sgd" else steps

    def make_hp(self, hpd: dict, key: int, cmul: int = 0):
        """The kernel's hyper-parameter struct of one (group, hp_key, carry multiplier) part."""
        carry_mul = float(cmul) if self.carry is not None else 0.0
        if self.kind == "sgd":
            if hpd["momentum"] != 0 and self.m is None:
                raise ValueError("zero_amd: a param group's momentum became non-zero after the "
                                 "optimizer was built without momentum buffers")
            return sgd_hparams(hpd["lr"], hpd["momentum"], hpd["dampening"], hpd["weight_decay"],
                               nesterov=hpd["nesterov"], maximize=hpd["maximize"], first=bool(key),
                               grad_div=float(self.ws), carry_mul=carry_mul)
        if self.kind == "lion":
            if self.state_dtype == torch.bfloat16:  # (groups are mutable between steps)
                check_bf16_state_lion_group(hpd, self.state_rounding)
            hp = lion_hparams(hpd["lr"], hpd["beta1"], hpd["beta2"], hpd["weight_decay"],
                              maximize=hpd["maximize"], grad_div=float(self.ws), carry_mul=carry_mul)
            if self.state_rounding == "stochastic":  # the launch's keys travel with its struct
                hp.sr_keys = sr_keys(self.state_seed, int(key))
            return hp
        if self.state_dtype == torch.bfloat16:  # (groups are mutable between steps)
            check_bf16_state_group(hpd, self.state_rounding)
        if self.master_free:
            check_master_free_group(hpd)
        if self.ema is not None:
            check_ema_group(hpd)
        if self.update_norms:
            check_update_norms_group(hpd)
        if hpd["amsgrad"] and self.vmax is None:
            raise RuntimeError("amsgrad state buffer missing")
        hp = self._adam_hp(hpd, key, carry_mul)
        # the launch's keys travel with its struct
        if self.state_rounding == "stochastic" or self.master_free:
            hp.sr_keys = sr_keys(self.state_seed, int(key))
        return hp

    def _adam_hp(self, hpd: dict, key: int, carry_mul: float):
        return adam_hparams(hpd["lr"], hpd["beta1"], hpd["beta2"], hpd["eps"], hpd["weight_decay"],
                            int(key), decoupled=hpd["decoupled"], amsgrad=hpd["amsgrad"],
                            maximize=hpd["maximize"], grad_div=float(self.ws), carry_mul=carry_mul)

    # kernel sets --------------------------------------------------------------------------------
    def cached(self, key, sig: bytes, build):
        hit = self._cache.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        obj = build()
        if hit is not None:
            # tensors moved: the old table may still be read by queued kernels, and hipFree
            # synchronises the device — keep it until the next point the device is idle
            self.retired.append(hit[1])
        self._cache[key] = (sig, obj)
        return obj

    def n_retired(self) -> int:
        return len(self.retired)

    def release_retired(self):
        """Free replaced segment tables; call only after the device has been synchronised."""
        self.retired.clear()

    def launch(self, aset, hp, stream, coef=None, guard=False, stats=None) -> None:
        """Run ``aset`` (``coef``: with the clip coefficient, a device scalar's address; ``guard``:
        a NaN coefficient skips the step on the device; ``stats``, an ``update_norms`` core: the
        address of the set's two planes of partials); with ``timing_events`` on, between two HIP
        events."""
        ev = self.timing_events
        if ev is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record(stream)
        if guard and coef is None:
            raise ValueError("zero_amd: the guarded update tests the clip coefficient")
        if self.kind == "lion":
            sr = (self.m.data_ptr(), hp.sr_keys) if self.state_rounding == "stochastic" else None
            aset.run(hp, stream, coef=coef, guard=guard, sr=sr)
        elif self.update_norms:
            if stats is None:
                raise ValueError("zero_amd: param_update_norms: a launch without its partials")
            aset.run_stats(hp, int(stats), stream, coef=coef, guard=guard)
        elif self.ema is not None:
            aset.run_ema(hp, ema_weight(self.ema_decay), stream, coef=coef, guard=guard)
        elif self.master_free:
            aset.run_psr(hp, self.m.data_ptr(), hp.sr_keys, stream, coef=coef, guard=guard)
        elif self.state_rounding == "stochastic":
            aset.run_sr(hp, self.m.data_ptr(), hp.sr_keys, stream, coef=coef, guard=guard)
        elif coef is None:
            aset.run(hp, stream)
        elif guard:
            aset.run_guarded(hp, coef, stream)
        else:
            aset.run_clipped(hp, coef, stream)
        if ev is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(stream)
            ev.append((e0, e1, aset.bytes))
        self.last_adam_bytes += aset.bytes

    def run_parts(self, tag, rows, param_idx, hparams_of, stream, *, carry_mul=None, gptr=None,
                  defer=None, new_set=None):
        """Partition rows by (group, step key, carry multiplier) — torch's bias correction is per
        param (SGD: by "first step?", the momentum buffer's birth is per param), and the ZeRO-1
        carry weight depends on which grads survived since the last step — and launch one fused
        set per part, built by ``new_set(rows)`` (default: ``self.new_set``) and cached under
        ``(group, rows, first row, tag)`` while its rows stay the same.  ``gptr`` (per row): gradient addresses bound into
        the sets before they run (AdamSet.set_grads; the rows then carry g = 0).  ``defer`` (a
        list; gradient clipping): nothing is launched, every part is appended as ``(aset, hp, gptr
        of its rows or None)`` for the caller to run once the clip coefficient exists.
        Every set carries the parameter index of each of its rows as ``seg_params``.
        Returns the parts as ``(group, aset)``."""
        parts = []
        if len(rows) == 0:
            return parts
        new_set = self.new_set if new_set is None else new_set
        if carry_mul is None:
            carry_mul = np.full(len(param_idx), self.ws - 1 if self.carry is not None else 0, np.int64)
        keys = np.stack([np.asarray(self.group_of)[param_idx], self.hp_key(self.steps[param_idx]),
                         np.asarray(carry_mul, np.int64)], axis=1)
        for key in np.unique(keys, axis=0):
            sel = np.nonzero((keys == key).all(axis=1))[0]
            sub = np.ascontiguousarray(rows[sel])
            gidx, step, cmul = int(key[0]), int(key[1]), int(key[2])
            aset = self.cached((gidx, len(sel), int(sel[0]), tag), sub.tobytes(),
                               lambda: new_set(sub))
            aset.seg_params = np.asarray(param_idx, np.int64)[sel]  # (GradClip per_param)
            parts.append((gidx, aset))
            g = None if gptr is None else np.asarray(gptr, np.uint64)[sel]
            hp = self.make_hp(hparams_of(gidx), step, cmul)
            if defer is not None:
                defer.append((aset, hp, g))
                continue
            if g is not None:
                aset.set_grads(g, stream)
            self.launch(aset, hp, stream)
        return parts


def check_max_grad_norm(m) -> None:
    """``max_grad_norm`` is None or a number >= 0 (infinity: report the norm, clip nothing);
    ValueError otherwise."""
    if m is None:
        return
    if isinstance(m, bool) or not isinstance(m, (int, float)) or not m >= 0:
        raise ValueError(f"max_grad_norm must be None or a number >= 0 (got {m!r})")


def check_skip_nonfinite(skip_nonfinite, max_grad_norm, kind: str) -> bool:
    """``skip_nonfinite`` as a bool; ValueError for what it cannot be combined with: no
    ``max_grad_norm`` (the norm is what is tested; infinity gives a pure skip) and SGD (its "first
    step" is told from the host's count, which a skipped first step would advance: the momentum
    buffer would be born wrong under dampening)."""
    if not skip_nonfinite:
        return False
    if max_grad_norm is None:
        raise ValueError("zero_amd: skip_nonfinite=True tests the gradient norm: it needs "
                         "max_grad_norm (float('inf') skips without clipping)")
    if kind == "sgd":
        raise ValueError("zero_amd: skip_nonfinite=True is not supported with torch.optim.SGD "
                         "(a skipped first step would be taken for the momentum buffer's birth)")
    return True


def check_param_grad_norms(param_grad_norms, max_grad_norm) -> bool:
    """``param_grad_norms`` as a bool; ValueError without ``max_grad_norm`` (the norms come out of
    the clipping pass; infinity reports them without clipping)."""
    if not param_grad_norms:
        return False
    if max_grad_norm is None:
        raise ValueError("zero_amd: param_grad_norms=True reports from the clipping pass: it needs "
                         "max_grad_norm (float('inf') reports without clipping)")
    return True


def slot_csr(base, seg_offsets, seg_params, n_params: int):
    """(row_ptr, slot_lo, slot_n) of the slot ranges per parameter over sets collected in order:
    set k's row i -- parameter ``seg_params[k][i]`` -- owns the slots ``base[k] + seg_offsets[k][i]
    .. base[k] + seg_offsets[k][i + 1]`` of one partials tensor.  Empty ranges are dropped; a
    parameter's ranges -- several for one cut across sets -- stand in the order the sets were
    collected; one without a range has an empty row."""
    par, lo, cnt = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for b, so, idx in zip(base, seg_offsets, seg_params):
        assert len(idx) == len(so) - 1
        par.append(np.asarray(idx, np.int64))
        lo.append(int(b) + so[:-1])
        cnt.append(np.diff(so))
    par, lo, cnt = np.concatenate(par), np.concatenate(lo), np.concatenate(cnt)
    keep = cnt > 0
    par, lo, cnt = par[keep], lo[keep], cnt[keep]
    order = np.argsort(par, kind="stable")  # per parameter: the order the sets were collected
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(par, minlength=n_params))])
    return row_ptr.astype(np.int64), lo[order].astype(np.int64), cnt[order].astype(np.int64)


class GradClip:
    """Global gradient-norm clipping around an ``UpdateCore``'s launches (clip_grad_norm_ between
    the reduction and the update): what the ZeRO-1/2 flat arena and ZeRO-3's update
    mode share.  The caller collects the step's parts as ``(aset, hp, gptr or None)``
    (``run_parts(defer=)``) and calls, in stream order, ``prepare`` (host only), ``norm`` (each
    set's sum of squares into its slice of one float64 partials tensor), ``reduce`` (all partials
    into the fp32 scalar ``sumsq``, which the caller all-reduces at world size > 1), ``coef``
    ({norm, coefficient} into ``out``) and ``run`` (the update with the coefficient).  How the
    streams are ordered around the all-reduce is the caller's.  The gradient is never rewritten and
    the host never waits.

    ``per_param`` (``param_grad_norms``): ``norm`` runs the pass keyed by segment, ``reduce`` also
    sums each parameter's slots into its element of ``reduced`` — ``len(core.steps) + 1`` floats
    whose last element is ``sumsq``; the caller all-reduces ``reduced``, whatever the mode — and
    ``coef`` also writes ``param_norms``, the L2 norm of each parameter's averaged gradient.

    ``guard`` (``skip_nonfinite``): the coefficient comes from zs_clip_coef_guarded — a non-finite
    norm gives a NaN coefficient and counts in ``skipped`` — and every launch is the guarded one,
    which a NaN coefficient ends before its first load."""

    def __init__(self, core: UpdateCore, guard: bool = False, per_param: bool = False):
        self.core, self.guard, self.per_param = core, bool(guard), bool(per_param)
        dev = core.device
        self.partials = None  # float64, sized on first use
        self._key, self._off = None, np.zeros(1, np.int64)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        # what the caller all-reduces at world size > 1: the scalar, or (``per_param``) the
        # per-parameter sums of squares with the scalar as their last element
        self.reduced = self.sumsq
        self.param_norms = None
        if self.per_param:
            n = self.n_params = len(core.steps)
            self.reduced = torch.zeros(n + 1, dtype=torch.float32, device=dev)
            self.sumsq = self.reduced[n:]
            self.param_norms = torch.zeros(n, dtype=torch.float32, device=dev)
            # the CSR of slot ranges per parameter, [row_ptr | slot_lo | slot_n] in one device
            # tensor; uploaded on a stream of its own, which the host waits for, so that an
            # upload never waits for the work queued on the caller's streams
            self._csr, self._upload_stream = None, torch.cuda.Stream(dev)
        self.out = torch.zeros(2, dtype=torch.float32, device=dev)  # {norm, coef}
        self.skipped = torch.zeros(1, dtype=torch.int64, device=dev) if guard else None
        self.norm_events = None  # optional list of (start, end, bytes) per norm pass
        self.last_norm_bytes = 0

    def prepare(self, deferred, seg_params=None) -> None:
        """Each collected set's slice of the partials tensor: sized on first use, regrown only when
        the list of sets changes (the old one is retired with the core's tables: queued kernels
        may still write it).  ``per_param``: ``seg_params[k]`` is the parameter index of each
        segment of ``deferred[k]``'s set; the slices hold the sets' per-segment slots, and the
        slot ranges of every parameter — several for one cut across sets — become a CSR in the
        order the sets were collected, rebuilt under the same rule."""
        if self.per_param:
            key = tuple((id(aset), int(aset.sqnorm_seg_offsets[-1]),
                         np.asarray(idx, np.int64).tobytes())
                        for (aset, _, _), idx in zip(deferred, seg_params))
        else:
            key = tuple((id(aset), aset.sqnorm_partials) for aset, _, _ in deferred)
        if self._key != key:
            self._off = np.concatenate([[0], np.cumsum([k[1] for k in key])]).astype(np.int64)
            total = int(self._off[-1])
            buf = self.partials
            if buf is None or buf.numel() < total:
                if buf is not None:
                    self.core.retired.append(buf)
                self.partials = torch.zeros(max(total, 1), dtype=torch.float64,
                                            device=self.core.device)
            if self.per_param:
                if self._csr is not None:
                    self.core.retired.append(self._csr)
                with torch.cuda.stream(self._upload_stream):
                    self._csr = torch.from_numpy(self._build_csr(deferred, seg_params)).to(
                        self.core.device)
                self._upload_stream.synchronize()
            self._key = key
        self.last_norm_bytes = 0

    def _build_csr(self, deferred, seg_params) -> np.ndarray:
        row_ptr, lo, cnt = slot_csr(self._off[:-1], [aset.sqnorm_seg_offsets for aset, _, _ in deferred],
                                    seg_params, self.n_params)
        return np.concatenate([row_ptr, lo, cnt]).astype(np.int64)

    def norm(self, deferred, first, stream) -> None:
        """Stage 1 for ``deferred[first:]``: bind the gradients where needed, then the sum of
        squares into the set's slice."""
        base = self.partials.data_ptr()
        for k in range(first, len(deferred)):
            aset, _, g = deferred[k]
            if g is not None:
                aset.set_grads(g, stream)
            ev = None
            if self.norm_events is not None:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(stream)
            if self.per_param:
                aset.grad_sqnorm_segs(base + int(self._off[k]) * 8, stream)
            else:
                aset.grad_sqnorm(base + int(self._off[k]) * 8, stream)
            nb = aset.grad_bytes  # what the pass reads
            if ev is not None:
                ev[1].record(stream)
                self.norm_events.append((ev[0], ev[1], nb))
            self.last_norm_bytes += nb

    def reduce(self, stream) -> None:
        """Stage 2: one fixed-order reduction of all partials into ``sumsq`` (no sets: 0);
        ``per_param``: before it, each parameter's slots into its element of ``reduced``."""
        from .kernels import sqnorm_reduce, sqnorm_reduce_params

        if self.per_param:
            n, t = self.n_params, self._csr
            nr = (t.numel() - (n + 1)) // 2
            sqnorm_reduce_params(self.partials, t[:n + 1], t[n + 1:n + 1 + nr], t[n + 1 + nr:], n,
                                 self.reduced, stream)
        sqnorm_reduce(self.partials, int(self._off[-1]), self.sumsq, stream)

    def coef(self, max_norm, stream) -> None:
        """Stage 3, after the caller's all-reduce of ``sumsq``: {norm, coefficient} of the gradient
        averaged over the core's world size."""
        from .kernels import clip_coef, param_norms

        clip_coef(self.sumsq, float(self.core.ws), float(max_norm), self.out, stream,
                  skipped=self.skipped if self.guard else None)
        if self.per_param:
            param_norms(self.reduced, self.n_params, float(self.core.ws), self.param_norms, stream)

    def run(self, deferred, first, last, stream, stats=None) -> None:
        """Stage 4 for ``deferred[first:last]``: the update with the coefficient (``stats``: the
        step's ``UpdateNorms``, prepared over the same list)."""
        coef = self.out.data_ptr() + 4
        for k in range(first, min(last, len(deferred))):
            aset, hp, _ = deferred[k]
            self.core.launch(aset, hp, stream, coef, guard=self.guard,
                             stats=None if stats is None else stats.planes(k))


class UpdateNorms:
    """Per-parameter update and weight norms out of an ``update_norms`` core's launches (DESIGN.md
    §4): a stage beside ``GradClip``, shared by the ZeRO-1/2 flat arena and ZeRO-3's update mode.
    The caller collects the step's parts as ``(aset, hp, gptr or None)`` and calls ``prepare`` (host
    only), launches set k with ``stats=planes(k)`` (``UpdateCore.launch`` / ``GradClip.run``), then
    in stream order ``reduce`` (each parameter's slots of both planes into ``sums3`` =
    [sum d^2 | sum p1^2 | touched], which the caller all-reduces at world size > 1) and ``finish``
    (the square roots into ``update`` and ``weight``; a skipped step or an untouched parameter:
    update +0.0, weight kept).  The host never waits for the step's work."""

    def __init__(self, core: UpdateCore):
        self.core = core
        dev = core.device
        n = self.n_params = len(core.steps)
        self.partials = None  # float64, sized on first use: per set two planes of its slots
        self._key, self._off = None, np.zeros(1, np.int64)
        self.sums3 = torch.zeros(3 * n, dtype=torch.float32, device=dev)
        self.update = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        self.weight = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        # [row_ptr | slot_lo of plane 0 | slot_lo of plane 1 | slot_n] and the touched mask, uploaded
        # like GradClip's CSR on a stream of its own, which the host waits for
        self._csr, self._touched = None, None
        self._upload_stream = torch.cuda.Stream(dev)

    @staticmethod
    def tables(base, seg_offsets, seg_params, n_params: int):
        """(csr, touched) on the host for sets whose two planes start at ``base[k]``: the CSR as
        [row_ptr | slot_lo of the update plane | slot_lo of the weight plane | slot_n] and the 0/1
        mark "a set has a range for parameter i" as float32."""
        row_ptr, lo_d, cnt = slot_csr(base, seg_offsets, seg_params, n_params)
        base_w = [int(b) + int(so[-1]) for b, so in zip(base, seg_offsets)]
        _, lo_w, _ = slot_csr(base_w, seg_offsets, seg_params, n_params)
        touched = (np.diff(row_ptr) > 0).astype(np.float32)
        return np.concatenate([row_ptr, lo_d, lo_w, cnt]).astype(np.int64), touched

    def prepare(self, deferred, seg_params) -> None:
        """Each collected set's slice (two planes) of the partials tensor, the CSR and the touched
        mask, under ``GradClip.prepare``'s rules: sized on first use, rebuilt only when the list of
        sets or their parameters change, what they replace retired with the core's tables."""
        key = tuple((id(aset), int(aset.update_norm_offsets[-1]), np.asarray(idx, np.int64).tobytes())
                    for (aset, _, _), idx in zip(deferred, seg_params))
        if self._key == key:
            return
        self._off = np.concatenate([[0], np.cumsum([2 * k[1] for k in key])]).astype(np.int64)
        total = int(self._off[-1])
        buf = self.partials
        if buf is None or buf.numel() < total:
            if buf is not None:
                self.core.retired.append(buf)
            self.partials = torch.zeros(max(total, 1), dtype=torch.float64, device=self.core.device)
        csr, touched = self.tables(self._off[:-1], [aset.update_norm_offsets for aset, _, _ in deferred],
                                   seg_params, self.n_params)
        if self._csr is not None:
            self.core.retired.extend([self._csr, self._touched])
        with torch.cuda.stream(self._upload_stream):
            self._csr = torch.from_numpy(csr).to(self.core.device)
            self._touched = torch.from_numpy(touched).to(self.core.device)
        self._upload_stream.synchronize()
        self._key = key

    def planes(self, k: int) -> int:
        """The address of set k's two planes."""
        return self.partials.data_ptr() + int(self._off[k]) * 8

    def reduce(self, stream) -> None:
        """Each parameter's slots of the two planes into ``sums3``, and this rank's touched mask
        behind them."""
        from .kernels import sqnorm_reduce_params

        n, t = self.n_params, self._csr
        nr = (t.numel() - (n + 1)) // 3
        row_ptr, cnt = t[:n + 1], t[n + 1 + 2 * nr:]
        for plane in (0, 1):
            sqnorm_reduce_params(self.partials, row_ptr, t[n + 1 + plane * nr:n + 1 + (plane + 1) * nr],
                                 cnt, n, self.sums3[plane * n:], stream)
        with torch.cuda.stream(stream):
            self.sums3[2 * n:].copy_(self._touched)

    def finish(self, coef_ptr, stream) -> None:
        """After the caller's all-reduce of ``sums3``: the norms (``coef_ptr``: the clip coefficient
        of a guarded step, whose NaN marks the step as skipped; None otherwise)."""
        from .kernels import update_norms

        update_norms(self.sums3, self.n_params, coef_ptr, self.update, self.weight, stream)
