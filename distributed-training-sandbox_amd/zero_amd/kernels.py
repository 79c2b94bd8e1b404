"""Python handles for the gfx950 kernels behind the C ABI (csrc/zs_kernels.hip).

``CopySet``  — one launch of the descriptor-driven gather/scatter copy (pack / unpack).
``copy_direct`` — the same copy with the segments in the kernel arguments (no table to keep).
``AdamSet``  — one launch of the fused Adam/AdamW update over a list of segments; its
``grad_sqnorm`` / ``run_clipped`` with ``sqnorm_reduce`` and ``clip_coef`` are global-norm clipping;
``run_guarded`` (``run_sr(guard=True)``) with ``clip_coef(skipped=)`` skips a step whose norm is not
finite; ``run_sr`` with ``sr_keys`` stores bf16 moments with stochastic rounding; a set with
``p_dtype=ZS_BF16_SR`` keeps no master and ``run_psr`` rounds its bf16 parameters stochastically.
``SgdSet``   — the same tables with torch.optim.SGD's update (momentum, Nesterov); ``sgd_hparams``.
``LionSet``  — the same tables with zero_amd.optim.Lion's update (one moment, fp32 or bf16);
``lion_hparams``.
``adam_step`` — the same update over one contiguous range (zs_adam_step_ex; no table to keep).

Both upload their segment table once; ``run(stream)`` only enqueues a kernel on ``stream``.
They raise ``ZeroAmdError`` on any failure; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from ._lib import AdamHParams, AdamSeg, LionHParams, SgdHParams

_PU64 = ctypes.POINTER(ctypes.c_uint64)
_PI64 = ctypes.POINTER(ctypes.c_int64)


def stream_handle(stream) -> int:
    """uintptr_t for a torch.cuda.Stream (or an int handle)."""
    return int(stream) if isinstance(stream, int) else int(stream.cuda_stream)


# Segment tables built from tensors are checked against those tensors' storage before anything is
# launched when this is on (``ZERO_AMD_CHECK_EXTENTS=1``; tests/conftest.py sets it): the raw-pointer
# entry points cannot check, and one segment past its buffer faults the device and fails every
# later call in the process (the r04 session that lost a whole suite to one bad table).
CHECK_EXTENTS = os.environ.get("ZERO_AMD_CHECK_EXTENTS", "0") not in ("", "0")


def check_extents_enabled() -> bool:
    return CHECK_EXTENTS


def check_extents(ptrs, nbytes, tensors, what: str = "segment") -> None:
    """Raise ``ValueError`` unless every segment [ptrs[i], ptrs[i] + nbytes[i]) with nbytes > 0 and
    ptrs != 0 (0 = zero fill) lies inside the storage of one of ``tensors`` (None entries ignored)."""
    ptrs = np.asarray(ptrs, dtype=np.uint64).reshape(-1)
    nb = np.asarray(nbytes, dtype=np.int64).reshape(-1)
    if ptrs.shape != nb.shape:
        raise ValueError(f"zero_amd: {what}: {ptrs.size} pointers for {nb.size} lengths")
    if (nb < 0).any():
        raise ValueError(f"zero_amd: {what}: negative length")
    live = (nb > 0) & (ptrs != 0)
    if not live.any():
        return
    spans = sorted({(int(t.untyped_storage().data_ptr()), int(t.untyped_storage().nbytes()))
                    for t in tensors if t is not None})
    if not spans:
        raise ValueError(f"zero_amd: {what}: no tensors to check the segments against")
    lo = np.array([s for s, _ in spans], np.uint64)
    hi = lo + np.array([n for _, n in spans], np.uint64)
    p, n = ptrs[live], nb[live].astype(np.uint64)
    k = np.searchsorted(lo, p, side="right") - 1
    ok = (k >= 0) & (p + n <= hi[np.maximum(k, 0)])
    if not ok.all():
        j = int(np.nonzero(~ok)[0][0])
        raise ValueError(f"zero_amd: {what} {int(np.nonzero(live)[0][j])}: [{int(p[j]):#x}, +{int(n[j])}) "
                         "is outside every buffer it may touch (the copy was not launched)")


def _check_bounds(src, dst, nb, bounds):
    if bounds is not None and CHECK_EXTENTS:
        src_t, dst_t = bounds
        check_extents(src, nb, src_t, "source segment")
        check_extents(dst, nb, dst_t, "destination segment")


class CopySet:
    """Copy ``nbytes[i]`` bytes from ``src[i]`` to ``dst[i]`` (src 0 = zero fill).  ``bounds``:
    (source tensors, destination tensors) the segments must lie in, checked when
    ``CHECK_EXTENTS`` is on."""

    def __init__(self, src, dst, nbytes, bounds=None):
        src = np.ascontiguousarray(np.asarray(src, dtype=np.uint64))
        dst = np.ascontiguousarray(np.asarray(dst, dtype=np.uint64))
        nb = np.ascontiguousarray(np.asarray(nbytes, dtype=np.int64))
        assert src.shape == dst.shape == nb.shape
        _check_bounds(src, dst, nb, bounds)
        self.nbytes = int(nb.sum()) if nb.size else 0
        self.nseg = int(nb.size)
        h = ctypes.c_void_p()
        _lib.call("zs_copyset_create", src.ctypes.data_as(_PU64), dst.ctypes.data_as(_PU64),
                  nb.ctypes.data_as(_PI64), int(nb.size), ctypes.byref(h))
        self._h = h

    def run(self, stream) -> None:
        _lib.call("zs_copyset_run", self._h, stream_handle(stream))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            try:
                _lib.lib.zs_copyset_destroy(h)
            except Exception:  # interpreter teardown
                pass
            self._h = None


def copy_direct(src, dst, nbytes, stream, bounds=None) -> None:
    """Copy ``nbytes[i]`` bytes from ``src[i]`` to ``dst[i]`` (src 0 = zero fill) with the segments
    in the kernel arguments (zs_copy_direct): nothing uploaded, so for pointers that change on
    every call (backward's fresh gradients).  ``bounds`` as for ``CopySet``."""
    src = np.ascontiguousarray(np.asarray(src, dtype=np.uint64))
    dst = np.ascontiguousarray(np.asarray(dst, dtype=np.uint64))
    nb = np.ascontiguousarray(np.asarray(nbytes, dtype=np.int64))
    assert src.shape == dst.shape == nb.shape
    _check_bounds(src, dst, nb, bounds)
    if nb.size:
        _lib.call("zs_copy_direct", int(nb.size), src.ctypes.data, dst.ctypes.data, nb.ctypes.data,
                  stream_handle(stream))


def adam_hparams(lr, beta1, beta2, eps, weight_decay, step, *, decoupled=False, amsgrad=False,
                 maximize=False, grad_div=1.0, carry_mul=0.0) -> AdamHParams:
    hp = AdamHParams()
    _lib.call("zs_adam_hparams_init", float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), int(bool(decoupled)), int(bool(amsgrad)), int(bool(maximize)),
              int(step), float(grad_div), float(carry_mul), ctypes.byref(hp))
    return hp


class AdamSet:
    """Fused Adam over segments; ``segs`` is an (n, 9) int64/uint64 array in zs_adam_seg order:
    g, master, master_out, p_out, m, v, vmax, carry, n.

    A ``ZS_BF16_SPLIT`` set reads bf16 gradients unless ``wide_grads=True`` says that the ``g``
    column points at fp32 buffers (ZeRO-3's fp32 accumulation arena).  The library accepts either
    width and cannot tell which one a raw pointer holds; the wrong one reads twice the buffer, so
    the wide one is refused here, before the library, unless it is asked for by name.

    ``state_dtype``: None / ``ZS_F32`` — the ``m`` and ``v`` columns point at fp32 arrays — or
    ``ZS_BF16``: at bf16 arrays (zs_adamset_create_ex: bf16 moments; no vmax, no carry, no
    amsgrad).

    ``p_dtype=ZS_BF16_SR`` — master-free: row i's ``master`` and ``p_out`` are both the bf16
    parameter, updated in place; ``master_out``, ``vmax`` and ``carry`` are 0; ``g`` is bf16, or
    fp32 with ``wide_grads=True``.  ``run_psr`` is the only way to run it.  ``state_rounding``
    ("nearest" / "stochastic") says how its ``ZS_BF16`` moments are stored."""

    FIELDS = ("g", "master", "master_out", "p_out", "m", "v", "vmax", "carry", "n")

    _CREATE = "zs_adamset_create"

    def __init__(self, segs: np.ndarray, g_dtype: int, p_dtype: int = _lib.ZS_BF16, *,
                 wide_grads: bool = False, state_dtype: int | None = None,
                 state_rounding: str = "nearest"):
        state_dtype = _lib.ZS_F32 if state_dtype is None else int(state_dtype)
        psr = int(p_dtype) == _lib.ZS_BF16_SR
        if state_rounding not in ("nearest", "stochastic"):
            raise ValueError(f"zero_amd: state_rounding must be 'nearest' or 'stochastic', got "
                             f"{state_rounding!r}")
        lion = self._CREATE == "zs_lionset_create"
        if state_rounding == "stochastic" and not ((psr or lion) and state_dtype == _lib.ZS_BF16):
            raise _lib.ZeroAmdError(self._CREATE, _lib.ZS_ERR_INVALID,
                                    "state_rounding is a ZS_BF16_SR set's with ZS_BF16 state (other "
                                    "sets choose by run / run_sr)")
        if int(p_dtype) in (_lib.ZS_BF16_SPLIT, _lib.ZS_BF16_SR) and int(g_dtype) == _lib.ZS_F32 and not wide_grads:
            raise _lib.ZeroAmdError(self._CREATE, _lib.ZS_ERR_INVALID,
                                    "ZS_BF16_SPLIT / ZS_BF16_SR need bf16 grads (fp32 gradient "
                                    "buffers: wide_grads=True)")
        segs = np.ascontiguousarray(np.asarray(segs, dtype=np.uint64).reshape(-1, 9))
        arr = (AdamSeg * max(len(segs), 1))()
        ctypes.memmove(arr, segs.ctypes.data, segs.nbytes)
        h = ctypes.c_void_p()
        if lion:
            _lib.call(self._CREATE, arr, len(segs), int(g_dtype), int(p_dtype), state_dtype,
                      ctypes.byref(h))
        elif state_dtype == _lib.ZS_F32 and not (psr and self._CREATE == "zs_adamset_create"):
            _lib.call(self._CREATE, arr, len(segs), int(g_dtype), int(p_dtype), ctypes.byref(h))
        elif self._CREATE != "zs_adamset_create":
            raise _lib.ZeroAmdError(self._CREATE, _lib.ZS_ERR_INVALID,
                                    "only the Adam set takes a state_dtype")
        else:
            _lib.call("zs_adamset_create_ex", arr, len(segs), int(g_dtype), int(p_dtype),
                      state_dtype, ctypes.byref(h))
        self.state_dtype = state_dtype
        self._h = h
        if state_rounding == "stochastic":
            _lib.call("zs_adamset_set_state_rounding", h, 1)
        self.state_rounding = state_rounding
        self.nseg = len(segs)
        self._g = np.ascontiguousarray(segs[:, 0])  # the gradients bound now, per input row
        self._n = segs[:, 8].astype(np.int64)
        self._gsz = 4 if int(g_dtype) == _lib.ZS_F32 else 2
        self._stats()

    def _stats(self):
        e, b = ctypes.c_int64(), ctypes.c_int64()
        _lib.call("zs_adamset_stats", self._h, ctypes.byref(e), ctypes.byref(b))
        self.elems, self.bytes = e.value, b.value

    def set_grads(self, g: np.ndarray, stream) -> None:
        """Re-point row i's gradient to ``g[i]`` (0 = none) in stream order (zs_adamset_set_grads:
        a patch kernel on ``stream`` when any pointer changed, nothing otherwise)."""
        g = np.ascontiguousarray(np.asarray(g, dtype=np.uint64))
        assert g.shape == (self.nseg,)
        if np.array_equal(g, self._g):
            return
        _lib.call("zs_adamset_set_grads", self._h, self.nseg, g.ctypes.data, stream_handle(stream))
        self._g = g
        self._stats()

    def run(self, hp: AdamHParams, stream) -> None:
        _lib.call("zs_adamset_run", self._h, ctypes.byref(hp), stream_handle(stream))

    @property
    def grad_bytes(self) -> int:
        """Bytes of the gradients bound now (what ``grad_sqnorm`` reads)."""
        return int(self._n[self._g != 0].sum()) * self._gsz

    @property
    def sqnorm_partials(self) -> int:
        """Double partials ``grad_sqnorm`` writes for this set (fixed when the set was created)."""
        n = getattr(self, "_sq_partials", None)
        if n is None:
            c = ctypes.c_int64()
            _lib.call("zs_adamset_sqnorm_partials", self._h, ctypes.byref(c))
            n = self._sq_partials = c.value
        return n

    def grad_sqnorm(self, partials, stream) -> None:
        """Sum of squares of the gradients bound now into ``partials`` (a float64 device tensor of
        at least ``sqnorm_partials`` elements, or its address): zs_adamset_grad_sqnorm."""
        if not isinstance(partials, int):
            assert partials.dtype.itemsize == 8 and partials.numel() >= self.sqnorm_partials
            partials = partials.data_ptr()
        _lib.call("zs_adamset_grad_sqnorm", self._h, partials, stream_handle(stream))

    @property
    def sqnorm_seg_offsets(self) -> np.ndarray:
        """``nseg + 1`` int64 offsets: row i's slots in what ``grad_sqnorm_segs`` writes are
        ``[off[i], off[i + 1])``, ``off[-1]`` the set's slot count (fixed when the set was created:
        zs_adamset_sqnorm_seg_partials)."""
        off = getattr(self, "_sq_seg_off", None)
        if off is None:
            c = ctypes.c_int64()
            off = np.zeros(self.nseg + 1, np.int64)
            _lib.call("zs_adamset_sqnorm_seg_partials", self._h, ctypes.byref(c),
                      off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
            assert int(off[-1]) == c.value
            self._sq_seg_off = off
        return off

    def grad_sqnorm_segs(self, partials, stream) -> None:
        """``grad_sqnorm`` keyed by row: the sums of squares of each row's gradient into its slots
        of ``partials`` (a float64 device tensor of at least ``sqnorm_seg_offsets[-1]`` elements, or
        its address): zs_adamset_grad_sqnorm_segs."""
        if not isinstance(partials, int):
            assert partials.dtype.itemsize == 8 and partials.numel() >= self.sqnorm_seg_offsets[-1]
            partials = partials.data_ptr()
        _lib.call("zs_adamset_grad_sqnorm_segs", self._h, partials, stream_handle(stream))

    def run_clipped(self, hp: AdamHParams, coef, stream) -> None:
        """``run`` with every averaged gradient times the fp32 device scalar ``coef`` (a tensor or
        its address), read when the kernel runs: zs_adamset_run_clipped."""
        ptr = coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_adamset_run_clipped", self._h, ctypes.byref(hp), ptr, stream_handle(stream))

    def run_guarded(self, hp: AdamHParams, coef, stream) -> None:
        """``run_clipped``, except that a NaN ``coef`` (``clip_coef(..., skipped=)``'s mark of a
        non-finite norm) skips the step: nothing is read or written (zs_adamset_run_guarded)."""
        ptr = coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_adamset_run_guarded", self._h, ctypes.byref(hp), ptr, stream_handle(stream))

    def run_sr(self, hp: AdamHParams, m_base: int, keys, stream, coef=None, guard=False) -> None:
        """``run`` (``coef`` None) or ``run_clipped`` of a set with ``ZS_BF16`` state, the moments
        stored with stochastic rounding (zs_adamset_run_sr): ``keys`` = ``sr_keys(seed, step)``,
        ``m_base`` the address of element 0 of the moment array the ``m`` column points into (only
        subtracted from, never read).  ``guard``: as ``run_guarded`` (zs_adamset_run_sr_guarded; it
        needs ``coef``)."""
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_adamset_run_sr_guarded" if guard else "zs_adamset_run_sr", self._h,
                  ctypes.byref(hp), ptr, int(m_base), int(keys[0]), int(keys[1]),
                  stream_handle(stream))

    def run_psr(self, hp: AdamHParams, m_base: int, keys, stream, coef=None, guard=False) -> None:
        """One step of a ``ZS_BF16_SR`` set (zs_adamset_run_psr): the bf16 parameters are updated
        in place and rounded stochastically, their draws keyed by ``sr_pkeys(keys)``; ``keys``,
        ``m_base``, ``coef`` and ``guard`` as ``run_sr`` (``m_base`` counts elements of the moment
        array's own type, fp32 or bf16)."""
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_adamset_run_psr", self._h, ctypes.byref(hp), ptr, int(bool(guard)),
                  int(m_base), int(keys[0]), int(keys[1]), stream_handle(stream))

    def run_ema(self, hp: AdamHParams, ema_w: float, stream, coef=None, guard=False) -> None:
        """``run`` (``coef`` None), ``run_clipped`` or, with ``guard``, ``run_guarded`` of a set
        whose ``vmax`` column points at fp32 EMA arrays, followed per element by
        ``ema = lerp(ema, master as stored, ema_w)`` in the same kernel (zs_adamset_run_ema);
        ``ema_w`` = fp32(1 - decay)."""
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_adamset_run_ema", self._h, ctypes.byref(hp), ptr, int(bool(guard)),
                  float(ema_w), stream_handle(stream))

    @property
    def update_norm_offsets(self) -> np.ndarray:
        """``nseg + 1`` int64 offsets: row i's slots in each plane ``run_stats`` writes are
        ``[off[i], off[i + 1])``, ``off[-1]`` the slots per plane — 4 per chunk of the row's vector
        part, then 4 per 256-element chunk of its scalar part (fixed when the set was created:
        zs_adamset_update_norm_slots)."""
        off = getattr(self, "_un_off", None)
        if off is None:
            c = ctypes.c_int64()
            off = np.zeros(self.nseg + 1, np.int64)
            _lib.call("zs_adamset_update_norm_slots", self._h, ctypes.byref(c),
                      off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
            assert int(off[-1]) == c.value
            self._un_off = off
        return off

    def run_stats(self, hp: AdamHParams, partials, stream, coef=None, guard=False) -> None:
        """``run`` (``coef`` None), ``run_clipped`` or, with ``guard``, ``run_guarded`` with the same
        bits, and per slot the sums of (master after - master before)^2 and of master after^2 into
        the two planes of ``partials`` (a float64 device tensor of at least
        ``2 * update_norm_offsets[-1]`` elements, or its address): zs_adamset_run_stats."""
        if not isinstance(partials, int):
            assert partials.dtype.itemsize == 8
            assert partials.numel() >= 2 * self.update_norm_offsets[-1]
            partials = partials.data_ptr()
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_adamset_run_stats", self._h, ctypes.byref(hp), ptr, int(bool(guard)),
                  partials or None, stream_handle(stream))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            try:
                _lib.lib.zs_adamset_destroy(h)
            except Exception:  # interpreter teardown
                pass
            self._h = None


def sr_keys(seed: int, step: int):
    """(key0, key1) of one stochastic-rounding launch from the optimizer's seed and the step count
    of the launched part (zs_sr_keys; a host function)."""
    k0, k1 = ctypes.c_uint32(), ctypes.c_uint32()
    _lib.call("zs_sr_keys", int(seed), int(step), ctypes.byref(k0), ctypes.byref(k1))
    return k0.value, k1.value


def sr_pkeys(keys):
    """(pkey0, pkey1): the keys of the parameter's draw in a master-free launch, from the
    launch's ``keys`` (zs_sr_pkeys; a host function).  The parameter of element ``e`` rounds with
    ``sr_bits(e, sr_pkeys(keys)) & 0xFFFF``."""
    k0, k1 = ctypes.c_uint32(), ctypes.c_uint32()
    _lib.call("zs_sr_pkeys", int(keys[0]), int(keys[1]), ctypes.byref(k0), ctypes.byref(k1))
    return k0.value, k1.value


def sr_bits(e: int, keys) -> int:
    """The 32 random bits of element ``e`` under ``keys`` (zs_sr_bits; a host function): exp_avg
    rounds with the low 16, exp_avg_sq with the high 16."""
    r = ctypes.c_uint32()
    _lib.call("zs_sr_bits", int(e), int(keys[0]), int(keys[1]), ctypes.byref(r))
    return r.value


def sgd_hparams(lr, momentum=0.0, dampening=0.0, weight_decay=0.0, *, nesterov=False,
                maximize=False, first=False, grad_div=1.0, carry_mul=0.0) -> SgdHParams:
    hp = SgdHParams()
    _lib.call("zs_sgd_hparams_init", float(lr), float(momentum), float(dampening),
              float(weight_decay), int(bool(nesterov)), int(bool(maximize)), int(bool(first)),
              float(grad_div), float(carry_mul), ctypes.byref(hp))
    return hp


class SgdSet(AdamSet):
    """Fused SGD over segments in zs_adam_seg order (zs_sgdset_create): column ``m`` is the
    momentum buffer, on every row or none; ``v`` and ``vmax`` are 0.  ``set_grads``, ``grad_sqnorm``,
    ``sqnorm_partials``, ``bytes`` and ``grad_bytes`` as ``AdamSet``."""

    _CREATE = "zs_sgdset_create"

    def run(self, hp: SgdHParams, stream, coef=None) -> None:
        """One step; ``coef``: None, or the fp32 device scalar (a tensor or its address) every
        averaged gradient is multiplied by (zs_sgdset_run)."""
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_sgdset_run", self._h, ctypes.byref(hp), ptr, stream_handle(stream))

    def run_clipped(self, hp, coef, stream) -> None:
        self.run(hp, stream, coef=coef)

    def run_guarded(self, hp, coef, stream) -> None:
        raise _lib.ZeroAmdError("zs_adamset_run_guarded", _lib.ZS_ERR_INVALID,
                                "the guarded update is Adam's (SGD tells its first step from the "
                                "host's count, which a skipped step would advance)")


def lion_hparams(lr, beta1=0.9, beta2=0.99, weight_decay=0.0, *, maximize=False, grad_div=1.0,
                 carry_mul=0.0) -> LionHParams:
    hp = LionHParams()
    _lib.call("zs_lion_hparams_init", float(lr), float(beta1), float(beta2), float(weight_decay),
              int(bool(maximize)), float(grad_div), float(carry_mul), ctypes.byref(hp))
    return hp


class LionSet(AdamSet):
    """Fused Lion over segments in zs_adam_seg order (zs_lionset_create): column ``m`` is
    ``exp_avg`` on every row, fp32 or (``state_dtype=ZS_BF16``) bf16, stored to nearest or with
    ``state_rounding="stochastic"``; ``v`` and ``vmax`` are 0.  ``set_grads``, ``grad_sqnorm``,
    ``grad_sqnorm_segs``, ``bytes`` and ``grad_bytes`` as ``AdamSet``."""

    _CREATE = "zs_lionset_create"

    def run(self, hp: LionHParams, stream, coef=None, guard=False, sr=None) -> None:
        """One step (zs_lionset_run).  ``coef``: None, or the fp32 device scalar (a tensor or its
        address) every averaged gradient is multiplied by; ``guard``: a NaN ``coef`` skips the
        step, nothing is read or written; ``sr`` (a set with stochastic rounding):
        ``(m_base, (key0, key1))`` as ``AdamSet.run_sr`` takes them."""
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        if (sr is None) != (self.state_rounding != "stochastic"):
            raise _lib.ZeroAmdError("zs_lionset_run", _lib.ZS_ERR_INVALID,
                                    "sr=(m_base, keys) goes with state_rounding='stochastic', and "
                                    "only with it")
        m_base, keys = (0, (0, 0)) if sr is None else sr
        _lib.call("zs_lionset_run", self._h, ctypes.byref(hp), ptr, int(bool(guard)), int(m_base),
                  int(keys[0]), int(keys[1]), stream_handle(stream))

    def run_clipped(self, hp, coef, stream) -> None:
        self.run(hp, stream, coef=coef)

    def run_guarded(self, hp, coef, stream) -> None:
        self.run(hp, stream, coef=coef, guard=True)

    def _not_lion(self, *a, **k):
        raise _lib.ZeroAmdError("zs_lionset_run", _lib.ZS_ERR_INVALID,
                                "a Lion set runs through LionSet.run")

    run_sr = run_psr = run_ema = run_stats = _not_lion


def sqnorm_reduce(partials, n: int, sumsq, stream) -> None:
    """``sumsq`` (one fp32 device element) = the fp32 rounding of the double sum of the first ``n``
    float64 ``partials``, added in a fixed order (zs_sqnorm_reduce)."""
    assert n == 0 or (partials.dtype.itemsize == 8 and partials.numel() >= n)
    _lib.call("zs_sqnorm_reduce", partials.data_ptr() if n else None, int(n), sumsq.data_ptr(),
              stream_handle(stream))


def sqnorm_reduce_params(partials, row_ptr, slot_lo, slot_n, n_params: int, out, stream) -> None:
    """``out[i]`` (fp32 device elements) = the fp32 rounding of the double sum of parameter i's
    slots of the float64 ``partials``: the ranges ``row_ptr[i] .. row_ptr[i + 1]`` of the CSR
    (``row_ptr``, ``slot_lo``, ``slot_n``: int64 device tensors), added in a fixed order; +0.0
    without a range (zs_sqnorm_reduce_params)."""
    assert row_ptr.dtype.itemsize == 8 and row_ptr.numel() >= n_params + 1
    assert slot_lo.dtype.itemsize == 8 and slot_n.dtype.itemsize == 8
    assert out.dtype.itemsize == 4 and out.numel() >= n_params
    _lib.call("zs_sqnorm_reduce_params", partials.data_ptr(), row_ptr.data_ptr(),
              slot_lo.data_ptr(), slot_n.data_ptr(), int(n_params), out.data_ptr(),
              stream_handle(stream))


def param_norms(sumsq_vec, n: int, grad_div: float, norms, stream) -> None:
    """``norms[i] = float32(sqrt(float64(sumsq_vec[i])) / grad_div)`` for the first ``n`` fp32
    device elements: ``clip_coef``'s norm per element (zs_param_norms)."""
    assert sumsq_vec.dtype.itemsize == 4 and norms.dtype.itemsize == 4
    assert sumsq_vec.numel() >= n and norms.numel() >= n
    _lib.call("zs_param_norms", sumsq_vec.data_ptr(), int(n), float(grad_div), norms.data_ptr(),
              stream_handle(stream))


def update_norms(sums3, n: int, coef, update, weight, stream) -> None:
    """The finishing step of the per-parameter update and weight norms (zs_update_norms) over
    ``sums3`` = [sum d^2 | sum p1^2 | touched], ``n`` fp32 device elements each: where
    ``touched[i] != 0`` and the fp32 device scalar ``coef`` (a tensor, its address or None) is not
    NaN, ``update[i]`` and ``weight[i]`` become the square roots (in double, rounded once);
    elsewhere ``update[i]`` = +0.0 and ``weight[i]`` stays."""
    assert sums3.dtype.itemsize == 4 and sums3.numel() >= 3 * n
    assert update.dtype.itemsize == 4 and weight.dtype.itemsize == 4
    assert update.numel() >= n and weight.numel() >= n
    ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
    _lib.call("zs_update_norms", sums3.data_ptr(), int(n), ptr, update.data_ptr(),
              weight.data_ptr(), stream_handle(stream))


def clip_coef(sumsq, grad_div: float, max_norm: float, out2, stream, skipped=None) -> None:
    """``out2`` (two fp32 device elements) = {norm, coef}: the L2 norm of the averaged gradient
    from the raw sum of squares ``sumsq`` and clip_grad_norm_'s clamped coefficient
    (zs_clip_coef).  ``skipped`` (one 8-byte integer device element): a non-finite norm gives the
    quiet NaN as the coefficient — the guarded runs' "skip this step" — and adds one to
    ``skipped`` (zs_clip_coef_guarded)."""
    assert out2.numel() >= 2 and out2.dtype.itemsize == 4 and sumsq.dtype.itemsize == 4
    if skipped is None:
        _lib.call("zs_clip_coef", sumsq.data_ptr(), float(grad_div), float(max_norm),
                  out2.data_ptr(), stream_handle(stream))
        return
    assert skipped.numel() >= 1 and skipped.dtype.itemsize == 8
    _lib.call("zs_clip_coef_guarded", sumsq.data_ptr(), float(grad_div), float(max_norm),
              out2.data_ptr(), skipped.data_ptr(), stream_handle(stream))


def adam_step(p, g, m, v, *, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0,
              decoupled=False, grad_div=1.0, p_bf16=None, carry=None, carry_mul=0.0,
              stream=None) -> None:
    """One Adam/AdamW step over the contiguous fp32 tensors ``p`` / ``m`` / ``v`` (in place) with
    gradient sum ``g`` (fp32 or bf16, or None = zero) divided by ``grad_div``; optional bf16 copy
    of the result into ``p_bf16`` and ZeRO-1 carry.  Enqueued on ``stream`` (default: torch's
    current stream on p's device)."""
    import torch

    n = p.numel()
    for name, t in (("p", p), ("m", m), ("v", v), ("carry", carry)):
        if t is not None:
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n, name
    if g is not None:
        assert g.dtype in (torch.float32, torch.bfloat16) and g.is_contiguous() and g.numel() == n
    if p_bf16 is not None:
        assert p_bf16.dtype == torch.bfloat16 and p_bf16.is_contiguous() and p_bf16.numel() == n
    g_dtype = _lib.ZS_BF16 if g is not None and g.dtype == torch.bfloat16 else _lib.ZS_F32
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream(p.device) if stream is None else stream
    _lib.call("zs_adam_step_ex", ptr(p), ptr(p_bf16), ptr(g), g_dtype, ptr(m), ptr(v), n, float(lr),
              float(beta1), float(beta2), float(eps), float(weight_decay), int(bool(decoupled)),
              int(step), float(grad_div), ptr(carry), float(carry_mul), stream_handle(st))


def convert(src, dst, stream=None) -> None:
    """dst[:] = src converted fp32 -> bf16 (round to nearest even) or bf16 -> fp32 (zs_convert);
    contiguous tensors of equal element count, enqueued on ``stream``."""
    import torch

    from .comm import zs_dtype

    assert src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
    st = torch.cuda.current_stream(src.device) if stream is None else stream
    _lib.call("zs_convert", src.data_ptr(), zs_dtype(src.dtype), dst.data_ptr(), zs_dtype(dst.dtype),
              src.numel(), stream_handle(st))


def accumulate(dst, src, stream=None) -> None:
    """dst[i] += src[i] (zs_accumulate): contiguous, 16-byte aligned fp32 or bf16 tensors of one
    dtype and element count, enqueued on ``stream``.  fp32: one IEEE add; bf16: an fp32 add rounded
    to nearest even — torch's ``add_``.  With ``CHECK_EXTENTS`` on, both ranges are checked against
    the tensors' storage before anything is launched."""
    import torch

    from .comm import zs_dtype

    if src.dtype != dst.dtype or src.numel() != dst.numel():
        raise ValueError("zero_amd: accumulate needs dst and src of one dtype and element count")
    if not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("zero_amd: accumulate needs contiguous tensors")
    n = dst.numel()
    if CHECK_EXTENTS:
        nb = [n * dst.element_size()]
        check_extents([dst.data_ptr()], nb, [dst], "accumulate destination")
        check_extents([src.data_ptr()], nb, [src], "accumulate source")
    st = torch.cuda.current_stream(dst.device) if stream is None else stream
    _lib.call("zs_accumulate", dst.data_ptr(), src.data_ptr(), n, zs_dtype(dst.dtype),
              stream_handle(st))


def accumulate_widen(dst, src, a=None, stream=None) -> None:
    """fp32 ``dst`` from bf16 contributions (zs_accumulate_widen): ``dst[i] = a[i] + src[i]`` when
    ``a`` (bf16) is given, ``dst[i] += src[i]`` otherwise; both bf16 operands are widened exactly
    and each element gets one IEEE fp32 add.  Contiguous tensors of one element count, ``dst``
    16-byte and ``a`` / ``src`` 8-byte aligned, enqueued on ``stream``.  With ``CHECK_EXTENTS`` on,
    every range is checked against its tensor's storage before anything is launched."""
    import torch

    if dst.dtype != torch.float32 or src.dtype != torch.bfloat16 or \
            (a is not None and a.dtype != torch.bfloat16):
        raise ValueError("zero_amd: accumulate_widen needs an fp32 dst and bf16 src (and a)")
    n = dst.numel()
    if src.numel() != n or (a is not None and a.numel() != n):
        raise ValueError("zero_amd: accumulate_widen needs dst, src (and a) of one element count")
    if not (src.is_contiguous() and dst.is_contiguous() and (a is None or a.is_contiguous())):
        raise ValueError("zero_amd: accumulate_widen needs contiguous tensors")
    if n and (dst.data_ptr() % 16 or src.data_ptr() % 8 or (a is not None and a.data_ptr() % 8)):
        raise ValueError("zero_amd: accumulate_widen needs dst 16-byte and src (and a) 8-byte "
                         "aligned")
    if CHECK_EXTENTS:
        check_extents([dst.data_ptr()], [4 * n], [dst], "accumulate_widen destination")
        check_extents([src.data_ptr()], [2 * n], [src], "accumulate_widen source")
        if a is not None:
            check_extents([a.data_ptr()], [2 * n], [a], "accumulate_widen first operand")
    st = torch.cuda.current_stream(dst.device) if stream is None else stream
    _lib.call("zs_accumulate_widen", dst.data_ptr(), None if a is None else a.data_ptr(),
              src.data_ptr(), n, stream_handle(st))
