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
``SfAdamSet`` — the same tables with zero_amd.optim.ScheduleFreeAdamW's update (the master is y,
``m`` is z) and ``swap``, the eval() / train() kernel; ``sfadam_hparams``.
``AdEMAMixSet`` — the same tables with zero_amd.optim.AdEMAMix's update (``m`` is exp_avg, ``v``
exp_avg_sq, ``vmax`` exp_avg_slow); ``ademamix_hparams``.
``AdamSet.run_lamb_moments`` / ``lamb_finish`` / ``AdamSet.run_lamb_apply`` — zero_amd.optim.LAMB's
update over an Adam set, two passes (csrc/zs_lamb.hip); ``lamb_hparams``.
``AdafactorSet`` — torch.optim.Adafactor's update over a table of matrices (csrc/zs_adafactor.hip):
factored second moment, three passes, every scalar on the device; ``adafactor_hparams``.
``MuonSet`` — torch.optim.Muon's update over a table of matrices (csrc/zs_muon.hip): momentum, the
Newton-Schulz iteration as bf16 MFMA products, the apply pass; ``muon_hparams``, ``muon_gemm_nt``.
With ``attach_rows`` the same set runs zero_amd.optim.NorMuon's update (``run_normuon``: the row
sums of squares, the row second moment and steps, a row-tiled apply); ``normuon_hparams``.
``AdamMiniSet`` — zero_amd.optim.AdamMini's update over a table of parameters cut into blocks
(csrc/zs_adamini.hip): a workgroup holds a block's gradient in registers between the reduction and
the apply, larger blocks take two passes; ``adamini_hparams``.
``ApolloSet`` — zero_amd.optim.Apollo's update over a table of matrices (csrc/zs_apollo.hip): the
sign sketch on MFMA with the signs formed in registers, the sketch-space Adam, the finish, the
apply; ``apollo_hparams``.
``adam_step`` — the same update over one contiguous range (zs_adam_step_ex; no table to keep).

Both upload their segment table once; ``run(stream)`` only enqueues a kernel on ``stream``.
They raise ``ZeroAmdError`` on any failure; there is no CPU path.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from ._lib import (AdafactorHParams, AdafactorSeg, AdamHParams, AdEMAMixHParams, AdamMiniHParams, AdamMiniSeg,
                   AdamSeg, ApolloHParams, ApolloSeg, LambHParams, LionHParams, MuonHParams, MuonSeg, NorMuonHParams,
                   SfAdamHParams, SgdHParams)

_PU64 = ctypes.POINTER(ctypes.c_uint64)
_PI64 = ctypes.POINTER(ctypes.c_int64)


def adam_groups(split: bool) -> int:
    """float4 groups per thread of the update kernels (csrc/zs_kernels.hip adam_groups): a chunk is
    256 * 4 * adam_groups elements, and a lane sums 4 * adam_groups fp32 terms of it."""
    return 4 if split else 2


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

    # fused LAMB (zero_amd.optim.LAMB) over an Adam set: L1, then lamb_finish, then L2
    def run_lamb_moments(self, hp: LambHParams, partials, stream, coef=None) -> None:
        """Pass L1 (zs_lambset_run_moments): m and v move as Adam's, the parameter stays; per slot
        the sums of u^2 and of master^2 into the two planes of ``partials`` (``run_stats``'s
        shape).  A row without a gradient is left out: its slots get +0.0."""
        if not isinstance(partials, int):
            assert partials.dtype.itemsize == 8
            assert partials.numel() >= 2 * self.update_norm_offsets[-1]
            partials = partials.data_ptr()
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_lambset_run_moments", self._h, ctypes.byref(hp), ptr, partials or None,
                  stream_handle(stream))

    def bind_params(self, seg_params) -> None:
        """Row i belongs to parameter ``seg_params[i]`` (zs_lambset_bind_params; the same indices
        again: nothing happens)."""
        idx = np.ascontiguousarray(np.asarray(seg_params, dtype=np.int32))
        assert idx.shape == (self.nseg,)
        if getattr(self, "_bound", None) is not None and np.array_equal(idx, self._bound):
            return
        _lib.call("zs_lambset_bind_params", self._h, self.nseg, idx.ctypes.data)
        self._bound = idx

    def run_lamb_apply(self, hp: LambHParams, neg_s, stream) -> None:
        """Pass L2 (zs_lambset_run_apply): p = fma(neg_s[parameter of the row], u, p) with u formed
        again from the moments L1 stored; ``neg_s``: the fp32 device tensor ``lamb_finish`` wrote."""
        _lib.call("zs_lambset_run_apply", self._h, ctypes.byref(hp), neg_s.data_ptr(),
                  int(neg_s.numel()), stream_handle(stream))

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

    run_sr = run_psr = run_ema = run_stats = run_lamb_moments = run_lamb_apply = _not_lion


def sfadam_hparams(lr_t, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, c=1.0, *,
                   maximize=False, grad_div=1.0, carry_mul=0.0) -> SfAdamHParams:
    """The scalars of one Schedule-Free AdamW step: ``lr_t`` the learning rate after warm-up,
    ``step`` the group's count after the increment, ``c`` its averaging weight."""
    hp = SfAdamHParams()
    _lib.call("zs_sfadam_hparams_init", float(lr_t), float(beta1), float(beta2), float(eps),
              float(weight_decay), int(step), float(c), int(bool(maximize)), float(grad_div),
              float(carry_mul), ctypes.byref(hp))
    return hp


class SfAdamSet(AdamSet):
    """Fused Schedule-Free AdamW over segments in zs_adam_seg order (zs_sfadamset_create): the
    master holds ``y``, column ``m`` is ``z`` and ``v`` is ``exp_avg_sq`` on every row, fp32;
    ``vmax`` is 0.  ``set_grads``, ``grad_sqnorm``, ``grad_sqnorm_segs``, ``bytes`` and
    ``grad_bytes`` as ``AdamSet``."""

    _CREATE = "zs_sfadamset_create"

    def run(self, hp: SfAdamHParams, stream, coef=None, guard=False) -> None:
        """One step (zs_sfadamset_run); ``coef`` as ``LionSet.run``.  ``guard`` is refused by the
        library: the rule has no guarded instances."""
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_sfadamset_run", self._h, ctypes.byref(hp), ptr, int(bool(guard)),
                  stream_handle(stream))

    def swap(self, weight: float, to_eval: bool, stream) -> None:
        """The model parameters to ``x`` (``to_eval``, ``weight = 1 - 1/beta1``) or back to ``y``
        (``weight = 1 - beta1``): zs_sfadamset_swap."""
        _lib.call("zs_sfadamset_swap", self._h, float(weight), int(bool(to_eval)),
                  stream_handle(stream))

    def run_clipped(self, hp, coef, stream) -> None:
        self.run(hp, stream, coef=coef)

    def run_guarded(self, hp, coef, stream) -> None:
        self.run(hp, stream, coef=coef, guard=True)

    def _not_sfadam(self, *a, **k):
        raise _lib.ZeroAmdError("zs_sfadamset_run", _lib.ZS_ERR_INVALID,
                                "a Schedule-Free AdamW set runs through SfAdamSet.run")

    run_sr = run_psr = run_ema = run_stats = run_lamb_moments = run_lamb_apply = _not_sfadam


def ademamix_hparams(lr, beta1=0.9, beta2=0.999, beta3_t=0.9999, alpha_t=5.0, eps=1e-8,
                     weight_decay=0.0, step=1, *, maximize=False, grad_div=1.0,
                     carry_mul=0.0) -> AdEMAMixHParams:
    """The scalars of one AdEMAMix step at the parameter's count ``step`` (after the increment);
    ``beta3_t`` and ``alpha_t``: what ``zero_amd.optim.ademamix_schedule`` gives at that count."""
    hp = AdEMAMixHParams()
    _lib.call("zs_ademamix_hparams_init", float(lr), float(beta1), float(beta2), float(beta3_t),
              float(alpha_t), float(eps), float(weight_decay), int(step), int(bool(maximize)),
              float(grad_div), float(carry_mul), ctypes.byref(hp))
    return hp


class AdEMAMixSet(AdamSet):
    """Fused AdEMAMix over segments in zs_adam_seg order (zs_ademamixset_create): column ``m`` is
    ``exp_avg``, ``v`` is ``exp_avg_sq`` and ``vmax`` is ``exp_avg_slow`` on every row, fp32.
    ``set_grads``, ``grad_sqnorm``, ``grad_sqnorm_segs``, ``bytes`` and ``grad_bytes`` as
    ``AdamSet``."""

    _CREATE = "zs_ademamixset_create"

    def run(self, hp: AdEMAMixHParams, stream, coef=None) -> None:
        """One step (zs_ademamixset_run); ``coef`` as ``LionSet.run``."""
        ptr = None if coef is None else coef if isinstance(coef, int) else coef.data_ptr()
        _lib.call("zs_ademamixset_run", self._h, ctypes.byref(hp), ptr, stream_handle(stream))

    def run_clipped(self, hp, coef, stream) -> None:
        self.run(hp, stream, coef=coef)

    def _not_ademamix(self, *a, **k):
        raise _lib.ZeroAmdError("zs_ademamixset_run", _lib.ZS_ERR_INVALID,
                                "an AdEMAMix set runs through AdEMAMixSet.run")

    run_guarded = run_sr = run_psr = run_ema = run_stats = run_lamb_moments = run_lamb_apply = \
        _not_ademamix


def lamb_hparams(beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, step=1, *,
                 bias_correction=True, maximize=False, grad_div=1.0) -> LambHParams:
    """A zero_amd.optim.LAMB group's scalars at step count ``step`` (zs_lamb_hparams_init); the
    learning rate goes to ``lamb_finish``."""
    hp = LambHParams()
    _lib.call("zs_lamb_hparams_init", float(beta1), float(beta2), float(eps), float(weight_decay),
              int(bool(bias_correction)), int(bool(maximize)), int(step), float(grad_div),
              ctypes.byref(hp))
    return hp


def lamb_finish(sums3, n: int, lr, norms2, ratios, neg_s, stream) -> None:
    """Between LAMB's passes (zs_lamb_finish) over ``sums3`` = [sum u^2 | sum p^2 | touched] and the
    per-parameter learning rates ``lr`` (fp32 device tensors): ``norms2`` = [‖w‖ | ‖u‖], the trust
    ratios and ``neg_s`` = -(lr * ratio)."""
    assert sums3.numel() >= 3 * n and norms2.numel() >= 2 * n
    assert min(lr.numel(), ratios.numel(), neg_s.numel()) >= n
    _lib.call("zs_lamb_finish", sums3.data_ptr(), int(n), lr.data_ptr(), norms2.data_ptr(),
              ratios.data_ptr(), neg_s.data_ptr(), stream_handle(stream))


def adafactor_hparams(lr=1e-2, beta2_decay=-0.8, eps=(None, 1e-3), d=1.0, weight_decay=0.0, *,
                      maximize=False, grad_div=1.0) -> AdafactorHParams:
    """A torch.optim.Adafactor group's scalars (zs_adafactor_hparams_init); ``eps[0]`` None is
    fp32's epsilon, whatever the parameter dtype: the arithmetic is fp32."""
    hp = AdafactorHParams()
    eps1, eps2 = eps
    _lib.call("zs_adafactor_hparams_init", float(lr), float(beta2_decay), int(eps1 is not None),
              0.0 if eps1 is None else float(eps1), float(eps2), float(d), float(weight_decay),
              int(bool(maximize)), float(grad_div), ctypes.byref(hp))
    return hp


class AdafactorSet:
    """Fused Adafactor over a table with one entry per (parameter, batch matrix); ``segs`` is an
    (n, 9) int64/uint64 array in zs_adafactor_seg order: g, master, master_out, p_out, row_var,
    col_var, R, C, param (col_var 0: a 1-D entry whose ``row_var`` is the variance).  ``run`` is
    one step: three passes and their reduce kernels, nothing on the host."""

    FIELDS = ("g", "master", "master_out", "p_out", "row_var", "col_var", "R", "C", "param")

    def __init__(self, segs: np.ndarray, g_dtype: int, p_dtype: int = _lib.ZS_BF16):
        segs = np.ascontiguousarray(np.asarray(segs, dtype=np.uint64).reshape(-1, 9))
        arr = (AdafactorSeg * max(len(segs), 1))()
        ctypes.memmove(arr, segs.ctypes.data, segs.nbytes)
        h = ctypes.c_void_p()
        _lib.call("zs_adafactorset_create", arr if len(segs) else None, len(segs), int(g_dtype),
                  int(p_dtype), ctypes.byref(h))
        self._h = h
        self.nseg = len(segs)
        e, b, s = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        pb = (ctypes.c_int64 * 3)()
        _lib.call("zs_adafactorset_stats", h, ctypes.byref(e), ctypes.byref(b), pb, ctypes.byref(s))
        self.elems, self.bytes, self.scratch_bytes = e.value, b.value, s.value
        self.pass_bytes = tuple(pb)

    def run(self, hp: AdafactorHParams, step: int, stream) -> None:
        """One step; ``step`` is the entries' step count after it (zs_adafactorset_run)."""
        _lib.call("zs_adafactorset_run", self._h, ctypes.byref(hp), int(step), stream_handle(stream))

    def run_pass(self, hp: AdafactorHParams, step: int, which: int, stream) -> None:
        """Pass ``which`` (0: statistics, 1: update norm, 2: apply) alone, for measurement."""
        _lib.call("zs_adafactorset_run_pass", self._h, ctypes.byref(hp), int(step), int(which),
                  stream_handle(stream))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            try:
                _lib.lib.zs_adafactorset_destroy(h)
            except Exception:  # interpreter teardown
                pass
            self._h = None


MUON_ADJUST_LR = {None: 0, "original": 0, "match_rms_adamw": 1}


def muon_hparams(lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
                 ns_coefficients=(3.4445, -4.775, 2.0315), eps=1e-7, ns_steps=5,
                 adjust_lr_fn=None, *, grad_div=1.0) -> MuonHParams:
    """A torch.optim.Muon group's scalars (zs_muon_hparams_init)."""
    if adjust_lr_fn not in MUON_ADJUST_LR:
        raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")
    if len(ns_coefficients) != 3:
        raise ValueError("Coefficients must be a tuple of exactly 3 values")
    a, b, c = (float(x) for x in ns_coefficients)
    hp = MuonHParams()
    _lib.call("zs_muon_hparams_init", float(lr), float(weight_decay), float(momentum),
              int(bool(nesterov)), a, b, c, float(eps), int(ns_steps),
              MUON_ADJUST_LR[adjust_lr_fn], float(grad_div), ctypes.byref(hp))
    return hp


def normuon_hparams(lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
                    ns_coefficients=(3.4445, -4.775, 2.0315), eps=1e-7, ns_steps=5, beta2=0.95,
                    norm_eps=1e-8, *, grad_div=1.0) -> NorMuonHParams:
    """A zero_amd.optim.NorMuon group's scalars (zs_normuon_hparams_init)."""
    if len(ns_coefficients) != 3:
        raise ValueError("Coefficients must be a tuple of exactly 3 values")
    a, b, c = (float(x) for x in ns_coefficients)
    hp = NorMuonHParams()
    _lib.call("zs_normuon_hparams_init", float(lr), float(weight_decay), float(momentum),
              int(bool(nesterov)), a, b, c, float(eps), int(ns_steps), float(beta2),
              float(norm_eps), float(grad_div), ctypes.byref(hp))
    return hp


class MuonSet:
    """Fused Muon over a table with one entry per owned matrix; ``segs`` is an (n, 8) int64/uint64
    array in zs_muon_seg order: g, master, master_out, p_out, buf, R, C, param.  ``run`` is one
    step: per batch of same-shape matrices the passes M1, M2, ns_steps x three MFMA products and
    P, nothing on the host.  ``scratch_budget`` (bytes, 0: the library's default) bounds the
    scratch and so the batch size."""

    FIELDS = ("g", "master", "master_out", "p_out", "buf", "R", "C", "param")
    STATS = ("elems", "bytes", "m1_bytes", "m2_bytes", "p_bytes", "scratch_bytes", "flops_iter",
             "flops_iter_run", "batches")

    def __init__(self, segs: np.ndarray, g_dtype: int, p_dtype: int = _lib.ZS_BF16,
                 scratch_budget: int = 0):
        segs = np.ascontiguousarray(np.asarray(segs, dtype=np.uint64).reshape(-1, 8))
        arr = (MuonSeg * max(len(segs), 1))()
        ctypes.memmove(arr, segs.ctypes.data, segs.nbytes)
        h = ctypes.c_void_p()
        _lib.call("zs_muonset_create", arr if len(segs) else None, len(segs), int(g_dtype),
                  int(p_dtype), int(scratch_budget), ctypes.byref(h))
        self._h = h
        self.nseg = len(segs)
        self._read_stats()

    def _read_stats(self) -> None:
        out = (ctypes.c_int64 * len(self.STATS))()
        _lib.call("zs_muonset_stats", self._h, out, len(self.STATS))
        for name, v in zip(self.STATS, out):
            setattr(self, name, int(v))

    def run(self, hp: MuonHParams, stream) -> None:
        _lib.call("zs_muonset_run", self._h, ctypes.byref(hp), stream_handle(stream))

    def run_pass(self, hp: MuonHParams, which: int, stream, *, product: int = -1,
                 batch: int = -1) -> None:
        """Pass ``which`` (0: M1 and the norm, 1: M2, 2: the products -- all iterations, or
        ``product`` 0, 1, 2 of one --, 3: P) over ``batch`` (-1: all), for tests and measurement."""
        _lib.call("zs_muonset_run_pass", self._h, ctypes.byref(hp), int(which), int(product),
                  int(batch), stream_handle(stream))

    def batch(self, b: int) -> dict:
        """Where batch ``b``'s scratch arrays lie (zs_muonset_batch)."""
        out = (ctypes.c_int64 * 12)()
        _lib.call("zs_muonset_batch", self._h, int(b), out)
        names = ("first", "count", "R", "C", "ldr", "ldc", "X", "XT", "A", "Bm", "norm",
                 "scratch_bytes")
        return dict(zip(names, (int(v) for v in out)))

    def attach_rows(self, row_v) -> None:
        """NorMuon's row state: ``row_v[k]`` is the device address of entry k's R fp32 second
        moments (zs_muonset_attach_rows); the set then takes ``run_normuon``."""
        arr = (ctypes.c_uint64 * max(len(row_v), 1))(*(int(a) for a in row_v))
        _lib.call("zs_muonset_attach_rows", self._h, arr if len(row_v) else None, len(row_v))
        self._read_stats()  # (the scratch bytes now count the row scratch)

    def run_normuon(self, hp: NorMuonHParams, stream) -> None:
        """One NorMuon step: M1, M2 and the products as ``run``, then N1, N2, N3."""
        _lib.call("zs_muonset_run_normuon", self._h, ctypes.byref(hp), stream_handle(stream))

    def run_normuon_pass(self, hp: NorMuonHParams, which: int, stream, *, product: int = -1,
                         batch: int = -1) -> None:
        """Pass ``which`` of ``run_normuon`` (0, 1, 2 as ``run_pass``; 3: N1, the row sums of
        squares; 4: N2, the row moments and steps; 5: N3, the apply), for tests and measurement."""
        _lib.call("zs_muonset_run_normuon_pass", self._h, ctypes.byref(hp), int(which),
                  int(product), int(batch), stream_handle(stream))

    def rows(self, b: int) -> dict:
        """Where batch ``b``'s row scratch lies (zs_muonset_rows)."""
        out = (ctypes.c_int64 * 4)()
        _lib.call("zs_muonset_rows", self._h, int(b), out)
        return dict(zip(("rowsq", "rowstep", "R", "row_bytes"), (int(v) for v in out)))

    def read(self, b: int, name: str, stream):
        """A copy of batch ``b``'s scratch array ``name`` ("X", "XT", "A", "Bm": bf16, (matrices,
        rows, columns); "norm": fp32, one per matrix; NorMuon's "rowsq": float64 and "rowstep": fp32,
        (matrices, R)) as it stands in stream order; diagnostic."""
        import torch

        info = self.batch(b)
        r, c = min(info["R"], info["C"]), max(info["R"], info["C"])
        dev = torch.device("cuda", torch.cuda.current_device())
        if name in ("rowsq", "rowstep"):
            info = {**info, **self.rows(b)}
            out = torch.empty((info["count"], info["R"]), device=dev,
                              dtype=torch.float64 if name == "rowsq" else torch.float32)
            cols = None
        elif name == "norm":
            out = torch.empty(info["count"], dtype=torch.float32, device=dev)
            cols = None
        else:
            rows, cols, ld = {"X": (r, c, info["ldc"]), "XT": (c, r, info["ldr"]),
                              "A": (r, r, info["ldr"]), "Bm": (r, r, info["ldr"])}[name]
            out = torch.empty((info["count"], rows, ld), dtype=torch.bfloat16, device=dev)
        copy_direct([info[name]], [out.data_ptr()], [out.numel() * out.element_size()], stream)
        return out if cols is None else out[:, :, :cols]

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            try:
                _lib.lib.zs_muonset_destroy(h)
            except Exception:  # interpreter teardown
                pass
            self._h = None


ADAMINI_RESIDENT_CAP = 16384  # elements; the shipped default of resident_cap


def adamini_hparams(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, *,
                    maximize=False, grad_div=1.0) -> AdamMiniHParams:
    """A zero_amd.optim.AdamMini group's scalars (zs_adamini_hparams_init)."""
    hp = AdamMiniHParams()
    _lib.call("zs_adamini_hparams_init", float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), int(bool(maximize)), float(grad_div), ctypes.byref(hp))
    return hp


class AdamMiniSet:
    """Fused Adam-mini over a table with one entry per parameter; ``segs`` is an (n, 10)
    int64/uint64 array in zs_adamini_seg order: g, master, master_out, p_out, m, v, R, C,
    block_rows, param.  A block of at most ``resident_cap`` elements is owned by one workgroup that
    reads its gradient once; larger blocks take two passes (0: every block).  ``run`` is one step,
    nothing on the host."""

    FIELDS = ("g", "master", "master_out", "p_out", "m", "v", "R", "C", "block_rows", "param")
    STATS = ("elems", "bytes", "resident_elems", "resident_bytes", "twopass_elems", "twopass_bytes",
             "scratch_bytes", "blocks", "a_addr")

    def __init__(self, segs: np.ndarray, g_dtype: int, p_dtype: int = _lib.ZS_BF16,
                 resident_cap: int = ADAMINI_RESIDENT_CAP):
        segs = np.ascontiguousarray(np.asarray(segs, dtype=np.uint64).reshape(-1, 10))
        arr = (AdamMiniSeg * max(len(segs), 1))()
        ctypes.memmove(arr, segs.ctypes.data, segs.nbytes)
        h = ctypes.c_void_p()
        _lib.call("zs_adaminiset_create", arr if len(segs) else None, len(segs), int(g_dtype),
                  int(p_dtype), int(resident_cap), ctypes.byref(h))
        self._h = h
        self.nseg = len(segs)
        out = (ctypes.c_int64 * len(self.STATS))()
        _lib.call("zs_adaminiset_stats", h, out, len(self.STATS))
        for name, v in zip(self.STATS, out):
            setattr(self, name, int(v))

    def run(self, hp: AdamMiniHParams, step: int, stream) -> None:
        """One step; ``step`` is the entries' step count after it (zs_adaminiset_run)."""
        _lib.call("zs_adaminiset_run", self._h, ctypes.byref(hp), int(step), stream_handle(stream))

    def run_pass(self, hp: AdamMiniHParams, step: int, which: int, stream) -> None:
        """Part ``which`` (0: the resident kernel, 1: pass 1 and the finish kernel, 2: pass 2)
        alone, for measurement."""
        _lib.call("zs_adaminiset_run_pass", self._h, ctypes.byref(hp), int(step), int(which),
                  stream_handle(stream))

    def read(self, name: str, stream):
        """A copy of the scratch array ``name`` ("a": the step a_b of every block, fp32, the
        entries' blocks in table order) as it stands in stream order; diagnostic."""
        import torch

        if name != "a":
            raise ValueError(f"AdamMiniSet.read: no array {name!r}")
        out = torch.empty(self.blocks, dtype=torch.float32,
                          device=torch.device("cuda", torch.cuda.current_device()))
        if self.blocks:
            copy_direct([self.a_addr], [out.data_ptr()], [4 * self.blocks], stream)
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            try:
                _lib.lib.zs_adaminiset_destroy(h)
            except Exception:  # interpreter teardown
                pass
            self._h = None


def apollo_hparams(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, *, scale=1.0,
                   scale_type="channel", update_proj_gap=200, norm_growth=1.01, maximize=False,
                   grad_div=1.0) -> ApolloHParams:
    """A zero_amd.optim.Apollo group's scalars (zs_apollo_hparams_init)."""
    if scale_type not in _lib.APOLLO_SCALE_TYPES:
        raise ValueError(f"apollo_hparams: scale_type must be 'channel' or 'tensor' (got {scale_type!r})")
    hp = ApolloHParams()
    _lib.call("zs_apollo_hparams_init", float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), float(scale), _lib.APOLLO_SCALE_TYPES[scale_type],
              int(update_proj_gap), float(norm_growth), int(bool(maximize)), float(grad_div),
              ctypes.byref(hp))
    return hp


class ApolloSet:
    """Fused APOLLO over a table with one entry per matrix; ``segs`` is an (n, 11) int64/uint64
    array in zs_apollo_seg order: g, master, master_out, p_out, m, v, fprev, R, C, seed, param.
    ``run`` is one step (the sketch, the sketch-space Adam, the finish, the apply), nothing on the
    host."""

    FIELDS = ("g", "master", "master_out", "p_out", "m", "v", "fprev", "R", "C", "seed", "param")
    STATS = ("elems", "bytes", "scratch_bytes", "a_addr", "channels", "state_elems", "sketch_addr",
             "sketch_workgroups", "sketch_elems")

    def __init__(self, segs: np.ndarray, g_dtype: int, p_dtype: int = _lib.ZS_BF16, rank: int = 256):
        segs = np.ascontiguousarray(np.asarray(segs, dtype=np.uint64).reshape(-1, 11))
        arr = (ApolloSeg * max(len(segs), 1))()
        ctypes.memmove(arr, segs.ctypes.data, segs.nbytes)
        h = ctypes.c_void_p()
        _lib.call("zs_apolloset_create", arr if len(segs) else None, len(segs), int(g_dtype),
                  int(p_dtype), int(rank), ctypes.byref(h))
        self._h = h
        self.nseg, self.rank = len(segs), int(rank)
        out = (ctypes.c_int64 * len(self.STATS))()
        _lib.call("zs_apolloset_stats", h, out, len(self.STATS))
        for name, v in zip(self.STATS, out):
            setattr(self, name, int(v))

    def run(self, hp: ApolloHParams, step: int, stream) -> None:
        """One step; ``step`` is the entries' step count after it (zs_apolloset_run)."""
        _lib.call("zs_apolloset_run", self._h, ctypes.byref(hp), int(step), stream_handle(stream))

    def run_pass(self, hp: ApolloHParams, step: int, which: int, stream) -> None:
        """Kernel ``which`` (0: the sketch, 1: the sketch-space Adam, 2: the finish, 3: the apply)
        alone, for measurement."""
        _lib.call("zs_apolloset_run_pass", self._h, ctypes.byref(hp), int(step), int(which),
                  stream_handle(stream))

    def read(self, name: str, stream, n: int | None = None):
        """A copy of a scratch array as it stands in stream order, fp32; diagnostic.  "a": the step
        a_c of every channel, the entries in table order; "sketch": the first ``n`` (default: all
        ``sketch_elems``) partial sketch sums, per entry [cut][channel][rank] at a multiple of 4
        floats, before the scale."""
        import torch

        if name not in ("a", "sketch"):
            raise ValueError(f"ApolloSet.read: no array {name!r}")
        n = self.channels if name == "a" else self.sketch_elems if n is None else int(n)
        out = torch.empty(n, dtype=torch.float32,
                          device=torch.device("cuda", torch.cuda.current_device()))
        if n:
            copy_direct([self.a_addr if name == "a" else self.sketch_addr], [out.data_ptr()],
                        [4 * n], stream)
        return out

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None:
            try:
                _lib.lib.zs_apolloset_destroy(h)
            except Exception:  # interpreter teardown
                pass
            self._h = None


def muon_gemm_nt(A, B, D, *, E=None, D2=None, alpha=1.0, beta=0.0, sym=False, stream=None) -> None:
    """``D = bf16(alpha * A @ B.T + beta * E)`` on 2-D bf16 tensors whose rows are contiguous
    (any row stride); ``D2`` receives ``D.T``; ``sym``: D is known symmetric (zs_muon_gemm_nt)."""
    def ld(t):
        if t is None:
            return 0, 0
        if t.dim() != 2 or t.stride(1) != 1 or t.element_size() != 2:
            raise ValueError("muon_gemm_nt: operands are 2-D bf16 tensors with contiguous rows")
        return t.data_ptr(), t.stride(0)
    (M, K), N = A.shape, B.shape[0]
    args = []
    for t in (A, B, E, D, D2):
        args += ld(t)
    _lib.call("zs_muon_gemm_nt", *args, M, N, K, float(alpha), float(beta), int(bool(sym)),
              stream_handle(stream))


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
