"""Fused uplink of one round: encode every client row with its codec and reduce, one call.

    out = (sum_i w_i * C_i(g_i)) / sum(w)        (flc_encode_reduce)

``C_i`` is the compressor of client i (``compressors.py:218-371``) under its own pattern; the sum
runs in client order with fp32 rounding per operation, i.e. bit-identical to encoding each row
with ``compressVector`` and reducing the dense outputs sequentially (the reference's
``serverGradient`` order, algorithms.py:1753-1768) — without materialising the N dense outputs.

Pattern sources
  * compat  — the reference's numpy stream: RandK index sets [N, K] int64 and dithering /
              natural uniforms [N, D] float64 drawn on the host (``stream_choice`` /
              ``stream_rand``) and uploaded; lazy draws [N] float64.
  * device  — counter-based draws keyed by (seed, client id, element) generated inside the
              kernels: no host work, no uniform bytes (the benchmark mode).
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .compressors import Compressor, CompressorType


def _device(device):
    """torch.device with its index resolved (``'cuda'`` -> the current device), so that it compares
    equal to a stream's device."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _fold_weights(weights, n, dev, keep, divisor):
    """``(w_ptr, total)`` of a weighted fold: the weights as an fp32 device tensor (None: every w_i = 1)
    and the fp32 divisor — the weights summed in order as Python floats (n without weights),
    ``divisor`` in its place when given."""
    w_ptr, total = None, float(n)
    if weights is not None:
        weights = [float(w) for w in weights]
        if len(weights) != n:
            raise ValueError(f"weights must hold {n} values")
        if n:
            total = weights[0]
            for w in weights[1:]:
                total += w
            wt = torch.tensor(weights, dtype=torch.float32, device=dev)
            keep.append(wt)
            w_ptr = wt.data_ptr()
    if divisor is not None:
        total = float(divisor)
    return w_ptr, total


def _pointer_table(tensors, dev, keep):
    """Device array of the tensors' addresses.  Pinned staging + async copy: no host wait on the
    work already queued on the stream."""
    host_pt = torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64).pin_memory()
    pt = host_pt.to(dev, non_blocking=True)
    keep.extend(tensors)
    keep.append(pt)
    return pt.data_ptr()


def _is_fp32_device(v):
    return v.dtype == torch.float32 and v.is_cuda


def _row_matrix(who, name, v, n, d, like=""):
    """``(ptr, ld)`` of an [N, D] row-contiguous operand; ``who``: the class the messages name."""
    if tuple(v.shape) != (n, d):
        raise ValueError(f"{who}: {name} must be [{n}, {d}]{like} (got {tuple(v.shape)})")
    if d > 1 and v.stride(1) != 1:
        raise ValueError(f"{who}: {name} must be row-contiguous")
    return v.data_ptr(), v.stride(0)


def _base_rows(who, base, n, d, rows):
    """``(ptr, ld)`` of a base: ONE [D] vector for every row (ld 0) or [N, D] rows through ``rows``."""
    if base.dim() == 1:
        if base.numel() != d or (d > 1 and base.stride(0) != 1):
            raise ValueError(f"{who}: a shared base must be a contiguous [{d}] vector")
        return base.data_ptr(), 0
    ptr, ld = rows("base", base)
    if n > 1 and ld == 0:
        raise ValueError(f"{who}: pass a shared base as a [D] vector")
    return ptr, ld


def _pattern_draws(pat, t, randk_idx, uniforms, lazy_u):
    """The compat draws of a call into ``pat``; returns whether the device RNG (a seed) is needed."""
    if t == CompressorType.RANDK_COMPRESSOR and randk_idx is not None:
        pat.d_randk_idx = randk_idx.data_ptr()
        pat.idx_ld = randk_idx.stride(0)
    if uniforms is not None:
        pat.d_uniforms = uniforms.data_ptr()
        pat.uniforms_ld = uniforms.stride(0)
    if t == CompressorType.LAZY_COMPRESSOR:
        if lazy_u is None:
            raise ValueError("lazy codec needs lazy_u [N] draws")
        pat.d_lazy_u = lazy_u.data_ptr()
    return (t == CompressorType.RANDK_COMPRESSOR and randk_idx is None) or \
           (t in (CompressorType.NATURAL_COMPRESSOR_FP32, CompressorType.STANDARD_DITHERING_FP32) and uniforms is None)


def _pattern_counts(pat, randk_counts, n, d):
    """RandK device draws: the chunk counts of ``UplinkReducer.randk_counts(n, d, client0)``."""
    if tuple(randk_counts.shape) != ((d + 4095) // 4096, n) or not randk_counts.is_cuda:
        raise ValueError("randk_counts must be a [ceil(d / 4096), n] device tensor")
    pat.d_randk_counts = randk_counts.data_ptr()


def select_row_flags(comp: Compressor, n, d, device=None):
    """Path report of the last TopK call on the current stream's workspace (flc_select_row_flags): a
    [n] int64 tensor of row state bits — 1 overflow, 2 short list, 4 ties cut on the fast path,
    8 exact path, 16 a lone row selected in registers (compressVector, D <= 16.7 M).  Call it right after the UplinkReducer / compressVector call, with its n and d
    (compressVector: n = 1).  Tests use it to assert which path ran."""
    dev = _device(device)
    lib = _lib.load()
    prm, _ = comp.codec_params(dev)
    ws_bytes = lib.flc_encode_reduce_workspace_size(ctypes.byref(prm), n, d)
    ws = _lib.WORKSPACE.get(dev, ws_bytes)
    flags = torch.zeros(n, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.flc_select_row_flags(ctypes.byref(prm), n, d, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                      ctypes.c_void_p(flags.data_ptr()), _lib.stream_ptr(dev))
    _lib.check(rc, "flc_select_row_flags")
    return flags.cpu().to(torch.int64)


class UplinkReducer:
    """Holds the codec constants + workspace for repeated fused encode+reduce calls."""

    def __init__(self, compressor: Compressor, device=None, seed=None):
        _lib.require_gpu()
        self.comp = compressor
        self.device = _device(device)
        self.seed = seed

    def params(self):
        prm, keep = self.comp.codec_params(self.device)
        if self.seed is not None:
            prm.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return prm, keep

    def norm_mode(self):
        """flc_encode_reduce_ex's norm_mode for this compressor: FLC_NORMMODE_TORCH_CPU when its
        ``norm_mode`` is "torch_cpu" and it is a p = 2 dithering codec (p = inf: the maximum, exact
        in any order; p = 1: NotImplementedError), else FLC_NORMMODE_EXACT."""
        return _lib.FLC_NORMMODE_TORCH_CPU if self.comp._torch_norm() else _lib.FLC_NORMMODE_EXACT

    def workspace_bytes(self, n, d, pnorms_in=False):
        prm, _ = self.params()
        mode = _lib.FLC_NORMMODE_EXACT if pnorms_in else self.norm_mode()
        return _lib.load().flc_encode_reduce_ex_workspace_size(ctypes.byref(prm), n, d, 1 if pnorms_in else 0, mode)

    def randk_counts(self, n, d, client0=0, out=None):
        """The device sampler's chunk counts [ceil(d / 4096), n] (uint32 as int32) of clients
        client0.. on the current stream (flc_device_randk_counts) — pure compute, no row is read;
        hand them to __call__(randk_counts=...) to take that work out of the call."""
        lib = _lib.load()
        dev = self.device
        if self.seed is None:
            raise ValueError("device-RNG counts need a seed")
        C = (d + 4095) // 4096
        if out is None:
            out = torch.empty((C, n), dtype=torch.int32, device=dev)
        wsb = lib.flc_device_randk_counts_workspace_size(n, d)
        if getattr(self, "_cnt_ws", None) is None or self._cnt_ws.numel() < wsb:
            self._cnt_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.flc_device_randk_counts(int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(client0), n, d, self.comp.K,
                                             ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(self._cnt_ws.data_ptr()),
                                             self._cnt_ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "flc_device_randk_counts")
        return out

    def __call__(self, rows, out=None, weights=None, client0=0, randk_idx=None, uniforms=None, lazy_u=None,
                 pnorms_out=None, stream=None, divisor=None, randk_counts=None, pnorms_in=None):
        """rows: [N, D] fp32 device tensor (row stride % 4 == 0 for the vector path) or a list of
        [D] device tensors.  Compat patterns: randk_idx [N, K] int64, uniforms [N, D] float64,
        lazy_u [N] float64 (device).  Without them (and with ``seed`` set) draws are on device.
        ``divisor`` overrides the fp32 divisor sum(w) (e.g. 1.0 for a partial sum across GPUs).
        ``stream``: every allocation, copy and the launch go to that stream (torch's stream
        semantics: the caller orders it after the producers of ``rows`` and the patterns).
        ``randk_counts``: RandK device mode, the chunk counts from ``randk_counts(n, d, client0)``.
        ``pnorms_in``: dithering codecs, an [N] fp32 device tensor of the rows' norms to encode with
        instead of computing any (the norms a server received on the wire); it takes the place of
        the compressor's ``norm_mode``.  ``pnorms_out`` reports the norms used in every mode: with
        ``norm_mode = "torch_cpu"`` (p = 2) the reference's own torch.norm bits."""
        if stream is not None:
            if stream.device != self.device:
                raise ValueError(f"stream is on {stream.device}, the reducer runs on {self.device}")
            with torch.cuda.stream(stream):
                return self._run(rows, out, weights, client0, randk_idx, uniforms, lazy_u, pnorms_out, divisor,
                                 randk_counts, pnorms_in)
        return self._run(rows, out, weights, client0, randk_idx, uniforms, lazy_u, pnorms_out, divisor, randk_counts,
                         pnorms_in)

    def _run(self, rows, out, weights, client0, randk_idx, uniforms, lazy_u, pnorms_out, divisor, randk_counts=None,
             pnorms_in=None):
        """The call on the current stream (allocations, uploads and the launch all on it)."""
        lib = _lib.load()
        dev = self.device
        # which norm the dithering codecs encode with: the caller's, torch's CPU order, or the exact one
        mode = _lib.FLC_NORMMODE_EXACT if pnorms_in is not None else self.norm_mode()
        prm, keep = self.params()
        pat = _lib.FlcPattern()
        pat.client0 = int(client0)
        if torch.is_tensor(rows) and rows.dim() == 2:
            n, d = rows.shape
            base, ld, ptrs = rows.data_ptr(), rows.stride(0), None
            if rows.stride(1) != 1:
                raise ValueError("rows must be row-contiguous")
        else:
            n = len(rows)
            d = rows[0].numel() if n else 0
            # the pointer-array entry reads rows with 16-byte vector loads: keep them aligned
            rows = [r if (r.is_contiguous() and r.data_ptr() % 16 == 0) else r.contiguous().clone() for r in rows]
            base, ld, ptrs = None, 0, _pointer_table(rows, dev, keep)
        if out is None:
            out = torch.empty(d, dtype=torch.float32, device=dev)
        if n == 0:
            return out.zero_()                                   # no clients (algorithms.py:2117-2118)
        t = self.comp.compressorType
        if randk_counts is not None and t == CompressorType.RANDK_COMPRESSOR and randk_idx is None:
            _pattern_counts(pat, randk_counts, n, d)
        if _pattern_draws(pat, t, randk_idx, uniforms, lazy_u) and self.seed is None:
            raise ValueError("no compat pattern given and no device-RNG seed set")
        w_ptr, total = _fold_weights(weights, n, dev, keep, divisor)
        pin_ptr = None
        if pnorms_in is not None:
            if (not torch.is_tensor(pnorms_in) or pnorms_in.dtype != torch.float32 or pnorms_in.device != dev
                    or pnorms_in.numel() != n):
                raise ValueError(f"pnorms_in must be an [N] fp32 tensor on {dev}")
            pnorms_in = pnorms_in.reshape(-1).contiguous()
            keep.append(pnorms_in)
            pin_ptr = pnorms_in.data_ptr()
        st = _lib.stream_ptr(dev)
        if not hasattr(lib, "flc_encode_reduce_ex"):
            # an A/B build of an older revision (tools/ab_inproc.py): the same call without the selectors
            if pin_ptr or mode != _lib.FLC_NORMMODE_EXACT:
                raise NotImplementedError("this library build has no flc_encode_reduce_ex (pnorms_in / norm_mode)")
            ws = _lib.WORKSPACE.get(dev, lib.flc_encode_reduce_workspace_size(ctypes.byref(prm), n, d))
            with torch.cuda.device(dev):
                rc = lib.flc_encode_reduce(ctypes.byref(prm), ctypes.byref(pat), ctypes.c_void_p(base), ld,
                                           ctypes.c_void_p(ptrs), n, d, ctypes.c_void_p(w_ptr), ctypes.c_float(total),
                                           ctypes.c_void_p(pnorms_out.data_ptr() if pnorms_out is not None else None),
                                           ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(), st)
            _lib.check(rc, "flc_encode_reduce")
            return out
        ws_bytes = lib.flc_encode_reduce_ex_workspace_size(ctypes.byref(prm), n, d, 1 if pin_ptr else 0, mode)
        ws = _lib.WORKSPACE.get(dev, ws_bytes)
        with torch.cuda.device(dev):
            rc = lib.flc_encode_reduce_ex(ctypes.byref(prm), ctypes.byref(pat), ctypes.c_void_p(base), ld,
                                          ctypes.c_void_p(ptrs), n, d, ctypes.c_void_p(w_ptr), ctypes.c_float(total),
                                          ctypes.c_void_p(pin_ptr), mode,
                                          ctypes.c_void_p(pnorms_out.data_ptr() if pnorms_out is not None else None),
                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(), st)
        _lib.check(rc, "flc_encode_reduce_ex")
        return out


# ShiftUplinkReducer's rounds by keyword (None: the general entry):
#   ABI entry, it takes the pattern, its size query takes the pattern, it takes pnorms_out
_SHIFT_MODES = {
    None: ("flc_encode_shift_reduce", True, False, True),
    "one_read": ("flc_dither_shift_reduce", True, False, True),
    "batched": ("flc_topk_shift_reduce", False, False, False),
    "sparse": ("flc_randk_shift_reduce", True, True, False),
}


def _shift_mode(sparse, batched, one_read):
    return "one_read" if one_read else "batched" if batched else "sparse" if sparse else None


def _shift_workspace_size(lib, mode, prm, pat, n, d, sampled=False):
    entry, _, size_pat, _ = _SHIFT_MODES[mode]
    args = (ctypes.byref(prm), ctypes.byref(pat), n, d) if size_pat else (ctypes.byref(prm), n, d)
    return getattr(lib, entry + ("_sampled" if sampled else "") + "_workspace_size")(*args)


# ShiftUplinkReducer's per-row operands other than a, by keyword, with their flc_row_map.indexed bits
_IDX_BITS = {"b": _lib.FLC_IDX_B, "base": _lib.FLC_IDX_BASE, "msg_out": _lib.FLC_IDX_MSG, "shift": _lib.FLC_IDX_SHIFT_IN,
             "shift_out": _lib.FLC_IDX_SHIFT_OUT}


def _client_ids(who, clients, n):
    """The participants of a sampled round as a list of distinct non-negative ints, one per row of a."""
    ids = [int(c) for c in (clients.tolist() if hasattr(clients, "tolist") else clients)]
    if len(ids) != n:
        raise ValueError(f"{who}: clients must name one client per row of a ({n}), got {len(ids)}")
    if any(c < 0 or c > 0x7FFFFFFF for c in ids):
        raise ValueError(f"{who}: client ids must be in [0, 2^31)")
    if len(set(ids)) != len(ids):
        raise ValueError(f"{who}: a client takes part in a round once (duplicate ids in clients)")
    return ids


class ShiftUplinkReducer:
    """A DIANA / EF21 / MARINA / FRECON / COFIG round of N resident clients in one call
    (flc_encode_shift_reduce):

        msg_i = base_i + C_i(a_i - b_i) * scale;   shift_i' = shift_i + alpha * C_i(a_i - b_i)
        out   = (sum_i w_i * msg_i) / sum(w)

    Row i gets exactly the bits ``Compressor.compressShift`` gives for (a_i, b_i, base_i, shift_i)
    under pattern row i / client ``client0 + i``, and ``out`` the bits of ``reduce_rows`` over the N
    messages in client order — without storing them.  Elementwise codecs run one tile-owner pass
    (k_ew_shift_accum, after one norm pass over the differences for dithering); RandK / TopK /
    Rank-K run their rows in order with a fold step each (correct, not a fast path).  Dithering
    encodes with the exactly rounded norm of a_i - b_i, like ``compressShift``: the compressor's
    ``norm_mode = "torch_cpu"`` does not apply to shifted steps.

    ``sparse=True`` (RandK only) runs the round through ``flc_randk_shift_reduce``: work
    proportional to N K, not N D.  It takes shapes A - D of the table in ``include/flcodec.h``, in this
    call's terms ``shift is shift_out is b`` (A), ``base is msg_out is b`` (B), a shared [D] ``base``
    (C) and none of them (D); anything else raises ``NotImplementedError``.  Elements
    of the in-place operand OUTSIDE a row's index set are not written (the general entry stores
    ``x + 0`` there: the same bits except that a stored -0 becomes +0); selected elements and
    ``out`` carry the general entry's bits whenever the operand holds no -0 at an unselected
    place.

    ``batched=True`` (TopK only) runs the round through ``flc_topk_shift_reduce``: the N
    differences formed in one launch, the many-row selection of the fused uplink over them, a sparse
    epilogue and a list fold — a constant number of launches instead of N lone selections.  Same
    four shapes, same contract and same bits as ``sparse=True`` states them for RandK (unselected
    elements of the in-place operand are not written); any other compressor or shape raises
    ``NotImplementedError``.

    ``clients=[...]`` runs a SAMPLED round (partial participation; the ``_sampled`` entries): ``a`` holds
    the [n, D] gradients of the n participants, in order, and participant i is client ``clients[i]`` of
    the ``N_total`` resident ones.  An operand named in ``indexed`` is an [N_total, D] state matrix whose
    row for participant i is row ``clients[i]``; the others stay [n, D] in participant order, like the
    patterns, ``weights`` and ``pnorms_out``.  Draws are those of client ``client0 + clients[i]``, so a
    client's row does not depend on who else takes part, and rows of an indexed operand outside
    ``clients`` are neither read nor written."""

    def __init__(self, compressor: Compressor, device=None, seed=None):
        _lib.require_gpu()
        self.comp = compressor
        self.device = _device(device)
        self.seed = seed

    def params(self):
        prm, keep = self.comp.codec_params(self.device)
        if self.seed is not None:
            prm.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return prm, keep

    def workspace_bytes(self, n, d, sparse=False, compat=False, batched=False, one_read=False, sampled=False):
        """``sparse``: flc_randk_shift_reduce's workspace (``compat``: with numpy-stream index rows);
        ``batched``: flc_topk_shift_reduce's (the selection state, then the [n, d] difference matrix);
        ``one_read``: flc_dither_shift_reduce's (the sparse QSGD pipeline's state, no [n, d] matrix);
        ``sampled``: the ``clients=`` form of the general, ``sparse`` or ``batched`` round (n participants)."""
        if sampled and one_read:
            raise NotImplementedError("ShiftUplinkReducer: the one-read QSGD round has no sampled form")
        prm, _ = self.params()
        pat = _lib.FlcPattern()
        pat.d_randk_idx = 1 if compat else None                 # (the size query only tells the modes apart)
        return _shift_workspace_size(_lib.load(), _shift_mode(sparse, batched, one_read), prm, pat, n, d, sampled)

    def __call__(self, a, b, *, scale=1.0, base=None, msg_out=None, alpha=None, shift=None, shift_out=None, out=None,
                 weights=None, divisor=None, client0=0, randk_idx=None, uniforms=None, lazy_u=None, pnorms_out=None,
                 stream=None, sparse=False, randk_counts=None, batched=False, one_read=False, clients=None, indexed=None):
        """a, b: [N, D] fp32 row-contiguous device matrices (local gradients; shifts / previous
        estimators / previous gradients).  ``base``: None, [N, D], or ONE [D] vector for every row
        (MARINA's g_prev).  ``msg_out``: None (the messages are not stored) or [N, D]; it may be ``b``
        / ``base`` (EF21 in place).  ``alpha`` with ``shift`` [N, D]: the updated shifts go to
        ``shift_out`` (a new matrix when None; it may be ``shift`` / ``b``: DIANA in place).
        Patterns, ``weights``, ``divisor`` and ``stream`` as in ``UplinkReducer``; ``lazy_u`` is read
        back to the host once for the wire statistics.  Returns ``(out, msg_out, shift_out)``.  The
        compressor's wire statistics advance as N consecutive ``compressShift`` calls would leave them.
        The vector kernel needs every operand 16-byte aligned with a row stride that is a multiple
        of 4; anything else runs the scalar kernel (same bits).  ``sparse=True``: the class docstring's
        RandK round (``NotImplementedError`` when the library refuses the codec or the shape — no
        silent fallback; ``pnorms_out`` is a ``ValueError``); ``randk_counts``: its device draws' chunk
        counts from ``UplinkReducer.randk_counts(n, d, client0)`` with the same seed, as in ``UplinkReducer``.
        ``batched=True``: the class docstring's TopK round (``NotImplementedError`` for another
        compressor, before any operand is looked at, or when the library refuses the shape — no silent
        fallback; together with ``sparse``, ``pnorms_out`` or ``randk_counts`` it is a ``ValueError``).
        ``one_read=True``: the QSGD round (standard dithering with p = 2, device draws) through
        ``flc_dither_shift_reduce``: a and b read once by the sparse QSGD pipeline over a - b, the
        in-place operand written at the nonzero elements of C(a - b) only.  It takes the in-place DIANA
        shape (``scale`` 1), the in-place EF21 shape and the plain fold (``scale`` 1) under the
        untouched-elements contract of ``sparse=True`` with "selected" read as "encoded value nonzero";
        ``pnorms_out`` is supported.  ``NotImplementedError`` for another compressor, before any operand
        is looked at, or when the library refuses the call (MARINA's shared base, a dense path hint, a
        candidate share past the staging capacity) — no silent fallback; together with ``sparse``,
        ``batched``, ``uniforms`` or ``randk_counts`` it is a ``ValueError``.
        ``clients``: a host sequence of n distinct client ids, the class docstring's sampled round
        (``ValueError`` for a duplicate or an id outside the state matrices).  ``indexed``: a tuple of
        names from ("b", "base", "msg_out", "shift", "shift_out"), the operands that are [N_total, D]
        state matrices; by default every per-row operand passed other than ``a``, except a shared [D]
        base.  An indexed ``shift`` needs ``shift_out`` (the state is updated in place, or into a given
        matrix).  ``client0`` still offsets the key; ``sparse`` / ``batched`` route to their sampled
        entries; ``one_read`` or ``randk_counts`` with ``clients`` raise ``NotImplementedError``."""
        if clients is None and indexed is not None:
            raise ValueError("ShiftUplinkReducer: indexed names operands of a sampled round (clients=...)")
        if clients is not None and (one_read or randk_counts is not None):
            raise NotImplementedError("ShiftUplinkReducer: a sampled round (clients=...) has no one_read form and takes no "
                                      "randk_counts (they are keyed by position, not by client id)")
        if one_read:
            if sparse or batched or uniforms is not None or randk_counts is not None:
                raise ValueError("ShiftUplinkReducer: one_read=True takes no sparse, batched, uniforms or randk_counts "
                                 "(the QSGD round with device draws)")
            if self.comp.compressorType != CompressorType.STANDARD_DITHERING_FP32 or getattr(self.comp, "p", None) != 2:
                raise NotImplementedError("ShiftUplinkReducer: one_read=True is the QSGD round (standard dithering with "
                                          f"p = 2, flc_dither_shift_reduce); this compressor is {self.comp.compressorType}"
                                          f"{' with p = %s' % self.comp.p if hasattr(self.comp, 'p') else ''}")
        if batched:
            if sparse or pnorms_out is not None or randk_counts is not None:
                raise ValueError("ShiftUplinkReducer: batched=True takes no sparse, pnorms_out or randk_counts "
                                 "(TopK draws nothing and uses no norm)")
            if self.comp.compressorType != CompressorType.TOPK_COMPRESSOR:
                raise NotImplementedError("ShiftUplinkReducer: batched=True is the TOPK round (flc_topk_shift_reduce); "
                                          f"this compressor is {self.comp.compressorType}")
        if sparse and pnorms_out is not None:
            raise ValueError("ShiftUplinkReducer: pnorms_out is not available with sparse=True (RandK uses no norm)")
        if randk_counts is not None and not sparse:
            raise ValueError("ShiftUplinkReducer: randk_counts is read by the sparse round only (sparse=True)")
        args = (a, b, scale, base, msg_out, alpha, shift, shift_out, out, weights, divisor, client0, randk_idx, uniforms,
                lazy_u, pnorms_out, sparse, randk_counts, batched, one_read, clients, indexed)
        if stream is not None:
            if stream.device != self.device:
                raise ValueError(f"stream is on {stream.device}, the reducer runs on {self.device}")
            with torch.cuda.stream(stream):
                return self._run(*args)
        return self._run(*args)

    def _run(self, a, b, scale, base, msg_out, alpha, shift, shift_out, out, weights, divisor, client0, randk_idx,
             uniforms, lazy_u, pnorms_out, sparse=False, randk_counts=None, batched=False, one_read=False, clients=None,
             indexed=None):
        lib = _lib.load()
        who = "ShiftUplinkReducer"
        mode = _shift_mode(sparse, batched, one_read)
        entry, takes_pat, _, takes_pnorms = _SHIFT_MODES[mode]
        sampled = clients is not None
        if sampled:
            entry += "_sampled"
        for name in ("flc_encode_shift_reduce", entry):
            if not hasattr(lib, name):
                raise NotImplementedError(f"this library build has no {name}")
        if sampled and alpha is not None and shift_out is None and (indexed is None or "shift" in indexed):
            raise ValueError(f"{who}: an indexed shift is updated in place or into a given matrix (pass shift_out)")
        if mode and alpha is not None and shift_out is None:
            raise NotImplementedError(f"{who}: {mode}=True updates the shift in place (shift_out = shift = b)")
        dev = self.device
        for name, v in (("a", a), ("b", b), ("base", base), ("msg_out", msg_out), ("shift", shift),
                        ("shift_out", shift_out), ("out", out)):
            if v is not None and (not torch.is_tensor(v) or not _is_fp32_device(v)):
                raise TypeError(f"{who}: {name} must be an fp32 device tensor")
        if a.dim() != 2:
            raise ValueError(f"{who}: a must be an [N, D] matrix")
        n, d = a.shape
        ids, idx_names, n_total = None, (), n
        if sampled:
            ids = _client_ids(who, clients, n)
            given = {"b": b, "base": base, "msg_out": msg_out, "shift": shift, "shift_out": shift_out}
            if indexed is None:
                idx_names = tuple(k for k, v in given.items() if v is not None and not (k == "base" and v.dim() == 1))
            else:
                idx_names = tuple(indexed)
                for k in idx_names:
                    if k not in _IDX_BITS:
                        raise ValueError(f"{who}: indexed names {sorted(_IDX_BITS)}, got {k!r}")
                    if given[k] is None:
                        raise ValueError(f"{who}: indexed operand {k} is not given")
                    if k == "base" and base.dim() == 1:
                        raise ValueError(f"{who}: a shared [D] base is never indexed")
            totals = {int(given[k].shape[0]) for k in idx_names if given[k].dim() == 2}
            if len(totals) > 1:
                raise ValueError(f"{who}: the indexed operands must all be [N_total, {d}] (got row counts {sorted(totals)})")
            n_total = totals.pop() if totals else (max(ids) + 1 if ids else 1)
            if ids and max(ids) >= n_total:
                raise ValueError(f"{who}: client id {max(ids)} outside the [{n_total}, {d}] state matrices")

        def rows(name, v):
            if name in idx_names:
                return _row_matrix(who, name, v, n_total, d, like=" (an indexed state matrix)")
            return _row_matrix(who, name, v, n, d, like=" like a")
        sr = _lib.FlcShiftRows()
        sr.d_a, sr.lda = rows("a", a)
        sr.d_b, sr.ldb = rows("b", b)
        if base is not None:
            sr.d_base, sr.ldbase = _base_rows(who, base, n, d, rows)
        if alpha is not None and shift is None:
            raise ValueError("ShiftUplinkReducer: alpha given without a shift matrix")
        if alpha is None and shift_out is not None:
            raise ValueError("ShiftUplinkReducer: shift_out given without alpha")
        if msg_out is not None:
            sr.d_msg, sr.ldmsg = rows("msg_out", msg_out)
        if alpha is not None:
            sr.d_shift_in, sr.ldin = rows("shift", shift)
            if shift_out is None:
                shift_out = torch.empty((n, d), dtype=torch.float32, device=dev)
            sr.d_shift_out, sr.ldout = rows("shift_out", shift_out)
        sr.msg_scale = float(np.float32(scale))
        sr.shift_alpha = float(np.float32(alpha if alpha is not None else 0.0))
        if out is None:
            out = torch.empty(d, dtype=torch.float32, device=dev)
        elif out.numel() != d or not out.is_contiguous():
            raise ValueError(f"ShiftUplinkReducer: out must be a contiguous [{d}] vector")
        if n == 0:
            return out.zero_(), msg_out, shift_out               # no clients (algorithms.py:2117-2118)
        prm, keep = self.params()
        pat = _lib.FlcPattern()
        pat.client0 = int(client0)
        t = self.comp.compressorType
        lazy_host = None
        if t == CompressorType.LAZY_COMPRESSOR and lazy_u is not None:
            lazy_u = torch.as_tensor(lazy_u, dtype=torch.float64)
            if lazy_u.numel() != n:
                raise ValueError(f"lazy_u must hold {n} draws")
            lazy_host = [float(x) for x in lazy_u.detach().cpu().reshape(-1).tolist()]
            lazy_u = lazy_u.to(dev).contiguous()
            keep.append(lazy_u)
        if _pattern_draws(pat, t, randk_idx, uniforms, lazy_u) and self.seed is None and self.comp.device_rng is None:
            raise ValueError("no compat pattern given and no device-RNG seed set")
        w_ptr, total = _fold_weights(weights, n, dev, keep, divisor)
        if randk_counts is not None and randk_idx is None:
            _pattern_counts(pat, randk_counts, n, d)
        if d > 0:
            vp = ctypes.c_void_p
            ws = _lib.WORKSPACE.get(dev, _shift_workspace_size(lib, mode, prm, pat, n, d, sampled))
            args = [ctypes.byref(prm)] + ([ctypes.byref(pat)] if takes_pat else []) + [ctypes.byref(sr)]
            if sampled:
                h_ids = np.asarray(ids, dtype=np.int32)
                d_ids = torch.from_numpy(h_ids).to(dev)
                keep += [h_ids, d_ids]
                rmap = _lib.FlcRowMap()
                rmap.h_ids, rmap.d_ids, rmap.n_total = h_ids.ctypes.data, d_ids.data_ptr(), n_total
                rmap.indexed = sum(_IDX_BITS[k] for k in set(idx_names))
                args.append(ctypes.byref(rmap))
            args += [n, d, vp(w_ptr), ctypes.c_float(total)]
            if takes_pnorms:
                args.append(vp(pnorms_out.data_ptr() if pnorms_out is not None else None))
            with torch.cuda.device(dev):
                rc = getattr(lib, entry)(*args, vp(out.data_ptr()), vp(ws.data_ptr()), ws.numel(), _lib.stream_ptr(dev))
            _lib.check(rc, entry)                               # (a refusal: NotImplementedError with the reason)
        for i in range(n):                                        # N compressShift calls' statistics
            if lazy_host is not None:
                self.comp.testp = lazy_host[i]
            self.comp._account(d)
        return out, msg_out, shift_out


_ELEMENTWISE = (CompressorType.IDENTICAL, CompressorType.LAZY_COMPRESSOR, CompressorType.NATURAL_COMPRESSOR_FP32,
                CompressorType.STANDARD_DITHERING_FP32, CompressorType.NATURAL_DITHERING_FP32)


class FreconUplinkReducer:
    """A FRECON round of N resident clients in one call (flc_frecon_reduce): both client messages
    from one read of the gradients, under one pattern per client (algorithms.py:1104-1119),

        u_i = C_i(G_i - H_i);   q_i = C_i(G_i - P_i);   H_i += alpha * u_i   (in place)
        u_avg = (sum_i w_i u_i) / sum(w);   q_avg = (sum_i w_i q_i) / sum(w)

    and, with ``server``, the server's combination (1124-1176, 1181):

        result  = q_avg + (1 - lambda_) * g_server_prev + lambda_ * (u_avg + h_prev)
        h_prev' = h_prev + alpha_update * u_avg

    Every row and both folds carry the bits of N ``freconStep(in_place=True)`` calls and
    ``reduce_rows`` of their messages.  The elementwise codecs (ident, lazy, natural, standard and
    natural dithering) run the one-kernel entry; RandK, TopK and Rank-K are composed from
    ``ShiftUplinkReducer`` — the in-place DIANA shape over ``(G, H)``, then the plain fold over
    ``(G, P)`` with the same seed, ``client0`` and patterns — followed by the tail in torch
    (``sparse`` / ``batched`` go to those two calls under their own rules; for an elementwise codec
    they raise ``NotImplementedError`` like ``ShiftUplinkReducer``).  The compressor's wire
    statistics advance as 2 N ``compressVector`` calls."""

    def __init__(self, compressor: Compressor, device=None, seed=None):
        _lib.require_gpu()
        self.comp = compressor
        self.device = _device(device)
        self.seed = seed

    def params(self):
        prm, keep = self.comp.codec_params(self.device)
        if self.seed is not None:
            prm.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return prm, keep

    def workspace_bytes(self, n, d):
        prm, _ = self.params()
        return _lib.load().flc_frecon_reduce_workspace_size(ctypes.byref(prm), n, d)

    def __call__(self, G, H, P, alpha, *, server=None, weights=None, divisor=None, client0=0, randk_idx=None,
                 uniforms=None, lazy_u=None, out_u=None, out_q=None, pnorms_u_out=None, pnorms_q_out=None, stream=None,
                 sparse=False, batched=False, clients=None):
        """G, H, P: [N, D] fp32 row-contiguous device matrices (the local gradients, the clients'
        shifts — updated in place — and the gradients at the previous iterate).  ``server``: None or
        a dict with ``lambda_``, ``g_server_prev`` and ``h_prev`` ([D] device vectors), optionally
        ``alpha_update`` (then h_prev' is formed: into ``h_prev_out`` when given, which may be
        ``h_prev`` itself, else into a new vector) and ``out`` for the result.  Patterns, ``weights``,
        ``divisor``, ``client0`` and ``stream`` as in ``ShiftUplinkReducer``.  Returns
        ``(u_avg, q_avg, result, h_prev_new)``, the last two None without ``server`` /
        ``alpha_update``.  ``clients`` (a sampled round) raises ``NotImplementedError``: flc_frecon_reduce
        has no sampled form."""
        if clients is not None:
            raise NotImplementedError("FreconUplinkReducer: the two-message round has no sampled form (clients=...)")
        args = (G, H, P, alpha, server, weights, divisor, client0, randk_idx, uniforms, lazy_u, out_u, out_q,
                pnorms_u_out, pnorms_q_out, sparse, batched)
        if stream is not None:
            if stream.device != self.device:
                raise ValueError(f"stream is on {stream.device}, the reducer runs on {self.device}")
            with torch.cuda.stream(stream):
                return self._run(*args)
        return self._run(*args)

    def _tail_operands(self, who, server, d):
        for key in ("lambda_", "g_server_prev", "h_prev"):
            if key not in server:
                raise ValueError(f"{who}: server needs {key!r}")
        unknown = set(server) - {"lambda_", "g_server_prev", "h_prev", "alpha_update", "h_prev_out", "out"}
        if unknown:
            raise ValueError(f"{who}: unknown server keys {sorted(unknown)}")
        if server.get("h_prev_out") is not None and server.get("alpha_update") is None:
            raise ValueError(f"{who}: h_prev_out given without alpha_update")
        for key in ("g_server_prev", "h_prev", "h_prev_out", "out"):
            v = server.get(key)
            if v is None:
                continue
            if not torch.is_tensor(v) or not _is_fp32_device(v):
                raise TypeError(f"{who}: server[{key!r}] must be an fp32 device tensor")
            if v.dim() != 1 or v.numel() != d or not v.is_contiguous():
                raise ValueError(f"{who}: server[{key!r}] must be a contiguous [{d}] vector")

    def _run(self, G, H, P, alpha, server, weights, divisor, client0, randk_idx, uniforms, lazy_u, out_u, out_q,
             pnorms_u_out, pnorms_q_out, sparse, batched):
        lib = _lib.load()
        who = "FreconUplinkReducer"
        dev = self.device
        for name, v in (("G", G), ("H", H), ("P", P), ("out_u", out_u), ("out_q", out_q)):
            if v is not None and (not torch.is_tensor(v) or not _is_fp32_device(v)):
                raise TypeError(f"{who}: {name} must be an fp32 device tensor")
        if G.dim() != 2:
            raise ValueError(f"{who}: G must be an [N, D] matrix")
        n, d = G.shape
        if server is not None:
            self._tail_operands(who, server, d)
        for name, v in (("out_u", out_u), ("out_q", out_q)):
            if v is not None and (v.numel() != d or not v.is_contiguous()):
                raise ValueError(f"{who}: {name} must be a contiguous [{d}] vector")
        if self.comp.compressorType not in _ELEMENTWISE:
            return self._composed(G, H, P, alpha, server, weights, divisor, client0, randk_idx, uniforms, lazy_u, out_u,
                                  out_q, pnorms_u_out, pnorms_q_out, sparse, batched)
        if sparse or batched:
            raise NotImplementedError(f"{who}: sparse / batched are RandK's and TopK's rounds; this compressor is "
                                      f"{self.comp.compressorType}")
        if not hasattr(lib, "flc_frecon_reduce"):
            raise NotImplementedError("this library build has no flc_frecon_reduce")

        def rows(name, v):
            return _row_matrix(who, name, v, n, d, like=" like G")
        fr = _lib.FlcFreconRows()
        fr.d_a, fr.lda = rows("G", G)
        fr.d_h, fr.ldh = rows("H", H)
        fr.d_p, fr.ldp = rows("P", P)
        fr.shift_alpha = float(np.float32(alpha))
        if out_u is None:
            out_u = torch.empty(d, dtype=torch.float32, device=dev)
        if out_q is None:
            out_q = torch.empty(d, dtype=torch.float32, device=dev)
        result = h_new = None
        srv = None
        if server is not None:
            lam = float(server["lambda_"])
            result = server.get("out")
            if result is None:
                result = torch.empty(d, dtype=torch.float32, device=dev)
            srv = _lib.FlcFreconServer()
            srv.d_g_server_prev = server["g_server_prev"].data_ptr()
            srv.d_h_prev = server["h_prev"].data_ptr()
            srv.lambda_ = float(np.float32(lam))
            srv.one_minus_lambda = float(np.float32(1.0 - lam))           # the double difference, cast once
            srv.d_result = result.data_ptr()
            if server.get("alpha_update") is not None:
                h_new = server.get("h_prev_out")
                if h_new is None:
                    h_new = torch.empty(d, dtype=torch.float32, device=dev)
                srv.alpha_update = float(np.float32(server["alpha_update"]))
                srv.d_h_prev_out = h_new.data_ptr()
        if n == 0:                                                   # no clients (algorithms.py:2117-2118)
            return out_u.zero_(), out_q.zero_(), (result.zero_() if result is not None else None), None
        prm, keep = self.params()
        pat = _lib.FlcPattern()
        pat.client0 = int(client0)
        t = self.comp.compressorType
        lazy_host = None
        if t == CompressorType.LAZY_COMPRESSOR and lazy_u is not None:
            lazy_u = torch.as_tensor(lazy_u, dtype=torch.float64)
            if lazy_u.numel() != n:
                raise ValueError(f"lazy_u must hold {n} draws")
            lazy_host = [float(x) for x in lazy_u.detach().cpu().reshape(-1).tolist()]
            lazy_u = lazy_u.to(dev).contiguous()
            keep.append(lazy_u)
        if _pattern_draws(pat, t, randk_idx, uniforms, lazy_u) and self.seed is None and self.comp.device_rng is None:
            raise ValueError("no compat pattern given and no device-RNG seed set")
        w_ptr, total = _fold_weights(weights, n, dev, keep, divisor)
        if d > 0:
            vp = ctypes.c_void_p
            ws = _lib.WORKSPACE.get(dev, lib.flc_frecon_reduce_workspace_size(ctypes.byref(prm), n, d))
            with torch.cuda.device(dev):
                rc = lib.flc_frecon_reduce(ctypes.byref(prm), ctypes.byref(pat), ctypes.byref(fr), n, d, vp(w_ptr),
                                           ctypes.c_float(total),
                                           vp(pnorms_u_out.data_ptr() if pnorms_u_out is not None else None),
                                           vp(pnorms_q_out.data_ptr() if pnorms_q_out is not None else None),
                                           vp(out_u.data_ptr()), vp(out_q.data_ptr()),
                                           ctypes.byref(srv) if srv is not None else None,
                                           vp(ws.data_ptr()), ws.numel(), _lib.stream_ptr(dev))
            _lib.check(rc, "flc_frecon_reduce")
        for i in range(n):                                            # u_i then q_i: 2 N compressVector calls
            if lazy_host is not None:
                self.comp.testp = lazy_host[i]
            self.comp._account(d)
            self.comp._account(d)
        return out_u, out_q, result, h_new

    def _composed(self, G, H, P, alpha, server, weights, divisor, client0, randk_idx, uniforms, lazy_u, out_u, out_q,
                  pnorms_u_out, pnorms_q_out, sparse, batched):
        """RandK / TopK / Rank-K: the two rounds of the existing reducer, then the tail in torch."""
        red = ShiftUplinkReducer(self.comp, device=self.device, seed=self.seed)
        kw = dict(weights=weights, divisor=divisor, client0=client0, randk_idx=randk_idx, uniforms=uniforms,
                  lazy_u=lazy_u, sparse=sparse, batched=batched)
        u, _, _ = red(G, H, alpha=alpha, shift=H, shift_out=H, out=out_u, pnorms_out=pnorms_u_out, **kw)
        q, _, _ = red(G, P, out=out_q, pnorms_out=pnorms_q_out, **kw)
        result = h_new = None
        if server is not None:
            lam = float(server["lambda_"])
            h_prev = server["h_prev"]
            result = q + (1.0 - lam) * server["g_server_prev"] + lam * (u + h_prev)     # algorithms.py:1171
            if server.get("out") is not None:
                result = server["out"].copy_(result)
            if server.get("alpha_update") is not None:
                h_new = h_prev + float(server["alpha_update"]) * u                       # algorithms.py:1181
                if server.get("h_prev_out") is not None:
                    h_new = server["h_prev_out"].copy_(h_new)
        return u, q, result, h_new


class PayloadReducer:
    """Server side of the wire format: out = (sum_i w_i * decode(payload_i)) / sum(w), folded in
    client order straight from the messages (flc_unpack_reduce) — the same bits as
    flc_encode_reduce of the rows the payloads were packed from."""

    def __init__(self, compressor: Compressor, device=None):
        _lib.require_gpu()
        self.comp = compressor
        self.device = _device(device)

    def __call__(self, payloads, d=None, out=None, weights=None, divisor=None):
        """payloads: [N, ld] uint8 device tensor (rows 16-byte aligned, ld % 16 == 0) or a list of
        uint8 device tensors."""
        lib = _lib.load()
        dev = self.device
        d = self.comp._dim(d)
        prm, keep = self.comp.codec_params(dev)
        if torch.is_tensor(payloads) and payloads.dim() == 2:
            n, ld = payloads.shape
            if payloads.stride(1) != 1 or payloads.stride(0) % 16 or payloads.data_ptr() % 16:
                raise ValueError("payload rows must be contiguous and 16-byte aligned")
            base, ldb, ptrs = payloads.data_ptr(), payloads.stride(0), None
        else:
            n = len(payloads)
            for p in payloads:
                if p.data_ptr() % 16:
                    raise ValueError("payloads must be 16-byte aligned")
            base, ldb, ptrs = None, 0, _pointer_table(payloads, dev, keep)
        if out is None:
            out = torch.empty(d, dtype=torch.float32, device=dev)
        w_ptr, total = _fold_weights(weights, n, dev, keep, divisor)
        ws_bytes = lib.flc_unpack_reduce_workspace_size(ctypes.byref(prm), n, d)
        ws = _lib.WORKSPACE.get(dev, ws_bytes)
        with torch.cuda.device(dev):
            rc = lib.flc_unpack_reduce(ctypes.byref(prm), ctypes.c_void_p(base), ldb, ctypes.c_void_p(ptrs), n, d,
                                       ctypes.c_void_p(w_ptr), ctypes.c_float(total), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "flc_unpack_reduce")
        return out


class ShiftPayloadReducer:
    """Server side of a shifted round on the wire (flc_unpack_shift_reduce):

        msg_i = base_i + decode(payload_i) * scale;   out = (sum_i w_i * msg_i) / sum(w)

    folded in client order straight from the messages.  For payloads made by
    ``Compressor.compressShiftPayload`` it leaves the ``out`` and the ``msg_out`` rows of
    ``ShiftUplinkReducer`` (flc_encode_shift_reduce) over the rows they were packed from, bit for
    bit.  Dense formats run one tile-owner pass (k_unpack_shift_accum); RandK / TopK payloads go row
    by row through a dense workspace row (the dense round's bits, not a fast path).  Rank-K raises
    ``NotImplementedError``."""

    def __init__(self, compressor: Compressor, device=None):
        _lib.require_gpu()
        self.comp = compressor
        self.device = _device(device)

    def __call__(self, payloads, d=None, *, scale=1.0, base=None, msg_out=None, out=None, weights=None, divisor=None):
        """payloads: [N, ld] uint8 device tensor (rows 16-byte aligned, ld % 16 == 0) or a list of N
        16-byte aligned uint8 device tensors.  ``base``: None, [N, D], or ONE [D] vector for every row
        (MARINA's g_prev).  ``msg_out``: None or [N, D]; it may be ``base`` (EF21's server mirror in
        place).  ``weights`` / ``divisor`` as in ``PayloadReducer``.  Returns ``out``."""
        lib = _lib.load()
        if not hasattr(lib, "flc_unpack_shift_reduce"):
            raise NotImplementedError("this library build has no flc_unpack_shift_reduce")
        dev = self.device
        d = self.comp._dim(d)
        prm, keep = self.comp.codec_params(dev)
        pr = _lib.FlcPayloadRows()
        if torch.is_tensor(payloads) and payloads.dim() == 2:
            n = payloads.shape[0]
            if payloads.dtype != torch.uint8 or not payloads.is_cuda:
                raise TypeError("ShiftPayloadReducer: payloads must be a uint8 device tensor")
            if payloads.stride(1) != 1 or payloads.stride(0) % 16 or payloads.data_ptr() % 16:
                raise ValueError("payload rows must be contiguous and 16-byte aligned")
            pr.d_payloads, pr.ld_bytes = payloads.data_ptr(), payloads.stride(0)
        else:
            payloads = list(payloads)
            n = len(payloads)
            nbytes = int(lib.flc_payload_bytes(ctypes.byref(prm), d))
            for p in payloads:
                if not torch.is_tensor(p) or p.dtype != torch.uint8 or not p.is_cuda:
                    raise TypeError("ShiftPayloadReducer: payloads must be uint8 device tensors")
                if p.data_ptr() % 16 or not p.is_contiguous() or p.numel() < nbytes:
                    raise ValueError(f"payloads must be contiguous, 16-byte aligned and hold {nbytes} bytes")
            if n:
                pr.d_payload_ptrs = _pointer_table(payloads, dev, keep)
        who = "ShiftPayloadReducer"

        def rows(name, v):
            if not _is_fp32_device(v):
                raise TypeError(f"{who}: {name} must be an fp32 device tensor")
            return _row_matrix(who, name, v, n, d)
        if base is not None:
            if base.dim() == 1 and not _is_fp32_device(base):
                raise TypeError(f"{who}: base must be an fp32 device tensor")
            pr.d_base, pr.ldbase = _base_rows(who, base, n, d, rows)
        if msg_out is not None:
            pr.d_msg, pr.ldmsg = rows("msg_out", msg_out)
        pr.msg_scale = float(np.float32(scale))
        if out is None:
            out = torch.empty(d, dtype=torch.float32, device=dev)
        elif out.dtype != torch.float32 or not out.is_cuda or out.numel() != d or not out.is_contiguous():
            raise ValueError(f"ShiftPayloadReducer: out must be a contiguous fp32 device [{d}] vector")
        w_ptr, total = _fold_weights(weights, n, dev, keep, divisor)
        ws_bytes = lib.flc_unpack_shift_reduce_workspace_size(ctypes.byref(prm), n, d)
        ws = _lib.WORKSPACE.get(dev, ws_bytes)
        with torch.cuda.device(dev):
            rc = lib.flc_unpack_shift_reduce(ctypes.byref(prm), ctypes.byref(pr), n, d, ctypes.c_void_p(w_ptr),
                                             ctypes.c_float(total), ctypes.c_void_p(out.data_ptr()),
                                             ctypes.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, "flc_unpack_shift_reduce")
        return out
