"""Client steps of the compressed algorithms on the shift codecs.

Each helper is the torch expression of the reference's ``localGradientEvaluation`` after the local
gradient is known, executed as ONE ``flc_encode_shift`` call (``Compressor.compressShift``): the
compressed difference is never materialised for the elementwise codecs, and the shift / estimator
update is written in the same pass.  Results are bit-identical to the reference's expressions
(tests/test_gpu_shift.py).  Wire statistics advance exactly as the reference's compressVector call.
"""


def dianaStep(compressor, grad_cur, h, alpha, in_place=False):
    """DIANA (algorithms.py:1383-1391), also FRECON's / COFIG's u_i (1104-1110, 1265-1269):
    ``m_i = C(grad - h); h = h + alpha * m_i``.  Returns ``(m_i, h_new)``; ``in_place`` writes
    h_new over ``h`` (the reference rebinds a new tensor: keep the default unless h is owned)."""
    return compressor.compressShift(grad_cur, h, alpha=alpha, shift=h, shift_out=h if in_place else None)


def ef21Step(compressor, grad_cur, g_prev, in_place=False):
    """EF21 (algorithms.py:1506-1517): ``g_next = g_prev + C(grad - g_prev) * mult`` with
    ``mult = 1 / (1 + w)`` for an unbiased (non-contraction) codec, else 1."""
    mult = 1.0
    if not compressor.isContractionCompressor():
        mult = 1.0 / (1.0 + compressor.getW())
    msg, _ = compressor.compressShift(grad_cur, g_prev, scale=mult, base=g_prev, out=g_prev if in_place else None)
    return msg


def marinaStep(compressor, grad_cur, grad_prev, g_prev):
    """MARINA / PP-MARINA (algorithms.py:537, 691): ``g_next = g_prev + C(grad_cur - grad_prev)``."""
    msg, _ = compressor.compressShift(grad_cur, grad_prev, base=g_prev)
    return msg


def cofigStep(compressor, grad_cur, h, alpha, in_place=False):
    """COFIG's client step (algorithms.py:1265-1269): ``u_i = C(grad - h_i); h_i += alpha * u_i`` —
    ``dianaStep`` under its own name.  Returns ``(u_i, h_new)``."""
    return dianaStep(compressor, grad_cur, h, alpha, in_place=in_place)


def freconStep(compressor, grad_cur, h, grad_prev, alpha, in_place=False):
    """FRECON's client step (algorithms.py:1104-1119): ``u_i = C(grad - h_i); h_i += alpha * u_i`` and
    ``q_i = C(grad - grad_prev)`` with ``grad_prev`` the gradient at the server's previous iterate,
    both under the one pattern already generated — one ``dianaStep`` plus one
    ``compressShift(grad_cur, grad_prev)``.  Returns ``(u_i, h_new, q_i)``; the wire statistics
    advance twice, ``last_need_to_send_advance`` holding one message's count as after each of the
    reference's two ``compressVector`` calls."""
    u, h_new = dianaStep(compressor, grad_cur, h, alpha, in_place=in_place)
    q, _ = compressor.compressShift(grad_cur, grad_prev)
    return u, h_new, q


# -- the same steps emitting the message the client sends (flc_pack_shift) -------------------------
def dianaStepWire(compressor, grad_cur, h, alpha, in_place=False):
    """``dianaStep`` on the wire: returns ``(payload, h_new)`` — the payload decodes to ``m_i``
    (``decompressShiftPayload(payload)``), written in the pass that updates the shift."""
    payload, _, h_new = compressor.compressShiftPayload(grad_cur, h, alpha=alpha, shift=h,
                                                        shift_out=h if in_place else None)
    return payload, h_new


def ef21StepWire(compressor, grad_cur, g_prev, in_place=False):
    """``ef21Step`` on the wire: returns ``(payload, g_next)``; the server mirror applies
    ``decompressShiftPayload(payload, scale=mult, base=g_prev)`` with the same ``mult``."""
    mult = 1.0
    if not compressor.isContractionCompressor():
        mult = 1.0 / (1.0 + compressor.getW())
    payload, msg, _ = compressor.compressShiftPayload(grad_cur, g_prev, scale=mult, base=g_prev,
                                                      out=g_prev if in_place else None, message=True)
    return payload, msg


def marinaStepWire(compressor, grad_cur, grad_prev):
    """MARINA's client on the wire: the payload of ``C(grad_cur - grad_prev)`` and nothing else (the
    server adds it to its ``g_prev``: ``decompressShiftPayload(payload, base=g_prev)``)."""
    payload, _, _ = compressor.compressShiftPayload(grad_cur, grad_prev)
    return payload


# -- a whole round of N resident clients in one call (flc_encode_shift_reduce) --------------------
def _uplink(compressor, like, seed):
    from .fused import ShiftUplinkReducer
    if seed is None and compressor.device_rng is not None:
        seed = compressor.device_rng[0]
    return ShiftUplinkReducer(compressor, device=like.device, seed=seed)


def dianaUplink(compressor, G, H, alpha, *, seed=None, **kw):
    """The DIANA round of N resident clients (rows of ``G`` and ``H``), also FRECON's / COFIG's u_i:
    ``m_i = C_i(G_i - H_i); H_i += alpha * m_i`` in place, and the fold ``(sum_i w_i m_i) / sum(w)``
    is returned — the server's ``gs`` before it adds its own shift — without storing any m_i.  Same
    bits as N ``dianaStep(in_place=True)`` calls and ``reduce_rows`` of their messages.  ``kw``:
    ``ShiftUplinkReducer.__call__``'s weights / divisor / client0 / patterns / out / stream / sparse /
    batched.

    ``sparse=True`` (RandK only; anything else raises ``NotImplementedError``) runs the round through
    ``flc_randk_shift_reduce``: only the K selected elements of each ``H_i`` are read and written, work
    ~ N K instead of N D.  The untouched-elements contract: an element of ``H_i`` outside row i's
    index set keeps its stored bits (the general call stores ``h + 0`` there: the same bits unless
    ``h`` is -0, which it turns into +0); selected elements and the returned fold have the general
    call's bits whenever ``H`` holds no -0 at an unselected place — always the case for shifts that
    started as +0 and were only updated by these steps.

    ``batched=True`` (TopK only; anything else raises ``NotImplementedError``) runs the round through
    ``flc_topk_shift_reduce``: all N differences, ONE many-row selection, a sparse epilogue and a list
    fold instead of N lone selections in series.  The same untouched-elements contract and the same
    bits as stated above for ``sparse=True``.

    ``one_read=True`` (QSGD, i.e. standard dithering with p = 2, device draws; anything else raises
    ``NotImplementedError``) runs the round through ``flc_dither_shift_reduce``: ``G`` and ``H`` are read
    once by the sparse QSGD pipeline over ``G_i - H_i`` and ``H_i`` is written only where
    ``C_i(G_i - H_i)`` is nonzero.  The same contract with "selected" read as "encoded value nonzero";
    ``ef21Uplink`` takes it too.

    ``clients=[...]`` (partial participation): ``H`` is the [N_total, D] state of all resident clients and
    ``G`` the [n, D] gradients of the n participants, in order; only the rows ``H[clients[i]]`` are read
    and updated, under the draws of client ``client0 + clients[i]``.  Same bits as n in-place client
    steps on those rows; ``sparse`` / ``batched`` keep their contract, ``one_read`` raises
    ``NotImplementedError``.  ``ef21Uplink`` and ``cofigUplink`` take it the same way."""
    out, _, _ = _uplink(compressor, G, seed)(G, H, alpha=alpha, shift=H, shift_out=H, **kw)
    return out


def ef21Uplink(compressor, G, G_prev, *, seed=None, **kw):
    """The EF21 round: ``G_prev_i += C_i(G_i - G_prev_i) * mult`` in place (``mult`` as in
    ``ef21Step``) and the fold of the new estimators is returned.  ``sparse=True`` (RandK only): only
    the K selected elements of each ``G_prev_i`` are written, then the updated rows are folded densely;
    unselected elements keep their stored bits (``dianaUplink``'s contract; the fold can then differ
    from the general call's only in the sign of a zero, and only if ``G_prev`` held a -0).
    ``batched=True`` (TopK only, a contractive compressor: ``mult`` is 1): the same round through
    ``flc_topk_shift_reduce`` under the same contract."""
    mult = 1.0
    if not compressor.isContractionCompressor():
        mult = 1.0 / (1.0 + compressor.getW())
    out, _, _ = _uplink(compressor, G, seed)(G, G_prev, scale=mult, base=G_prev, msg_out=G_prev, **kw)
    return out


def marinaUplink(compressor, G_cur, G_prev_rows, g_prev, *, seed=None, **kw):
    """The MARINA / PP-MARINA compressed round: the fold of ``g_prev + C_i(G_cur_i - G_prev_rows_i)``
    with ONE shared ``g_prev`` [D] vector; no message is stored.  ``sparse=True`` (RandK only): no row is
    read outside its index set; the fold is bit-identical to the general call's without condition.
    ``batched=True`` (TopK only): the round through ``flc_topk_shift_reduce``, bit-identical as well.
    ``one_read=True`` raises ``NotImplementedError``: the one-read QSGD round does not take a shared base yet.
    ``clients=[...]`` (PP-MARINA's compressed round): both gradient matrices are fresh per round and stay
    [n, D] in participant order; nothing is indexed, only the draws are keyed by ``client0 + clients[i]``."""
    if kw.get("one_read"):
        raise NotImplementedError("marinaUplink: one_read=True (flc_dither_shift_reduce) does not take MARINA's shared "
                                  "base yet; use the general round")
    if kw.get("clients") is not None:
        kw.setdefault("indexed", ())
    out, _, _ = _uplink(compressor, G_cur, seed)(G_cur, G_prev_rows, base=g_prev, **kw)
    return out


def cofigUplink(compressor, G, H, alpha, h_prev, *, seed=None, **kw):
    """The COFIG round of N resident clients (algorithms.py:1265-1307): ``dianaUplink`` — ``H_i``
    updated in place, the fold u of the messages — returned as the server returns it, ``u + h_prev``.
    Needs no kernel of its own; ``kw`` as in ``dianaUplink``.  The server's own update,
    ``h_prev += alpha_update * u``, wants u: pass ``out=`` to keep it."""
    u = dianaUplink(compressor, G, H, alpha, seed=seed, **kw)
    return u + h_prev


def freconUplink(compressor, G, H, P, alpha, lambda_, g_server_prev, h_prev, alpha_update=None, *, seed=None,
                 h_prev_out=None, **kw):
    """The FRECON round of N resident clients (algorithms.py:1104-1176): per client
    ``u_i = C_i(G_i - H_i)``, ``q_i = C_i(G_i - P_i)`` under one pattern, ``H_i += alpha * u_i`` in
    place; both folds, and the server's
    ``q_avg + (1 - lambda_) * g_server_prev + lambda_ * (u_avg + h_prev)`` is returned.  With
    ``alpha_update`` the server shift is advanced too, ``h_prev + alpha_update * u_avg`` (1181), into
    ``h_prev_out`` (which may be ``h_prev``; default: ``h_prev`` itself, in place).  Same bits as N
    ``freconStep(in_place=True)`` calls, ``reduce_rows`` of their messages and the torch
    expressions.  Elementwise codecs run ``flc_frecon_reduce`` (one kernel, ``G`` read once per
    pass); RandK / TopK / Rank-K are composed from ``ShiftUplinkReducer``'s rounds (``sparse=True``
    / ``batched=True`` under ``dianaUplink``'s rules).  ``kw``: ``FreconUplinkReducer.__call__``'s
    weights / divisor / client0 / patterns / out_u / out_q / stream / sparse / batched.  ``clients=`` raises
    ``NotImplementedError``: flc_frecon_reduce has no sampled form."""
    from .fused import FreconUplinkReducer
    if kw.get("clients") is not None:
        raise NotImplementedError("freconUplink: the two-message round has no sampled form (clients=...)")
    kw.pop("clients", None)
    if seed is None and compressor.device_rng is not None:
        seed = compressor.device_rng[0]
    server = {"lambda_": lambda_, "g_server_prev": g_server_prev, "h_prev": h_prev}
    if alpha_update is not None:
        server["alpha_update"] = alpha_update
        server["h_prev_out"] = h_prev if h_prev_out is None else h_prev_out
    _, _, result, _ = FreconUplinkReducer(compressor, device=G.device, seed=seed)(G, H, P, alpha, server=server, **kw)
    return result
