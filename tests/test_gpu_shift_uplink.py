"""GPU parity of the fused shifted uplink (flc_encode_shift_reduce, aggregation.ShiftUplinkReducer):
a DIANA / EF21 / MARINA round of N resident clients in one call,

    msg_i = base_i + C_i(a_i - b_i) * scale;  h_i' = h_i + alpha * C_i(a_i - b_i);  out = (sum_i w_i msg_i) / sum(w)

bit-exact against the oracle (oracle.codecs.shift_step per row + reduce_plain) and against the
library's own per-row composition (N x compressShift into stored rows, then reduce_rows)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import codecs as oc
from oracle import devrng

pytestmark = pytest.mark.gpu

SEED, CLIENT0 = 2024, 3
ALPHA = 0.75
SPECS = ["ident", "bernulli:0.5", "natural", "qsgd:127", "terngrad", "std.dithering:16:inf", "nat.dithering:6:2"]
ALGOS = ["diana", "ef21", "marina"]
NS = (1, 2, 5)               # one row; exactly the ring depth; odd and above the ring depth
DS = (7, 4099, 100003)       # scalar only; vector + tail; several 8192-element tiles, ragged last tile
LAZY_U = [0.3, 0.7, 0.1, 0.9, 0.4]
DRAWN = (oc.NATURAL, oc.STD_DITHERING, oc.NAT_DITHERING)


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).ravel()


def assert_bitexact(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else want
    g, w = bits(got), bits(want)
    # NaN results must sit at the same positions; their payload / sign bit is not compared
    same = (g == w) | (np.isnan(np.asarray(got, np.float32)).ravel() & np.isnan(np.asarray(want, np.float32)).ravel())
    if not same.all():
        bad = np.nonzero(~same)[0]
        raise AssertionError(f"{bad.size} of {g.size} elements differ; first {bad[:5]}: "
                             f"{np.asarray(got).ravel()[bad[:5]]} vs {np.asarray(want).ravel()[bad[:5]]}")


@functools.lru_cache(maxsize=None)
def inputs(n, d):
    """a rows, b rows, one shared vector, compat uniforms — read-only, shared by the tests."""
    g = np.random.default_rng([n, d])
    a = g.standard_normal((n, d)).astype(np.float32)
    b = (a + g.standard_normal((n, d))).astype(np.float32)
    b[:, ::13] = a[:, ::13]                         # zero differences (out[x == 0] = 0)
    gp = g.standard_normal(d).astype(np.float32)
    u = g.random((n, d))
    for v in (a, b, gp, u):
        v.setflags(write=False)
    return a, b, gp, u


@functools.lru_cache(maxsize=None)
def dev_uniforms(client, d):
    return devrng.uniforms(SEED, client, d)


def oracle_comp(spec, d, i, mode, u):
    o = oc.OracleCompressor(spec, d)
    if o.type == oc.LAZY:
        o.testp = LAZY_U[i]
    elif o.type in DRAWN:
        o.testp = u[i] if mode == "compat" else dev_uniforms(CLIENT0 + i, d)
    return o


def ef21_mult(o):
    return 1.0 if hasattr(o, "alpha") else 1.0 / (1.0 + o.w)


def oracle_round(spec, algo, n, d, mode, weights=None):
    a, b, gp, u = inputs(n, d)
    msgs, hs = [], []
    for i in range(n):
        o = oracle_comp(spec, d, i, mode, u)
        if algo == "diana":
            m, h = oc.shift_step(o, a[i], b[i], alpha=ALPHA, h=b[i])
        elif algo == "ef21":
            m, h = oc.shift_step(o, a[i], b[i], scale=ef21_mult(o), base=b[i])
        else:
            m, h = oc.shift_step(o, a[i], b[i], base=gp)
        msgs.append(m)
        hs.append(h)
    return oc.reduce_plain(msgs, weights), msgs, hs


def lib_comp(ag, spec, d, i, mode, u):
    """The Compressor of client CLIENT0 + i holding pattern row i (what compressShift encodes with)."""
    c = ag.initCompressor(spec, d)
    o = oc.OracleCompressor(spec, d)
    if o.type == oc.LAZY:
        c.testp = LAZY_U[i]
    elif o.type in DRAWN:
        if mode == "compat":
            c.testp = torch.from_numpy(u[i].copy())
        else:
            c.device_rng = (SEED, CLIENT0 + i)
    return c


def pattern_kw(spec, n, d, mode, u):
    o = oc.OracleCompressor(spec, d)
    kw = {"client0": CLIENT0}
    if o.type == oc.LAZY:
        kw["lazy_u"] = torch.tensor(LAZY_U[:n], dtype=torch.float64, device="cuda")
    if o.type in DRAWN and mode == "compat":
        kw["uniforms"] = torch.from_numpy(u.copy()).cuda()
    return kw


def run_round(ag, spec, algo, n, d, mode, store_msg=True, **extra):
    """One fused round on fresh device copies; returns (out, messages, updated shifts, reducer)."""
    a, b, gp, u = inputs(n, d)
    ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a, b, gp))
    comp = ag.initCompressor(spec, d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    kw = pattern_kw(spec, n, d, mode, u)
    kw.update(extra)
    if algo == "diana":        # scale 1, no base, alpha, in place
        msg = torch.empty_like(ta) if store_msg else None
        out, m, h = red(ta, tb, alpha=ALPHA, shift=tb, shift_out=tb, msg_out=msg, **kw)
        assert h is tb and m is msg
    elif algo == "ef21":       # base = b, msg_out = b, scale = 1 / (1 + w)
        mult = 1.0 if comp.isContractionCompressor() else 1.0 / (1.0 + comp.getW())
        out, m, h = red(ta, tb, scale=mult, base=tb, msg_out=tb, **kw)
        assert m is tb and h is None
    else:                      # MARINA: one shared [D] base
        msg = torch.empty_like(ta) if store_msg else None
        out, m, h = red(ta, tb, base=tg, msg_out=msg, **kw)
        assert h is None
    return out, m, h, red


def modes_of(spec):
    return ("device", "compat") if oc.OracleCompressor(spec, 8).type in DRAWN else ("none",)


# ------------------------------------------------------------------------------------------------
# 1. oracle parity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("spec", SPECS)
def test_oracle_parity(ag, spec, algo, d):
    for n in NS:
        for mode in modes_of(spec):
            want_out, want_m, want_h = oracle_round(spec, algo, n, d, mode)
            out, m, h, _ = run_round(ag, spec, algo, n, d, mode)
            assert_bitexact(out, want_out)
            assert_bitexact(m, np.stack(want_m))
            if algo == "diana":
                assert_bitexact(h, np.stack(want_h))
            if n == 1:         # one row is compressShift, bit for bit
                a, b, gp, u = inputs(n, d)
                ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a[0], b[0], gp))
                c = lib_comp(ag, spec, d, 0, mode, u)
                if algo == "diana":
                    m1, h1 = c.compressShift(ta, tb, alpha=ALPHA, shift=tb)
                    assert_bitexact(h[0], h1)
                elif algo == "ef21":
                    m1, _ = c.compressShift(ta, tb, scale=ef21_mult(oc.OracleCompressor(spec, d)), base=tb)
                else:
                    m1, _ = c.compressShift(ta, tb, base=tg)
                assert_bitexact(m[0], m1)
                assert_bitexact(out, m1)           # (1 row, no weights: m / 1)


# ------------------------------------------------------------------------------------------------
# 2. the library's own per-row composition
# ------------------------------------------------------------------------------------------------
def composition(ag, spec, algo, n, d, mode, weights=None, randk_idx=None, a=None, b=None):
    """N x compressShift into stored rows, then reduce_rows: what the library offered before."""
    a0, b0, gp, u = inputs(n, d)
    a = a0 if a is None else a
    b = b0 if b is None else b
    ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a, b, gp))
    msgs = torch.empty_like(ta)
    hs = torch.empty_like(ta)
    comps = []
    for i in range(n):
        c = lib_comp(ag, spec, d, i, mode, u)
        if randk_idx is not None:
            c.S = torch.from_numpy(randk_idx[i].copy()).cuda()
        elif spec.startswith("randk"):
            c.device_rng = (SEED, CLIENT0 + i)
        if algo == "diana":
            c.compressShift(ta[i], tb[i], out=msgs[i], alpha=ALPHA, shift=tb[i], shift_out=hs[i])
        elif algo == "ef21":
            mult = 1.0 if c.isContractionCompressor() else 1.0 / (1.0 + c.getW())
            c.compressShift(ta[i], tb[i], scale=mult, base=tb[i], out=msgs[i])
        else:
            c.compressShift(ta[i], tb[i], base=tg, out=msgs[i])
        comps.append(c)
    out = ag.reduce_rows(tg, msgs, weights=weights, relative=False)
    return out, msgs, hs, comps


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("spec", SPECS)
def test_same_bits_as_per_row_composition(ag, spec, algo):
    n, d = 5, 4099
    weights = [1.0, 0.5, 2.0, 1.25, 3.0]
    for mode in modes_of(spec):
        want_out, want_m, want_h, _ = composition(ag, spec, algo, n, d, mode, weights)
        out, m, h, _ = run_round(ag, spec, algo, n, d, mode, weights=weights)
        assert_bitexact(out, want_out)
        assert_bitexact(m, want_m)
        if algo == "diana":
            assert_bitexact(h, want_h)


def tied_rows(n, d):
    """Differences with ties at the K-th magnitude: row 1 of a - b holds small integers only."""
    a, b, _, _ = inputs(n, d)
    a, b = a.copy(), b.copy()
    b[1] = 0.0
    a[1] = np.random.default_rng(5).integers(-3, 4, d).astype(np.float32)
    return a, b


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("spec,draws", [("randk:3%", "compat"), ("randk:3%", "device"), ("topk:2%", None)])
def test_selecting_codecs_match_the_composition(ag, spec, draws, algo):
    n, d = 3, 30011
    a, b = tied_rows(n, d)
    idx = None
    if draws == "compat":
        k = oc.OracleCompressor(spec, d).K
        g = np.random.default_rng(9)
        idx = np.stack([g.choice(d, k, replace=False) for _ in range(n)]).astype(np.int64)
    want_out, want_m, want_h, _ = composition(ag, spec, algo, n, d, "none", randk_idx=idx, a=a, b=b)
    ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a, b, inputs(n, d)[2]))
    comp = ag.initCompressor(spec, d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    kw = {"client0": CLIENT0}
    if idx is not None:
        kw["randk_idx"] = torch.from_numpy(idx).cuda()
    for store in (True, False):        # messages in the caller's rows, or in the workspace row
        x, y = ta.clone(), tb.clone()
        msg = torch.empty_like(x) if store else None
        if algo == "diana":
            out, m, h = red(x, y, alpha=ALPHA, shift=y, shift_out=y, msg_out=msg, **kw)
            assert_bitexact(h, want_h)
        elif algo == "ef21":
            out, m, h = red(x, y, scale=1.0 if comp.isContractionCompressor() else 1.0 / (1.0 + comp.getW()),
                            base=y, msg_out=y if store else None, **kw)
        else:
            out, m, h = red(x, y, base=tg, msg_out=msg, **kw)
        assert_bitexact(out, want_out)
        if store:
            assert_bitexact(m, want_m)
    if spec.startswith("topk"):        # the tied row kept exactly K entries
        k = oc.OracleCompressor(spec, d).K
        e = oc.OracleCompressor(spec, d).compress((a[1] - b[1]).astype(np.float32))
        assert np.count_nonzero(e) == k


def test_rank_k_matches_the_composition(ag):
    """Rank-K goes through rocSOLVER: compared within the README's 5e-5 relative."""
    n, d, spec = 3, 30000, "rank_k:2"
    want_out, want_m, want_h, _ = composition(ag, spec, "diana", n, d, "none")
    out, m, h, _ = run_round(ag, spec, "diana", n, d, "none")
    for x, y in ((out, want_out), (m, want_m), (h, want_h)):
        rel = (x - y).norm().item() / (1.0 + y.norm().item())
        print("rank_k relative difference", rel)
        assert rel <= 5e-5


# ------------------------------------------------------------------------------------------------
# 3. weights, divisor, strides and alignment
# ------------------------------------------------------------------------------------------------
def padded(t, pad):
    """The same [N, D] values in rows ``D + pad`` elements apart."""
    n, d = t.shape
    buf = torch.zeros((n, d + pad), dtype=t.dtype, device=t.device)
    buf[:, :d] = t
    return buf[:, :d]


def offset_view(t):
    """The same [N, D] values starting one element into a buffer (4-byte aligned only)."""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("spec", ["natural", "qsgd:127", "ident"])
def test_weights_divisor_strides_alignment(ag, spec):
    n, d = 5, 4099
    a, b, gp, u = inputs(n, d)
    weights = [1.0, 0.5, 2.0, 1.25, 3.0]
    ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    red = ag.ShiftUplinkReducer(ag.initCompressor(spec, d), seed=SEED)

    def go(make, **kw):
        x, y = make(ta), make(tb)
        msg, hout = make(torch.zeros_like(ta)), make(torch.zeros_like(ta))
        out, m, h = red(x, y, alpha=ALPHA, shift=y, shift_out=hout, base=y, scale=0.25, msg_out=msg, client0=CLIENT0, **kw)
        return out, m.clone(), h.clone()
    ref = go(lambda t: t.clone(), weights=weights, divisor=7.0)
    # the oracle, with the weights and the divisor
    msgs, hs = [], []
    for i in range(n):
        o = oracle_comp(spec, d, i, "device", u)
        m, h = oc.shift_step(o, a[i], b[i], scale=0.25, base=b[i], alpha=ALPHA, h=b[i])
        msgs.append(m)
        hs.append(h)
    f32 = np.float32
    acc = f32(weights[0]) * msgs[0]          # reduce_plain's fold, divided by the caller's divisor
    for i in range(1, n):
        acc = acc + f32(weights[i]) * msgs[i]
    want = acc / f32(7.0)
    assert_bitexact(ref[0], want)
    assert_bitexact(ref[1], np.stack(msgs))
    assert_bitexact(ref[2], np.stack(hs))
    for make in (lambda t: padded(t, 4),        # row stride d + 4: the vector kernel (+ scalar tail)
                 lambda t: padded(t, 3),        # row stride d + 3: the scalar kernel
                 offset_view):                  # 4-byte aligned rows: the scalar kernel
        got = go(make, weights=weights, divisor=7.0)
        for x, y in zip(got, ref):
            assert_bitexact(x, y)


# ------------------------------------------------------------------------------------------------
# 4. in place versus out of place
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["natural", "qsgd:127", "topk:2%"])
def test_in_place_equals_out_of_place(ag, spec):
    n, d = 5, 4099
    a, b, gp, u = inputs(n, d)
    ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    red = ag.ShiftUplinkReducer(ag.initCompressor(spec, d), seed=SEED)
    # DIANA: shift_out is shift is b
    o1, _, h1 = red(ta, tb.clone(), alpha=ALPHA, shift=tb.clone(), client0=CLIENT0)
    y = tb.clone()
    o2, _, h2 = red(ta, y, alpha=ALPHA, shift=y, shift_out=y, client0=CLIENT0)
    assert h2 is y
    assert_bitexact(o2, o1)
    assert_bitexact(h2, h1)
    # EF21: msg_out is base is b
    o1, m1, _ = red(ta, tb.clone(), scale=0.5, base=tb.clone(), msg_out=torch.empty_like(tb), client0=CLIENT0)
    y = tb.clone()
    o2, m2, _ = red(ta, y, scale=0.5, base=y, msg_out=y, client0=CLIENT0)
    assert m2 is y
    assert_bitexact(o2, o1)
    assert_bitexact(m2, m1)


def test_helpers(ag):
    """dianaUplink / ef21Uplink / marinaUplink are the *Step helpers over the rows, then the fold."""
    n, d, spec = 3, 4099, "natural"
    a, b, gp, u = inputs(n, d)
    ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a, b, gp))

    def comp(i):
        c = ag.initCompressor(spec, d)
        c.device_rng = (SEED, i)
        return c
    alpha = 1.0 / (1.0 + comp(0).getW())
    steps = [ag.dianaStep(comp(i), ta[i], tb[i], alpha) for i in range(n)]
    h = tb.clone()
    out = ag.dianaUplink(comp(0), ta, h, alpha)
    assert_bitexact(out, ag.reduce_rows(tg, torch.stack([s[0] for s in steps]), relative=False))
    assert_bitexact(h, torch.stack([s[1] for s in steps]))
    steps = [ag.ef21Step(comp(i), ta[i], tb[i]) for i in range(n)]
    gprev = tb.clone()
    out = ag.ef21Uplink(comp(0), ta, gprev)
    assert_bitexact(gprev, torch.stack(steps))
    assert_bitexact(out, ag.reduce_rows(tg, torch.stack(steps), relative=False))
    steps = [ag.marinaStep(comp(i), ta[i], tb[i], tg) for i in range(n)]
    out = ag.marinaUplink(comp(0), ta, tb, tg)
    assert_bitexact(out, ag.reduce_rows(tg, torch.stack(steps), relative=False))


# ------------------------------------------------------------------------------------------------
# 5. which kernels ran
# ------------------------------------------------------------------------------------------------
def test_paths(ag):
    from flpytorch_amd import _lib
    names = ("k_ew_shift_accum", "k_ew_shift", "k_norm_partials")
    _lib.profile_enable(True)
    try:
        for k in names:
            _lib.profile_collect(k)
        run_round(ag, "natural", "diana", 5, 4099, "device", store_msg=False)
        assert _lib.profile_collect("k_ew_shift_accum")[1] == 1
        assert _lib.profile_collect("k_ew_shift")[1] == 0
        run_round(ag, "qsgd:127", "ef21", 5, 100003, "device")
        assert _lib.profile_collect("k_ew_shift_accum")[1] == 1
        assert _lib.profile_collect("k_ew_shift")[1] == 0
        assert _lib.profile_collect("k_norm_partials")[1] == 1      # one norm launch for the n differences
        a, b, gp, u = inputs(3, 30011)
        red = ag.ShiftUplinkReducer(ag.initCompressor("topk:2%", 30011))
        y = torch.from_numpy(b.copy()).cuda()
        red(torch.from_numpy(a.copy()).cuda(), y, alpha=ALPHA, shift=y, shift_out=y)
        assert _lib.profile_collect("k_ew_shift_accum")[1] == 0
    finally:
        _lib.profile_enable(False)
        for k in names:
            _lib.profile_collect(k)


@pytest.mark.parametrize("spec", ["qsgd:127", "std.dithering:16:inf", "nat.dithering:6:2"])
def test_pnorms_out_are_the_differences_norms(ag, spec):
    n, d = 5, 4099
    a, b, _, _ = inputs(n, d)
    pn = torch.zeros(n, device="cuda")
    run_round(ag, spec, "diana", n, d, "device", pnorms_out=pn)
    o = oc.OracleCompressor(spec, d)
    want = np.array([o.norm((a[i] - b[i]).astype(np.float32)) for i in range(n)], dtype=np.float32)
    assert_bitexact(pn, want)


# ------------------------------------------------------------------------------------------------
# 6. the ABI's refusals, and n = 0
# ------------------------------------------------------------------------------------------------
SENTINEL = -12345.0


def test_abi_errors_leave_outputs_untouched(ag):
    from flpytorch_amd import _lib
    lib = _lib.load()
    n, d = 3, 64
    comp = ag.initCompressor("natural", d)
    prm, keep = comp.codec_params(torch.device("cuda", 0))
    prm.seed = SEED
    a = torch.ones((n, d), device="cuda")
    b = torch.full((n, d), SENTINEL, device="cuda")          # the shift rows (in place)
    base = torch.zeros(d, device="cuda")
    msg = torch.full((n, d), SENTINEL, device="cuda")
    out = torch.full((d,), SENTINEL, device="cuda")
    wsb = lib.flc_encode_shift_reduce_workspace_size(ctypes.byref(prm), n, d)
    assert wsb > 0
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    pat = _lib.FlcPattern()

    def rows(**kw):
        r = _lib.FlcShiftRows()
        r.d_a, r.lda, r.d_b, r.ldb = a.data_ptr(), d, b.data_ptr(), d
        r.msg_scale, r.shift_alpha = 1.0, 0.5
        r.d_shift_in, r.ldin, r.d_shift_out, r.ldout = b.data_ptr(), d, b.data_ptr(), d
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def call(r, prm=prm, n=n, out_ptr=out.data_ptr(), ws_bytes=wsb):
        return lib.flc_encode_shift_reduce(ctypes.byref(prm), ctypes.byref(pat), ctypes.byref(r), n, d, None,
                                           ctypes.c_float(float(n)), None, ctypes.c_void_p(out_ptr),
                                           ctypes.c_void_p(ws.data_ptr()), ws_bytes, _lib.stream_ptr())
    bad = _lib.FlcCodecParams()
    bad.codec = 99
    cases = [
        ("null a", call(rows(d_a=None)), _lib.FLC_ERR_ARG),
        ("null b", call(rows(d_b=None)), _lib.FLC_ERR_ARG),
        ("null out", call(rows(), out_ptr=None), _lib.FLC_ERR_ARG),
        ("too many rows", call(rows(), n=65536), _lib.FLC_ERR_ARG),
        ("shift_out without shift_in", call(rows(d_shift_in=None)), _lib.FLC_ERR_ARG),
        ("shift_out rows overlap", call(rows(ldout=d - 1)), _lib.FLC_ERR_ARG),
        ("msg rows overlap", call(rows(d_msg=msg.data_ptr(), ldmsg=-(d - 1))), _lib.FLC_ERR_ARG),
        ("msg is the shared base", call(rows(d_base=base.data_ptr(), ldbase=0, d_msg=base.data_ptr(), ldmsg=d)),
         _lib.FLC_ERR_ARG),
        ("msg overlaps the shared base", call(rows(d_base=msg.data_ptr() + 4 * (d + 8), ldbase=0, d_msg=msg.data_ptr(), ldmsg=d)),
         _lib.FLC_ERR_ARG),
        ("workspace one byte short", call(rows(), ws_bytes=wsb - 1), _lib.FLC_ERR_WORKSPACE),
        ("unknown codec", call(rows(), prm=bad), _lib.FLC_ERR_UNSUPPORTED),
    ]
    torch.cuda.synchronize()
    for what, rc, want in cases:
        assert rc == want, what
    for t in (out, b, msg):
        assert bool((t == SENTINEL).all())
    assert bool((base == 0).all())
    assert len(lib.flc_last_error_string()) > 0
    # and the same arguments, all in order, run
    assert call(rows(d_msg=msg.data_ptr(), ldmsg=d)) == _lib.FLC_OK
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()) and not bool((b == SENTINEL).any()) and not bool((msg == SENTINEL).any())
    del keep


def test_python_errors_and_empty_round(ag):
    d = 16
    comp = ag.initCompressor("qsgd:4", d)
    red = ag.ShiftUplinkReducer(comp, seed=1)
    x = torch.ones((2, d), device="cuda")
    with pytest.raises(TypeError):
        red(x.double(), x)
    with pytest.raises(TypeError):
        red(x.cpu(), x)
    with pytest.raises(ValueError):
        red(x, torch.ones((3, d), device="cuda"))
    with pytest.raises(ValueError):
        red(x, x, alpha=0.5)
    with pytest.raises(ValueError):
        red(x.t().contiguous().t(), x)
    with pytest.raises(ValueError):
        red(x, x, base=torch.ones(d + 1, device="cuda"))
    out, m, h = red(torch.empty((0, d), device="cuda"), torch.empty((0, d), device="cuda"),
                    out=torch.full((d,), SENTINEL, device="cuda"))
    assert bool((out == 0).all()) and m is None and h is None
    assert comp.total_input_components == 0


# ------------------------------------------------------------------------------------------------
# 7. wire statistics
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["bernulli:0.5", "qsgd:127", "topk:2%", "natural"])
def test_wire_statistics(ag, spec):
    n, d = 3, 4099
    _, _, _, comps = composition(ag, spec, "diana", n, d, "device")
    want = ag.initCompressor(spec, d)
    for c in comps:                          # three compressShift calls' worth, on one compressor
        want.total_input_components += c.last_input_advance
        want.really_need_to_send_components += c.last_need_to_send_advance
    _, _, _, red = run_round(ag, spec, "diana", n, d, "device")
    got = red.comp
    assert got.total_input_components == want.total_input_components == n * d
    assert got.really_need_to_send_components == want.really_need_to_send_components
    assert got.last_input_advance == comps[-1].last_input_advance
    assert got.last_need_to_send_advance == comps[-1].last_need_to_send_advance
