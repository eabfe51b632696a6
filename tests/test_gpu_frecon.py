"""GPU parity of FRECON's two-message uplink (flc_frecon_reduce, aggregation.FreconUplinkReducer,
freconUplink / cofigUplink): per client both messages from one read of the gradient under one pattern,

    u_i = C_i(a_i - h_i);  q_i = C_i(a_i - p_i);  h_i += alpha * u_i;  u_avg, q_avg folded in row order
    result = q_avg + (1 - lambda) * g_server_prev + lambda * (u_avg + h_prev);  h_prev' = h_prev + alpha_update * u_avg

bit-exact against the oracle (oracle.codecs.shift_step twice with one pattern + reduce_plain), against
the library's own two-call composition (flc_encode_shift_reduce: in-place DIANA over (a, h), then the
plain fold over (a, p)), and — the tail — against the torch expression evaluated on the CPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import codecs as oc
from oracle import devrng
from tests import edge_rows as er
from tests.test_gpu_shift_uplink import (CLIENT0, DS, NS, SEED, SPECS, assert_bitexact, inputs, lib_comp, modes_of,
                                         oracle_comp, pattern_kw)

pytestmark = pytest.mark.gpu

ALPHA = 0.75
WEIGHTS = [1.0, 0.5, 2.0, 1.25, 3.0]


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def same(got, want, tag):
    try:
        assert_bitexact(got, want)
    except AssertionError as e:
        raise AssertionError(f"{tag}: {e}") from None


def dithering(spec):
    return oc.OracleCompressor(spec, 8).type in (oc.STD_DITHERING, oc.NAT_DITHERING)


@functools.lru_cache(maxsize=None)
def operands(n, d):
    """a rows, h rows, p rows (the gradient at the previous iterate), compat uniforms, and the
    server's g_server_prev / h_prev vectors — read-only, shared by the tests."""
    a, h, gp, u = inputs(n, d)
    g = np.random.default_rng([n, d, 7])
    p = (a + 0.25 * g.standard_normal((n, d))).astype(np.float32)
    p[:, 5::17] = a[:, 5::17]                        # zero differences in the second message too
    hp = g.standard_normal(d).astype(np.float32)
    for v in (p, hp):
        v.setflags(write=False)
    return a, h, p, u, gp, hp


@functools.lru_cache(maxsize=None)
def oracle_round(spec, n, d, mode, weighted=False):
    """Per row shift_step twice under ONE pattern, then reduce_plain of each message set; the
    norms of both differences for the dithering codecs."""
    a, h, p, u, _, _ = operands(n, d)
    us, qs, hs, nu, nq = [], [], [], [], []
    for i in range(n):
        o = oracle_comp(spec, d, i, mode, u)
        m, h2 = oc.shift_step(o, a[i], h[i], alpha=ALPHA, h=h[i])
        q, _ = oc.shift_step(o, a[i], p[i])
        us.append(m)
        qs.append(q)
        hs.append(h2)
        if dithering(spec):
            nu.append(o.norm((a[i] - h[i]).astype(np.float32)))
            nq.append(o.norm((a[i] - p[i]).astype(np.float32)))
    w = WEIGHTS[:n] if weighted else None
    return oc.reduce_plain(us, w), oc.reduce_plain(qs, w), np.stack(hs), np.array(nu, np.float32), np.array(nq, np.float32)


def dev(*arrays):
    return tuple(torch.from_numpy(np.array(v, dtype=np.float32)).cuda() for v in arrays)


def strided(rows, ld, off=0):
    """[n, d] device matrix with row stride ld, its first row `off` floats past 16-byte alignment."""
    n, d = rows.shape
    buf = torch.zeros(n * ld + 4, dtype=torch.float32, device="cuda")
    m = buf[off:off + n * ld].view(n, ld)[:, :d]
    m.copy_(torch.from_numpy(np.array(rows)))
    assert m.data_ptr() % 16 == 4 * off and m.stride(0) == ld
    return m


def padded(*mats):
    """The matrices on the device with a row stride that is a multiple of 4: the vector kernel takes
    d // 4 groups of every row and the scalar twin the d % 4 tail (dev()'s contiguous rows of an odd d
    go through the scalar twin alone)."""
    return tuple(strided(m, (m.shape[1] + 3) // 4 * 4 + 4) for m in mats)


def two_calls(ag, spec, ta, th, tp, n, d, mode, u, **kw):
    """The library's own composition: flc_encode_shift_reduce twice with the same prm and pat."""
    red = ag.ShiftUplinkReducer(ag.initCompressor(spec, d), seed=SEED)
    pk = pattern_kw(spec, n, d, mode, u)
    pk.update(kw)
    nu, nq = (torch.zeros(n, device="cuda") for _ in range(2))
    pn = dithering(spec)
    out_u, _, _ = red(ta, th, alpha=ALPHA, shift=th, shift_out=th, pnorms_out=nu if pn else None, **pk)
    out_q, _, _ = red(ta, tp, pnorms_out=nq if pn else None, **pk)
    return out_u, out_q, nu, nq


def one_call(ag, spec, ta, th, tp, n, d, mode, u, server=None, **kw):
    comp = ag.initCompressor(spec, d)
    red = ag.FreconUplinkReducer(comp, seed=SEED)
    pk = pattern_kw(spec, n, d, mode, u)
    pk.update(kw)
    nu, nq = (torch.zeros(n, device="cuda") for _ in range(2))
    pn = dithering(spec)
    out_u, out_q, result, h_new = red(ta, th, tp, ALPHA, server=server, pnorms_u_out=nu if pn else None,
                                      pnorms_q_out=nq if pn else None, **pk)
    return out_u, out_q, nu, nq, result, h_new, comp


# ------------------------------------------------------------------------------------------------
# 1. the oracle composition and the library's two-call composition
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("spec", SPECS)
def test_oracle_and_two_call_parity(ag, spec, d):
    for n in NS:
        a, h, p, u, _, _ = operands(n, d)
        for mode in modes_of(spec):
            want_u, want_q, want_h, want_nu, want_nq = oracle_round(spec, n, d, mode)
            ta, th, tp = padded(a, h, p)                                             # the vector kernel + its tail
            got_u, got_q, nu, nq, _, _, _ = one_call(ag, spec, ta, th, tp, n, d, mode, u)
            tag = f"{spec} n={n} d={d} {mode}"
            same(th, want_h, tag)
            same(got_u, want_u, tag)
            same(got_q, want_q, tag)
            assert torch.equal(ta, dev(a)[0]) and torch.equal(tp, dev(p)[0])         # inputs untouched
            sa, sh, sp = dev(a, h, p)                                                # contiguous odd d: the scalar twin
            sc_u, sc_q, sc_nu, sc_nq, _, _, _ = one_call(ag, spec, sa, sh, sp, n, d, mode, u)
            same(sh, want_h, tag + " scalar")
            same(sc_u, want_u, tag + " scalar")
            same(sc_q, want_q, tag + " scalar")
            if dithering(spec):
                same(sc_nu, want_nu, tag + " scalar")
                same(sc_nq, want_nq, tag + " scalar")
            t2a, t2h, t2p = padded(a, h, p)
            lib_u, lib_q, lib_nu, lib_nq = two_calls(ag, spec, t2a, t2h, t2p, n, d, mode, u)
            same(th, t2h, tag)
            same(got_u, lib_u, tag)
            same(got_q, lib_q, tag)
            if dithering(spec):
                same(nu, want_nu, tag)
                same(nq, want_nq, tag)
                same(nu, lib_nu, tag)
                same(nq, lib_nq, tag)


def test_one_row_is_frecon_step(ag):
    """n = 1: the h row and both averages are freconStep's outputs (m / 1)."""
    d = 4099
    a, h, p, u, _, _ = operands(1, d)
    for spec in ("natural", "qsgd:127"):
        for mode in modes_of(spec):
            ta, th, tp = dev(a, h, p)
            got_u, got_q, *_ = one_call(ag, spec, ta, th, tp, 1, d, mode, u)
            sa, sh, sp = dev(a[0], h[0], p[0])
            c = lib_comp(ag, spec, d, 0, mode, u)
            su, sh2, sq = ag.freconStep(c, sa, sh, sp, ALPHA)
            assert_bitexact(got_u, su)
            assert_bitexact(got_q, sq)
            assert_bitexact(th[0], sh2)
            assert torch.equal(sh, dev(h[0])[0])                                      # not in place by default
            assert c.total_input_components == 2 * d


# ------------------------------------------------------------------------------------------------
# 2. the server tail: the torch expression on the CPU, h_prev' over h_prev and apart from it
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("lam", [0.0, 1.0, 0.25, 0.3])
@pytest.mark.parametrize("d", [7, 4099])
def test_server_tail_matches_torch_cpu(ag, d, lam, alias):
    n, alpha_update = 5, 0.75 * (2 / 4)
    a, h, p, u, gp, hp = operands(n, d)
    for spec in ("natural", "qsgd:127"):
        mode = "device"
        (ta, th, tp), (tg, thp) = padded(a, h, p), dev(gp, hp)
        server = {"lambda_": lam, "g_server_prev": tg, "h_prev": thp, "alpha_update": alpha_update,
                  "h_prev_out": thp if alias else None}
        got_u, got_q, _, _, result, h_new, _ = one_call(ag, spec, ta, th, tp, n, d, mode, u, server=server)
        want_u, want_q, want_h, _, _ = oracle_round(spec, n, d, mode)
        assert_bitexact(got_u, want_u)
        assert_bitexact(got_q, want_q)
        assert_bitexact(th, want_h)
        cu, cq = got_u.cpu(), got_q.cpu()
        cg, chp = torch.from_numpy(gp.copy()), torch.from_numpy(hp.copy())
        want = cq + (1.0 - lam) * cg + lam * (cu + chp)                               # algorithms.py:1171
        want_hp = chp + alpha_update * cu                                             # algorithms.py:1181
        assert_bitexact(result, want)
        assert_bitexact(h_new, want_hp)
        assert (h_new is thp) == alias
        if not alias:
            assert torch.equal(thp, dev(hp)[0])                                       # h_prev untouched
        assert torch.equal(tg, dev(gp)[0])
        # without alpha_update no shift is formed
        ta, th, tp, tg, thp = dev(a, h, p, gp, hp)
        _, _, _, _, result2, none, _ = one_call(ag, spec, ta, th, tp, n, d, mode, u,
                                                server={"lambda_": lam, "g_server_prev": tg, "h_prev": thp})
        assert none is None
        assert_bitexact(result2, want)
        assert torch.equal(thp, dev(hp)[0])


@pytest.mark.parametrize("d", [4099, 4100])            # the scalar twin (ld % 4 != 0); the vector kernel
def test_tail_without_average_outputs(ag, d):
    """The C entry with a server tail and d_u_out == d_q_out == NULL: only the result and h_prev' are
    written, with the bits of the call that also stores the averages."""
    from flpytorch_amd import _lib
    n, spec, lam, alpha_update = 5, "qsgd:127", 0.25, 0.375
    a, h, p, u, gp, hp = operands(n, d)
    ta, th, tp, tg, thp = dev(a, h, p, gp, hp)
    server = {"lambda_": lam, "g_server_prev": tg, "h_prev": thp, "alpha_update": alpha_update}
    _, _, _, _, want, want_hp, _ = one_call(ag, spec, ta, th, tp, n, d, "device", u, server=server)
    t2a, t2h, t2p = dev(a, h, p)
    lib = _lib.load()
    comp = ag.initCompressor(spec, d)
    cuda = torch.device("cuda", torch.cuda.current_device())
    prm, keep = comp.codec_params(cuda)
    prm.seed = SEED
    pat = _lib.FlcPattern()
    pat.client0 = CLIENT0
    fr = _lib.FlcFreconRows()
    fr.d_a, fr.lda, fr.d_h, fr.ldh, fr.d_p, fr.ldp = t2a.data_ptr(), d, t2h.data_ptr(), d, t2p.data_ptr(), d
    fr.shift_alpha = ALPHA
    result, h_new = torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
    srv = _lib.FlcFreconServer()
    srv.d_g_server_prev, srv.d_h_prev = tg.data_ptr(), thp.data_ptr()
    srv.lambda_, srv.one_minus_lambda = float(np.float32(lam)), float(np.float32(1.0 - lam))
    srv.d_result, srv.alpha_update, srv.d_h_prev_out = result.data_ptr(), float(np.float32(alpha_update)), h_new.data_ptr()
    ws = torch.empty(lib.flc_frecon_reduce_workspace_size(ctypes.byref(prm), n, d), dtype=torch.uint8, device="cuda")
    rc = lib.flc_frecon_reduce(ctypes.byref(prm), ctypes.byref(pat), ctypes.byref(fr), n, d, None, ctypes.c_float(n),
                               None, None, None, None, ctypes.byref(srv), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                               _lib.stream_ptr(cuda))
    _lib.check(rc, "flc_frecon_reduce")
    torch.cuda.synchronize()
    assert_bitexact(result, want)
    assert_bitexact(h_new, want_hp)
    assert_bitexact(t2h, th)
    del keep


# ------------------------------------------------------------------------------------------------
# 3. weights and divisor, strided rows, a misaligned operand (the scalar kernel)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["natural", "qsgd:127", "std.dithering:16:inf", "bernulli:0.5"])
def test_weights_divisor_and_layouts(ag, spec):
    n, d = 5, 4099
    a, h, p, u, _, _ = operands(n, d)
    for mode in modes_of(spec):
        want_u, want_q, want_h, want_nu, want_nq = oracle_round(spec, n, d, mode, weighted=True)
        # (ld, offsets of a / h / p): aligned and padded; ld % 4 != 0; each operand misaligned in turn
        layouts = [(d + 5, (0, 0, 0)), (d + 2, (0, 0, 0)), (d + 5, (1, 0, 0)), (d + 5, (0, 1, 0)), (d + 5, (0, 0, 3))]
        for ld, (oa, oh, op) in layouts:
            tag = f"{spec} {mode} ld={ld} off={oa, oh, op}"
            ta, th, tp = strided(a, ld, oa), strided(h, ld, oh), strided(p, ld, op)
            got_u, got_q, nu, nq, _, _, _ = one_call(ag, spec, ta, th, tp, n, d, mode, u, weights=WEIGHTS)
            same(got_u, want_u, tag)
            same(got_q, want_q, tag)
            same(th, want_h, tag)
            t2a, t2h, t2p = strided(a, ld, oa), strided(h, ld, oh), strided(p, ld, op)
            lib_u, lib_q, lib_nu, lib_nq = two_calls(ag, spec, t2a, t2h, t2p, n, d, mode, u, weights=WEIGHTS)
            same(got_u, lib_u, tag)
            same(got_q, lib_q, tag)
            same(th, t2h, tag)
            if dithering(spec):
                same(nu, want_nu, tag)
                same(nq, want_nq, tag)
                same(nu, lib_nu, tag)
                same(nq, lib_nq, tag)
        # a divisor in place of sum(w): the same sums over another total
        ta, th, tp = dev(a, h, p)
        got_u, got_q, *_ = one_call(ag, spec, ta, th, tp, n, d, mode, u, weights=WEIGHTS, divisor=1.0)
        t2a, t2h, t2p = dev(a, h, p)
        lib_u, lib_q, _, _ = two_calls(ag, spec, t2a, t2h, t2p, n, d, mode, u, weights=WEIGHTS, divisor=1.0)
        assert_bitexact(got_u, lib_u)
        assert_bitexact(got_q, lib_q)
        tot = np.float32(sum(WEIGHTS))
        assert_bitexact((got_u.cpu().numpy() / tot).astype(np.float32), want_u)


def test_misaligned_outputs_take_the_scalar_kernel(ag):
    """out_u one float past alignment: every element through the scalar twin, the same bits."""
    n, d, spec, mode = 5, 4099, "qsgd:127", "device"
    a, h, p, u, gp, hp = operands(n, d)
    want_u, want_q, want_h, _, _ = oracle_round(spec, n, d, mode)
    ta, th, tp, tg, thp = dev(a, h, p, gp, hp)
    buf = torch.zeros(d + 4, device="cuda")
    out_u = buf[1:1 + d]
    assert out_u.data_ptr() % 16 == 4
    from flpytorch_amd import _lib
    _lib.profile_enable(True)
    for k in ("k_ew_frecon_accum", "k_norm_partials2"):
        _lib.profile_collect(k)
    got_u, got_q, *_ = one_call(ag, spec, ta, th, tp, n, d, mode, u, out_u=out_u)
    torch.cuda.synchronize()
    ran = {k: _lib.profile_collect(k)[1] for k in ("k_ew_frecon_accum", "k_norm_partials2")}
    _lib.profile_enable(False)
    assert ran == {"k_ew_frecon_accum": 1, "k_norm_partials2": 1}, ran
    assert got_u is out_u
    assert_bitexact(got_u, want_u)
    assert_bitexact(got_q, want_q)
    assert_bitexact(th, want_h)


# ------------------------------------------------------------------------------------------------
# 4. the Python round helpers: RandK / TopK composed from the existing reducers, COFIG, statistics
# ------------------------------------------------------------------------------------------------
def stepwise(ag, spec, n, d, a, h, p, gp, hp, lam, alpha_update, randk_idx=None):
    """N freconStep calls, reduce_rows of their messages, the tail in torch: what freconUplink returns."""
    ta, th, tp, tg, thp = dev(a, h, p, gp, hp)
    us, qs = torch.empty_like(ta), torch.empty_like(ta)
    comps = []
    for i in range(n):
        c = ag.initCompressor(spec, d)
        if randk_idx is not None:
            c.S = torch.from_numpy(randk_idx[i].copy()).cuda()
        else:
            c.device_rng = (SEED, CLIENT0 + i)
        us[i], _, qs[i] = ag.freconStep(c, ta[i], th[i], tp[i], ALPHA, in_place=True)
        comps.append(c)
    u_avg = ag.reduce_rows(tg, us, relative=False)
    q_avg = ag.reduce_rows(tg, qs, relative=False)
    result = q_avg + (1.0 - lam) * tg + lam * (u_avg + thp)
    return result, thp + alpha_update * u_avg, th, comps


@pytest.mark.parametrize("case", ["randk-compat", "randk-device", "randk-sparse", "topk", "topk-batched"])
def test_frecon_uplink_selection_codecs(ag, case):
    n, d, lam, alpha_update = 5, 4099, 0.25, 0.3
    a, h, p, _, gp, hp = operands(n, d)
    h = np.where(h == 0, np.float32(0), h)                     # (no -0 in the shifts: the sparse rounds' contract)
    spec = "randk:3%" if case.startswith("randk") else "topk:2%"
    idx = None
    kw = {"client0": CLIENT0}
    if case == "randk-compat":
        K = oc.OracleCompressor(spec, d).K
        g = np.random.default_rng(5)
        idx = np.stack([g.choice(d, K, replace=False) for _ in range(n)])
        kw["randk_idx"] = torch.from_numpy(idx).cuda()
    if case == "randk-sparse":
        kw["sparse"] = True
    if case == "topk-batched":
        kw["batched"] = True
    want, want_hp, want_h, _ = stepwise(ag, spec, n, d, a, h, p, gp, hp, lam, alpha_update, idx)
    ta, th, tp, tg, thp = dev(a, h, p, gp, hp)
    comp = ag.initCompressor(spec, d)
    got = ag.freconUplink(comp, ta, th, tp, ALPHA, lam, tg, thp, alpha_update, seed=SEED, **kw)
    assert_bitexact(got, want)
    assert_bitexact(thp, want_hp)                               # advanced in place by default
    assert_bitexact(th, want_h)
    K = oc.OracleCompressor(spec, d).K
    assert comp.total_input_components == 2 * n * d and comp.really_need_to_send_components == 2 * n * K
    # the one-kernel entry itself refuses these codecs
    from flpytorch_amd import _lib
    prm, _ = comp.codec_params(torch.device("cuda", torch.cuda.current_device()))
    assert _lib.load().flc_frecon_reduce_workspace_size(ctypes.byref(prm), n, d) == 0


@pytest.mark.parametrize("spec", ["natural", "qsgd:127", "bernulli:0.5"])
def test_frecon_uplink_elementwise_and_statistics(ag, spec):
    n, d, lam, alpha_update = 5, 4099, 0.5, 0.375
    a, h, p, u, gp, hp = operands(n, d)
    for mode in modes_of(spec):
        want_u, want_q, want_h, _, _ = oracle_round(spec, n, d, mode)
        cu, cq = torch.from_numpy(want_u), torch.from_numpy(want_q)
        cg, chp = torch.from_numpy(gp.copy()), torch.from_numpy(hp.copy())
        want = cq + (1.0 - lam) * cg + lam * (cu + chp)
        ta, th, tp, tg, thp = dev(a, h, p, gp, hp)
        comp = ag.initCompressor(spec, d)
        keep = torch.empty(d, device="cuda")
        got = ag.freconUplink(comp, ta, th, tp, ALPHA, lam, tg, thp, alpha_update, seed=SEED, h_prev_out=keep,
                              **pattern_kw(spec, n, d, mode, u))
        assert_bitexact(got, want)
        assert_bitexact(keep, chp + alpha_update * cu)
        assert torch.equal(thp, dev(hp)[0])
        assert_bitexact(th, want_h)
        # 2 N compressVector calls on the wire counters
        ref = [oracle_comp(spec, d, i, mode, u) for i in range(n)]
        need = 0
        for i, o in enumerate(ref):
            o.compress(a[i] - h[i])
            need += 2 * o.last_need_to_send_advance
        assert comp.total_input_components == 2 * n * d
        assert comp.really_need_to_send_components == need
        assert comp.last_need_to_send_advance == ref[-1].last_need_to_send_advance


@pytest.mark.parametrize("spec", ["natural", "randk:3%"])
def test_cofig_uplink_is_diana_uplink_plus_h_prev(ag, spec):
    n, d = 5, 4099
    a, h, _, u, _, hp = operands(n, d)
    mode = "device"
    ta, th, thp = dev(a, h, hp)
    keep_u = torch.empty(d, device="cuda")
    got = ag.cofigUplink(ag.initCompressor(spec, d), ta, th, ALPHA, thp, seed=SEED, client0=CLIENT0, out=keep_u)
    t2a, t2h = dev(a, h)
    want_u = ag.dianaUplink(ag.initCompressor(spec, d), t2a, t2h, ALPHA, seed=SEED, client0=CLIENT0)
    assert_bitexact(keep_u, want_u)
    assert_bitexact(got, want_u + thp)
    assert_bitexact(th, t2h)
    # cofigStep is dianaStep under its own name
    c1, c2 = (lib_comp(ag, spec, d, 0, mode, u) for _ in range(2))
    if spec.startswith("randk"):
        c1.device_rng = c2.device_rng = (SEED, CLIENT0)
    sa, sh = dev(a[0], h[0])
    m1, h1 = ag.cofigStep(c1, sa, sh, ALPHA)
    m2, h2 = ag.dianaStep(c2, sa, sh, ALPHA)
    assert_bitexact(m1, m2)
    assert_bitexact(h1, h2)


# ------------------------------------------------------------------------------------------------
# 5. IEEE edge values: the rows of tests/edge_rows.py as the first message's differences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["qsgd:8", "natural"])
def test_edge_rows(ag, spec):
    """a_i - h_i is edge row i bit for bit (edge_rows.shift_operands); p_i is the next kind's h, so
    the second message encodes unrelated magnitudes (NaN, inf, subnormal differences) with the same
    draws.  Own norms, compat draws (at 0.0 and beside the probabilities) and device draws."""
    D, kinds = er.D, er.KINDS
    n = len(kinds)
    rows = [er.row(k, spec) for k in kinds]
    ab = [er.shift_operands(x) for x in rows]
    a = np.stack([t[0] for t in ab])
    h = np.stack([t[1] for t in ab])
    p = np.roll(h, -1, axis=0)
    for mode in ("compat", "device"):
        ucompat = np.stack([er.uniforms(k, spec, x) for k, x in zip(kinds, rows)])
        us, qs, hs, nu, nq = [], [], [], [], []
        with np.errstate(all="ignore"):
            for i in range(n):
                o = oc.OracleCompressor(spec, D)
                o.testp = ucompat[i] if mode == "compat" else devrng.uniforms(SEED, CLIENT0 + i, D)
                m, h2 = oc.shift_step(o, a[i], h[i], alpha=ALPHA, h=h[i])
                q, _ = oc.shift_step(o, a[i], p[i])
                us.append(m)
                qs.append(q)
                hs.append(h2)
                if dithering(spec):
                    nu.append(o.norm((a[i] - h[i]).astype(np.float32)))
                    nq.append(o.norm((a[i] - p[i]).astype(np.float32)))
            want_u, want_q = oc.reduce_plain(us), oc.reduce_plain(qs)
        kw = {"client0": CLIENT0}
        if mode == "compat":
            kw["uniforms"] = torch.from_numpy(ucompat).cuda()
        for off in (0, 1):
            ld = D + 5
            ta, th, tp = strided(a, ld, off), strided(h, ld, off), strided(p, ld, off)
            red = ag.FreconUplinkReducer(ag.initCompressor(spec, D), seed=SEED)
            gnu, gnq = (torch.zeros(n, device="cuda") for _ in range(2))
            pn = dithering(spec)
            got_u, got_q, _, _ = red(ta, th, tp, ALPHA, pnorms_u_out=gnu if pn else None, pnorms_q_out=gnq if pn else None, **kw)
            tag = f"{spec} {mode} off{off}"
            same(th, np.stack(hs), tag)
            same(got_u, want_u, tag)
            same(got_q, want_q, tag)
            t2a, t2h, t2p = strided(a, ld, off), strided(h, ld, off), strided(p, ld, off)
            red2 = ag.ShiftUplinkReducer(ag.initCompressor(spec, D), seed=SEED)
            lnu, lnq = (torch.zeros(n, device="cuda") for _ in range(2))
            lib_u, _, _ = red2(t2a, t2h, alpha=ALPHA, shift=t2h, shift_out=t2h, pnorms_out=lnu if pn else None, **kw)
            lib_q, _, _ = red2(t2a, t2p, pnorms_out=lnq if pn else None, **kw)
            same(th, t2h, tag)
            same(got_u, lib_u, tag)
            same(got_q, lib_q, tag)
            if pn:
                same(gnu, np.array(nu, np.float32), tag)
                same(gnq, np.array(nq, np.float32), tag)
                same(gnu, lnu, tag)
                same(gnq, lnq, tag)
