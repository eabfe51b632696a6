"""GPU tests of the sampled shifted rounds (partial participation): flc_encode / randk / topk
_shift_reduce_sampled through ``ShiftUplinkReducer(..., clients=ids)`` and the uplink helpers.

n of N_total resident clients take part; the state rows (h_i, g_prev_i) are rows ``ids[i]`` of an
[N_total, D] matrix S, the gradients G are [n, D] in participant order, and the draws are those of client
``client0 + ids[i]``.  Every comparison is bit for bit (int32 views).  Non-participants' rows of S are
pre-filled with arbitrary bit patterns (-0 and NaN payloads among them) and must keep them.

Shapes: N_total = 7 with an unordered, a single, a reversed, the identity, a two-row and a four-row id set
(n = 3, 1, 7, 7, 2, 4: the two-row ring's odd and single cases, no refill at n = 2, both slots ending in one
turn at n = 4), every one of them through every test of the elementwise kernels; D = 4111 for those codecs
(two 2048-element tiles, three more float4 groups, a 3-element scalar tail); D = 8292 for RandK (two 4096
chunks and a short one) with K = 83 and 829, and n = 66 of 80 across the 64-row batch; D = 4099 for TopK."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import codecs as oc
from oracle import devrng

pytestmark = pytest.mark.gpu

SEED, CLIENT0, ALPHA = 2024, 11, 0.75
N_TOTAL = 7
IDSETS = ((5, 0, 3), (6,), (6, 5, 4, 3, 2, 1, 0), (0, 1, 2, 3, 4, 5, 6), (2, 4), (1, 6, 0, 4))
IDSETS_SAMPLED = tuple(s for s in IDSETS if s != tuple(range(N_TOTAL)))      # (the identity keys like the contiguous entry)
D_EW, D_RK, D_TK = 4111, 8292, 4099
NEG0 = np.uint32(0x80000000)
PLANTED = np.array([0x80000000, 0x7FC00123, 0xFFC0BEEF, 0x00000001, 0x80000001, 0x7F7FFFFF], dtype=np.uint32)
LAZY_U = [0.3, 0.7, 0.1, 0.9, 0.4, 0.6, 0.2]
DRAWN = (oc.NATURAL, oc.STD_DITHERING, oc.NAT_DITHERING)


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def i32(t):
    if torch.is_tensor(t):
        return t.detach().contiguous().view(torch.int32).cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32).view(np.int32)


def assert_same_bits(got, want, what=""):
    g, w = i32(got).ravel(), i32(want).ravel()
    assert g.size == w.size, what
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        raise AssertionError(f"{what}: {bad.size} of {g.size} elements differ; first {bad[:5]}: "
                             f"{g[bad[:5]].view(np.float32)} vs {w[bad[:5]].view(np.float32)}")


@functools.lru_cache(maxsize=None)
def state(ids, d, n_total=N_TOTAL):
    """G [n, d] Gaussian; S [n_total, d]: arbitrary bit patterns everywhere (the planted -0 / NaN payloads
    first in each row), then the participants' rows built from their gradients (no -0 there); g [d];
    compat uniforms [n, d] in participant order.  Read-only, shared by the tests."""
    r = np.random.default_rng([len(ids), d, n_total, 79] + list(ids))
    n = len(ids)
    G = r.standard_normal((n, d)).astype(np.float32)
    S = r.integers(0, 1 << 32, (n_total, d), dtype=np.uint64).astype(np.uint32)
    S[:, :PLANTED.size] = PLANTED[: min(d, PLANTED.size)]
    S = S.view(np.float32)
    for i, c in enumerate(ids):
        S[c] = (G[i] + r.standard_normal(d)).astype(np.float32)
        S[c, ::13] = G[i, ::13]                       # zero differences
    assert not (S[list(ids)].view(np.uint32) == NEG0).any()
    g = r.standard_normal(d).astype(np.float32)
    u = r.random((n, d))
    for v in (G, S, g, u):
        v.setflags(write=False)
    return G, S, g, u


def cuda(v):
    return torch.from_numpy(np.array(v, copy=True)).cuda()


def others(ids, n_total=N_TOTAL):
    return [c for c in range(n_total) if c not in ids]


def assert_others_untouched(tS, S, ids, n_total=N_TOTAL, what=""):
    o = others(ids, n_total)
    if o:
        assert np.array_equal(i32(tS)[o], S.view(np.int32)[o]), f"{what}: a non-participant's row changed"


def mult_of(comp):
    return 1.0 if comp.isContractionCompressor() else 1.0 / (1.0 + comp.getW())


def compat_kw(spec, n, d, u):
    t = oc.OracleCompressor(spec, d).type
    kw = {}
    if t == oc.LAZY:
        kw["lazy_u"] = torch.tensor(LAZY_U[:n], dtype=torch.float64, device="cuda")
    if t in DRAWN:
        kw["uniforms"] = cuda(u)
    return kw


# ------------------------------------------------------------------------------------------------
# 1. compat draws and draw-free codecs: the sampled call against the contiguous entry on gathered rows
# ------------------------------------------------------------------------------------------------
SPECS_COMPAT = ["ident", "bernulli:0.5", "natural", "qsgd:10", "std.dithering:4:inf", "nat.dithering:4:2"]


def round_pair(ag, spec, ids, algo, d=D_EW, make=None, **extra):
    """(sampled, contiguous) results of one round with compat patterns: dicts of out / msg / pn / rows,
    the sampled one with the whole state matrix under "S"."""
    G, S, g, u = state(ids, d)
    n = len(ids)
    comp = ag.initCompressor(spec, d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    kw = compat_kw(spec, n, d, u)
    kw.update(extra)
    res = []
    for sampled in (True, False):
        tG = cuda(G)
        tS = cuda(S) if sampled else cuda(S[list(ids)])
        if make is not None:
            tG, tS = make(tG), make(tS)
        pn = torch.zeros(n, dtype=torch.float32, device="cuda")
        skw = dict(kw, clients=list(ids)) if sampled else dict(kw)
        if skw.get("stream") is not None:                      # the operands above were made on the current stream
            skw["stream"].wait_stream(torch.cuda.current_stream())
        if algo == "diana":            # stored messages in participant order, the shift in place by id
            msg = torch.zeros((n, d), dtype=torch.float32, device="cuda")
            if sampled:
                skw["indexed"] = ("b", "shift", "shift_out")
            out, m, h = red(tG, tS, alpha=ALPHA, shift=tS, shift_out=tS, msg_out=msg, pnorms_out=pn, **skw)
            assert h is tS and m is msg
        elif algo == "ef21":           # everything in place by id (the default indexed set)
            out, m, h = red(tG, tS, scale=mult_of(comp), base=tS, msg_out=tS, pnorms_out=pn, **skw)
            assert m is tS and h is None
            msg = None
        else:                          # marina: a shared base, b by id, nothing stored
            out, m, h = red(tG, tS, base=cuda(g), pnorms_out=pn, **skw)
            assert m is None and h is None
            msg = None
        if skw.get("stream") is not None:
            torch.cuda.current_stream().wait_stream(skw["stream"])
        rows = tS[list(ids)] if sampled else tS
        res.append({"out": out, "msg": msg, "pn": pn, "rows": rows, "S": tS})
    return res[0], res[1]


def assert_pair(s, c, S, ids, what):
    assert_same_bits(s["out"], c["out"], what + " out")
    assert_same_bits(s["pn"], c["pn"], what + " norms")
    assert_same_bits(s["rows"], c["rows"], what + " rows")
    if s["msg"] is not None:
        assert_same_bits(s["msg"], c["msg"], what + " messages")
    assert_others_untouched(s["S"], S, ids, what=what)


@pytest.mark.parametrize("ids", IDSETS)
@pytest.mark.parametrize("spec", SPECS_COMPAT)
def test_compat_and_draw_free_codecs(ag, spec, ids):
    for algo in ("diana", "ef21", "marina"):
        s, c = round_pair(ag, spec, ids, algo)
        assert_pair(s, c, state(ids, D_EW)[1], ids, f"{spec} {algo} {ids}")
        if algo == "marina":           # b is only read: the whole state keeps its bits
            assert_same_bits(s["S"], state(ids, D_EW)[1], "marina state")


# every per-row operand a matrix of its own: the base rows that are not b (BASE_ROWS), a shift_in that is
# not b, a stored message matrix and a shift_out apart from both, each addressed by its own bit
@pytest.mark.parametrize("scalar", [False, True])
@pytest.mark.parametrize("indexed", [None, ("base", "shift", "shift_out"), ("b", "msg_out"), ("shift",), ()])
@pytest.mark.parametrize("spec", ["natural", "qsgd:10"])
def test_separate_operands_each_by_its_own_bit(ag, spec, indexed, scalar):
    names = ("b", "base", "msg_out", "shift", "shift_out")
    idx = names if indexed is None else indexed
    d = D_EW
    for ids in ((5, 0, 3), (2, 4), (1, 6, 0, 4), (6,)):
        n = len(ids)
        G, S, g, u = state(ids, d)
        r = np.random.default_rng([n, 81])
        full = {"b": S}                                # [N_total, d] forms: arbitrary bits outside ids
        for k in ("base", "shift"):
            m = S.copy()
            m[list(ids)] = r.standard_normal((n, d)).astype(np.float32)
            full[k] = m
        full["msg_out"] = np.full((N_TOTAL, d), 7.5, np.float32)
        full["shift_out"] = np.full((N_TOTAL, d), -3.25, np.float32)
        red = ag.ShiftUplinkReducer(ag.initCompressor(spec, d), seed=SEED)
        kw = compat_kw(spec, n, d, u)
        res = []
        for sampled in (True, False):
            make = in_padded_storage(3, 1) if scalar else (lambda t: t)
            ops = {k: make(cuda(full[k] if (sampled and k in idx) else full[k][list(ids)])) for k in names}
            tG = make(cuda(G))
            pn = torch.zeros(n, dtype=torch.float32, device="cuda")
            skw = dict(kw, clients=list(ids), indexed=indexed) if sampled else kw
            out, m, h = red(tG, ops["b"], scale=0.25, base=ops["base"], msg_out=ops["msg_out"], alpha=ALPHA,
                            shift=ops["shift"], shift_out=ops["shift_out"], pnorms_out=pn, **skw)
            assert m is ops["msg_out"] and h is ops["shift_out"]
            res.append((out, pn, ops))
        (out, pn, ops), (cout, cpn, cops) = res
        what = f"{spec} {ids} indexed={indexed} scalar={scalar}"
        assert_same_bits(out, cout, what + " out")
        assert_same_bits(pn, cpn, what + " norms")
        for k in names:
            rows = ops[k][list(ids)] if k in idx else ops[k]
            assert_same_bits(rows, cops[k], f"{what} {k}")
            if k in idx:
                assert_others_untouched(ops[k], full[k], ids, what=f"{what} {k}")
            if k in ("b", "base", "shift"):            # inputs keep their bits
                assert_same_bits(ops[k], full[k] if k in idx else full[k][list(ids)], f"{what} input {k}")
        assert not np.array_equal(i32(cops["msg_out"]), i32(cuda(full["msg_out"][list(ids)])))


# ------------------------------------------------------------------------------------------------
# 2. device draws: n single-row steps under client CLIENT0 + ids[i] and reduce_rows; the oracle
# ------------------------------------------------------------------------------------------------
SPECS_DEVICE = [("natural", D_EW), ("qsgd:10", D_EW), ("std.dithering:4:inf", D_EW), ("randk:83", D_RK),
                ("randk:829", D_RK), ("topk:83", D_RK)]


def sampled_round(ag, spec, ids, algo, d, n_total=N_TOTAL, **kw):
    """One sampled round with device draws on fresh copies: (out, state matrix after, stored messages)."""
    G, S, g, _ = state(ids, d, n_total)
    comp = ag.initCompressor(spec, d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    tG, tS = cuda(G), cuda(S)
    kw = dict(kw, clients=list(ids), client0=CLIENT0)
    msg = None
    if algo == "diana_msg":
        msg = torch.zeros_like(tG)
        out, _, _ = red(tG, tS, alpha=ALPHA, shift=tS, shift_out=tS, msg_out=msg, indexed=("b", "shift", "shift_out"), **kw)
    elif algo == "diana":
        out, _, _ = red(tG, tS, alpha=ALPHA, shift=tS, shift_out=tS, **kw)
    elif algo == "ef21":
        out, _, _ = red(tG, tS, scale=mult_of(comp), base=tS, msg_out=tS, **kw)
    elif algo == "marina":
        out, _, _ = red(tG, tS, base=cuda(g), **kw)
    else:                              # the plain fold of C(a - b) * 0.5
        out, _, _ = red(tG, tS, scale=0.5, **kw)
    return out, tS, msg


def per_client_steps(ag, spec, ids, algo, d, weights=None):
    """n compressShift calls under client CLIENT0 + ids[i] into stored rows, then reduce_rows."""
    G, S, g, _ = state(ids, d)
    tG, tS, tg = cuda(G), cuda(S), cuda(g)
    msgs, hs = torch.empty_like(tG), torch.empty_like(tG)
    for i, cid in enumerate(ids):
        c = ag.initCompressor(spec, d)
        c.device_rng = (SEED, CLIENT0 + cid)
        if algo.startswith("diana"):
            c.compressShift(tG[i], tS[cid], out=msgs[i], alpha=ALPHA, shift=tS[cid], shift_out=hs[i])
        elif algo == "ef21":
            c.compressShift(tG[i], tS[cid], scale=mult_of(c), base=tS[cid], out=msgs[i])
        else:
            c.compressShift(tG[i], tS[cid], base=tg, out=msgs[i])
    return ag.reduce_rows(tg, msgs, weights=weights, relative=False), msgs, hs


def oracle_steps(spec, ids, algo, d):
    G, S, g, _ = state(ids, d)
    msgs, hs = [], []
    for i, cid in enumerate(ids):
        o = oc.OracleCompressor(spec, d)
        if o.type in DRAWN:
            o.testp = devrng.uniforms(SEED, CLIENT0 + cid, d)
        elif o.type == oc.RANDK:
            o.S = devrng.randk_indices(SEED, CLIENT0 + cid, d, o.K)
        if algo.startswith("diana"):
            m, h = oc.shift_step(o, G[i], S[cid], alpha=ALPHA, h=S[cid])
        elif algo == "ef21":
            m, h = oc.shift_step(o, G[i], S[cid], scale=(1.0 if hasattr(o, "alpha") else 1.0 / (1.0 + o.w)), base=S[cid])
        else:
            m, h = oc.shift_step(o, G[i], S[cid], base=g)
        msgs.append(m)
        hs.append(h)
    return oc.reduce_plain(msgs, None), msgs, hs


@pytest.mark.parametrize("ids", IDSETS_SAMPLED)
@pytest.mark.parametrize("spec,d", SPECS_DEVICE)
def test_device_draws_are_keyed_by_client(ag, spec, d, ids):
    S = state(ids, d)[1]
    for algo in ("diana_msg", "ef21", "marina"):
        what = f"{spec} {algo} {ids}"
        out, tS, msg = sampled_round(ag, spec, ids, algo, d)
        want_out, want_m, want_h = per_client_steps(ag, spec, ids, algo, d)
        o_out, o_m, o_h = oracle_steps(spec, ids, algo, d)
        assert_same_bits(out, want_out, what + " out / steps")
        assert_same_bits(out, o_out, what + " out / oracle")
        if algo == "diana_msg":
            assert_same_bits(msg, want_m, what + " messages / steps")
            assert_same_bits(msg, np.stack(o_m), what + " messages / oracle")
            assert_same_bits(tS[list(ids)], want_h, what + " shifts / steps")
            assert_same_bits(tS[list(ids)], np.stack(o_h), what + " shifts / oracle")
        elif algo == "ef21":
            assert_same_bits(tS[list(ids)], want_m, what + " estimators / steps")
            assert_same_bits(tS[list(ids)], np.stack(o_m), what + " estimators / oracle")
        else:
            assert_same_bits(tS, S, what + " state")
        assert_others_untouched(tS, S, ids, what=what)


# ------------------------------------------------------------------------------------------------
# 3. a client's row does not depend on the company it keeps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,d,kw", [("natural", D_EW, {}), ("qsgd:10", D_EW, {}), ("randk:83", D_RK, {}),
                                       ("randk:83", D_RK, {"sparse": True}), ("topk:83", D_TK, {"batched": True})])
def test_independence_of_company(ag, spec, d, kw):
    ids = (5, 0, 3)
    G, S, _, _ = state(ids, d)
    comp = ag.initCompressor(spec, d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    tS = cuda(S)
    red(cuda(G), tS, alpha=ALPHA, shift=tS, shift_out=tS, clients=list(ids), client0=CLIENT0, **kw)
    alone = cuda(S)
    out1, _, _ = red(cuda(G[2:3]), alone, alpha=ALPHA, shift=alone, shift_out=alone, clients=[3], client0=CLIENT0, **kw)
    assert_same_bits(alone[3], tS[3], f"{spec} client 3")
    assert not np.array_equal(i32(alone[3]), S.view(np.int32)[3])
    assert_others_untouched(alone, S, (3,), what="alone")


# ------------------------------------------------------------------------------------------------
# 4. unaligned row views and ld % 4 != 0: the scalar kernel, the same bits
# ------------------------------------------------------------------------------------------------
def in_padded_storage(pad, offset):
    def make(t):
        n, d = t.shape
        buf = torch.full((n * (d + pad) + offset,), 7.0, dtype=torch.float32, device="cuda")
        v = buf[offset:].view(n, d + pad)[:, :d]
        v.copy_(t)
        make.bufs.append((buf, v))
        return v
    make.bufs = []
    return make


@pytest.mark.parametrize("pad,offset", [(3, 0), (4, 1)])
@pytest.mark.parametrize("spec", ["natural", "qsgd:10", "ident"])
def test_scalar_kernel_on_unaligned_views(ag, spec, pad, offset):
    ids = (5, 0, 3)
    for algo in ("diana", "ef21"):
        ref, _ = round_pair(ag, spec, ids, algo)
        make = in_padded_storage(pad, offset)
        s, c = round_pair(ag, spec, ids, algo, make=make)
        if offset:
            assert s["S"].data_ptr() % 16 != 0
        else:
            assert s["S"].stride(0) % 4 != 0
        what = f"{spec} {algo} pad={pad} offset={offset}"
        assert_pair(s, c, state(ids, D_EW)[1], ids, what)
        for key in ("out", "pn", "rows"):
            assert_same_bits(s[key], ref[key], what + " against the vector kernel: " + key)
        for buf, v in make.bufs:           # nothing stored past a row's end
            n, d = v.shape
            assert bool((buf[offset:].view(n, d + pad)[:, d:] == 7.0).all())


# ------------------------------------------------------------------------------------------------
# 5. weights, divisor and a side stream
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["natural", "qsgd:10"])
def test_weights_divisor_and_side_stream(ag, spec):
    ids = (6, 5, 4, 3, 2, 1, 0)
    weights = [1.0, 0.5, 2.0, 1.25, 3.0, 0.75, 1.5]
    for algo in ("diana", "ef21"):
        s, c = round_pair(ag, spec, ids, algo, weights=weights, divisor=7.0)
        assert_pair(s, c, state(ids, D_EW)[1], ids, f"{spec} {algo} weighted")
        plain, _ = round_pair(ag, spec, ids, algo)
        assert not np.array_equal(i32(plain["out"]), i32(s["out"]))
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        side, _ = round_pair(ag, spec, ids, algo, weights=weights, divisor=7.0, stream=st)
        st.synchronize()
        for key in ("out", "pn", "S"):
            assert_same_bits(side[key], s[key], f"{spec} {algo} side stream {key}")
    # device draws with weights: the per-client steps folded with the same weights
    out, tS, _ = sampled_round(ag, spec, ids, "diana", D_EW, weights=weights)
    want_out, _, want_h = per_client_steps(ag, spec, ids, "diana", D_EW, weights=weights)
    assert_same_bits(out, want_out, "weighted device draws out")
    assert_same_bits(tS[list(ids)], want_h, "weighted device draws shifts")


# ------------------------------------------------------------------------------------------------
# 6. the sparse RandK and the batched TopK entry
# ------------------------------------------------------------------------------------------------
SHAPE_ALGO = {"A": "diana", "B": "ef21", "C": "marina", "D": "fold"}


def compat_idx(n, d, k):
    from flpytorch_amd.aggregation.compressors import stream_choice
    return np.stack([stream_choice(np.random.RandomState(100 + i), d, k) for i in range(n)]).astype(np.int64)


def sparse_against_general(ag, spec, ids, shape, d, fast, n_total=N_TOTAL, **kw):
    S = state(ids, d, n_total)[1]
    what = f"{spec} shape {shape} {ids if len(ids) < 8 else len(ids)} {sorted(kw)}"
    out, tS, _ = sampled_round(ag, spec, ids, SHAPE_ALGO[shape], d, n_total, **dict(kw, **fast))
    gout, gS, _ = sampled_round(ag, spec, ids, SHAPE_ALGO[shape], d, n_total, **kw)
    assert_same_bits(out, gout, what + " out")
    assert_same_bits(tS, gS, what + " state")          # (the participants' rows hold no -0)
    assert_others_untouched(tS, S, ids, n_total, what)
    if shape in "CD":
        assert_same_bits(tS, S, what + ": b is only read")
    else:
        assert not np.array_equal(i32(tS)[list(ids)], S.view(np.int32)[list(ids)])


@pytest.mark.parametrize("shape", "ABCD")
@pytest.mark.parametrize("k", [83, 829])
def test_sparse_randk(ag, k, shape):
    spec = f"randk:{k}"
    for ids in IDSETS:
        sparse_against_general(ag, spec, ids, shape, D_RK, {"sparse": True})
        idx = cuda(compat_idx(len(ids), D_RK, k))
        sparse_against_general(ag, spec, ids, shape, D_RK, {"sparse": True}, randk_idx=idx)


@pytest.mark.parametrize("shape", "ABCD")
def test_sparse_randk_across_the_row_batch(ag, shape):
    ids = tuple(int(c) for c in np.random.default_rng(80).permutation(80)[:66])
    weights = [1.0 + (i % 5) * 0.25 for i in range(66)]
    sparse_against_general(ag, "randk:83", ids, shape, D_RK, {"sparse": True}, n_total=80, weights=weights)


@pytest.mark.parametrize("shape", "ABCD")
def test_batched_topk(ag, shape):
    for k in (1, 82, D_TK // 16 + 1, D_TK):
        for ids in IDSETS:
            sparse_against_general(ag, f"topk:{k}", ids, shape, D_TK, {"batched": True})
    for d in (7, 4096):
        sparse_against_general(ag, "topk:3", (5, 0, 3), shape, d, {"batched": True})


@pytest.mark.parametrize("shape", "ABCD")
@pytest.mark.parametrize("n,n_total", [(17, 20), (66, 80)])
def test_batched_topk_many_rows(ag, n, n_total, shape):
    ids = tuple(int(c) for c in np.random.default_rng(n).permutation(n_total)[:n])
    sparse_against_general(ag, "topk:82", ids, shape, D_TK, {"batched": True}, n_total=n_total)


@pytest.mark.parametrize("shape", "AB")
@pytest.mark.parametrize("spec,d,fast", [("randk:83", D_RK, {"sparse": True}), ("topk:82", D_TK, {"batched": True})])
def test_untouched_elements_of_participants(ag, spec, d, fast, shape):
    """-0 and NaN sentinels at unselected places of the participants' rows keep their bits (the general
    entry turns the -0 into +0 there: the one documented difference), selected places carry the general
    entry's bits."""
    ids = (5, 0, 3)
    G, S, g, _ = state(ids, d)
    G, S = G.copy(), S.copy()
    k = int(spec.split(":")[1])
    places = []
    for i, cid in enumerate(ids):
        if spec.startswith("randk"):
            sel = np.asarray(devrng.randk_indices(SEED, CLIENT0 + cid, d, k))
            free = np.setdiff1d(np.arange(d), sel)
            p = free[:: max(1, free.size // 48)][:48]
            pat = PLANTED[np.arange(p.size) % PLANTED.size]       # NaN payloads too: RandK never reads them
            G[i, p] = np.nan
        else:
            sel = np.argsort(-np.abs(G[i] - S[cid]), kind="stable")[:k]
            free = np.setdiff1d(np.arange(d), sel)
            p = free[:: max(1, free.size // 48)][:48]
            finite = PLANTED[~np.isnan(PLANTED.view(np.float32))]
            pat = finite[np.arange(p.size) % finite.size]         # a zero difference there: never selected
            G.view(np.uint32)[i, p] = pat
        S.view(np.uint32)[cid, p] = pat
        places.append((p, sel))
    comp = ag.initCompressor(spec, d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    res = []
    for kw in (fast, {}):
        tG, tS = cuda(G), cuda(S)
        if shape == "A":
            out, _, _ = red(tG, tS, alpha=ALPHA, shift=tS, shift_out=tS, clients=list(ids), client0=CLIENT0, **kw)
        else:
            out, _, _ = red(tG, tS, scale=mult_of(comp), base=tS, msg_out=tS, clients=list(ids), client0=CLIENT0, **kw)
        res.append((out, tS))
    (out, tS), (gout, gS) = res
    got, gen, orig = i32(tS).view(np.uint32), i32(gS).view(np.uint32), S.view(np.uint32)
    for i, cid in enumerate(ids):
        p, sel = places[i]
        assert np.array_equal(got[cid, p], orig[cid, p])                  # the stored bits, exactly
        assert np.array_equal(got[cid, sel], gen[cid, sel])               # the selected places: the general entry's
        assert not np.array_equal(got[cid, sel], orig[cid, sel])
        z = p[orig[cid, p] == NEG0]
        assert z.size > 0 and (got[cid, z] == NEG0).all() and (gen[cid, z] == 0).all()
        rest = np.ones(d, bool)
        rest[p] = False
        assert np.array_equal(got[cid, rest], gen[cid, rest])
    assert_others_untouched(tS, S, ids)
    assert_others_untouched(gS, S, ids)
    if shape == "A":                                                      # the fold of the sparse messages
        assert_same_bits(out, gout, "out")


# ------------------------------------------------------------------------------------------------
# 7. refusals: nothing is written
# ------------------------------------------------------------------------------------------------
def poisoned(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda").view(torch.int32).fill_(0x7FC0ABCD).view(torch.float32)


def test_python_refusals_leave_everything_untouched(ag):
    ids = (5, 0, 3)
    d = D_RK
    G, S, g, _ = state(ids, d)
    tG, tS, tg = cuda(G), cuda(S), cuda(g)
    out = poisoned((d,))
    red = ag.ShiftUplinkReducer(ag.initCompressor("randk:83", d), seed=SEED)
    diana = dict(alpha=ALPHA, shift=tS, shift_out=tS, out=out)
    for kw in ({}, {"sparse": True}):
        with pytest.raises(ValueError):                                   # duplicate ids
            red(tG, tS, clients=[5, 0, 5], **diana, **kw)
        with pytest.raises(ValueError):                                   # an id equal to N_total
            red(tG, tS, clients=[5, N_TOTAL, 3], **diana, **kw)
        with pytest.raises(ValueError):                                   # one id per row of a
            red(tG, tS, clients=[5, 0], **diana, **kw)
        with pytest.raises(ValueError):                                   # FLC_IDX_BASE on a shared base
            red(tG, tS, base=tg, out=out, clients=list(ids), indexed=("b", "base"), **kw)
        with pytest.raises(ValueError):                                   # an indexed shift with nowhere to go
            red(tG, tS, alpha=ALPHA, shift=tS, out=out, clients=list(ids), **kw)
        with pytest.raises(ValueError):                                   # the in-place pair, one of them indexed
            red(tG, tS, clients=list(ids), indexed=("b",), **diana, **kw)
        with pytest.raises(ValueError):                                   # indexed without clients
            red(tG, tS[list(ids)].clone(), indexed=("b",), out=out, **kw)
    cnt = torch.zeros(((d + 4095) // 4096, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        red(tG, tS, clients=list(ids), sparse=True, randk_counts=cnt, **diana)
    q = ag.ShiftUplinkReducer(ag.initCompressor("qsgd:10", d), seed=SEED)
    with pytest.raises(NotImplementedError):
        q(tG, tS, clients=list(ids), one_read=True, **diana)
    with pytest.raises(NotImplementedError):
        q.workspace_bytes(3, d, one_read=True, sampled=True)
    with pytest.raises(NotImplementedError):
        ag.freconUplink(ag.initCompressor("natural", d), tG, tS, tG.clone(), ALPHA, 0.5, tg, tg.clone(), seed=SEED,
                        clients=list(ids))
    with pytest.raises(NotImplementedError):
        ag.FreconUplinkReducer(ag.initCompressor("natural", d), seed=SEED)(tG, tS, tG.clone(), ALPHA, clients=list(ids))
    # the identity round reaches the library with the state's own shape: the mismatched pair is refused there
    full = tuple(range(N_TOTAL))
    G7, S7, _, _ = state(full, d)
    tG7, tS7 = cuda(G7), cuda(S7)
    for kw in ({}, {"sparse": True}):
        with pytest.raises(ValueError, match="in place"):
            red(tG7, tS7, alpha=ALPHA, shift=tS7, shift_out=tS7, out=out, clients=list(full), indexed=("b",), **kw)
    torch.cuda.synchronize()
    assert_same_bits(tS, S, "state after refusals")
    assert_same_bits(tS7, S7, "state after refusals")
    assert bool((out.view(torch.int32) == 0x7FC0ABCD).all())
    assert red.workspace_bytes(3, d, sparse=True, sampled=True) > red.workspace_bytes(3, d, sparse=True)
    assert red.workspace_bytes(3, d, sampled=True) == red.workspace_bytes(3, d)


def test_library_refusals_leave_everything_untouched(ag):
    """The same cases at the C ABI, with real device operands: FLC_ERR_ARG, nothing written."""
    from flpytorch_amd import _lib
    lib = _lib.load()
    ids = (5, 0, 3)
    n, d = 3, D_RK
    G, S, g, _ = state(ids, d)
    tG, tS, tg = cuda(G), cuda(S), cuda(g)
    out = poisoned((d,))
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    comp = ag.initCompressor("randk:83", d)
    prm, keep = comp.codec_params(torch.device("cuda", torch.cuda.current_device()))
    prm.seed = SEED
    tprm, tkeep = ag.initCompressor("topk:83", d).codec_params(torch.device("cuda", torch.cuda.current_device()))
    cnt = torch.zeros(((d + 4095) // 4096, n), dtype=torch.int32, device="cuda")
    B_, BASE_, MSG_, IN_, OUT_ = 1, 2, 4, 8, 16

    def rows(kind):
        r = _lib.FlcShiftRows()
        r.d_a, r.lda, r.d_b, r.ldb = tG.data_ptr(), d, tS.data_ptr(), d
        r.msg_scale, r.shift_alpha = 1.0, ALPHA
        if kind == "diana":
            r.d_shift_in, r.ldin, r.d_shift_out, r.ldout = tS.data_ptr(), d, tS.data_ptr(), d
        elif kind == "ef21":
            r.d_base, r.ldbase, r.d_msg, r.ldmsg = tS.data_ptr(), d, tS.data_ptr(), d
        else:
            r.d_base, r.ldbase = tg.data_ptr(), 0
        return r

    def call(which, kind, id_list, bits, counts=False):
        h = np.asarray(id_list, dtype=np.int32)
        dv = torch.from_numpy(h).cuda()
        m = _lib.FlcRowMap()
        m.h_ids, m.d_ids, m.n_total, m.indexed = h.ctypes.data, dv.data_ptr(), N_TOTAL, bits
        pat = _lib.FlcPattern()
        pat.client0 = CLIENT0
        if counts:
            pat.d_randk_counts = cnt.data_ptr()
        r = rows(kind)
        vp = ctypes.c_void_p
        tail = (vp(out.data_ptr()), vp(ws.data_ptr()), ws.numel(), _lib.stream_ptr())
        if which == "general":
            rc = lib.flc_encode_shift_reduce_sampled(ctypes.byref(prm), ctypes.byref(pat), ctypes.byref(r), ctypes.byref(m),
                                                     n, d, None, ctypes.c_float(3.0), None, *tail)
        elif which == "randk":
            rc = lib.flc_randk_shift_reduce_sampled(ctypes.byref(prm), ctypes.byref(pat), ctypes.byref(r), ctypes.byref(m),
                                                    n, d, None, ctypes.c_float(3.0), *tail)
        else:
            rc = lib.flc_topk_shift_reduce_sampled(ctypes.byref(tprm), ctypes.byref(r), ctypes.byref(m), n, d, None,
                                                   ctypes.c_float(3.0), *tail)
        torch.cuda.synchronize()
        return rc

    diana_bits, ef21_bits = B_ | IN_ | OUT_, B_ | BASE_ | MSG_
    for which in ("general", "randk", "topk"):
        assert call(which, "diana", [5, 0, 5], diana_bits) == _lib.FLC_ERR_ARG          # duplicate ids
        assert call(which, "ef21", [5, N_TOTAL, 3], ef21_bits) == _lib.FLC_ERR_ARG      # an id equal to N_total
        assert call(which, "diana", [5, 0, 3], B_ | IN_) == _lib.FLC_ERR_ARG            # mismatched bits in place
        assert call(which, "ef21", [5, 0, 3], B_ | BASE_) == _lib.FLC_ERR_ARG
        assert call(which, "marina", [5, 0, 3], B_ | BASE_) == _lib.FLC_ERR_ARG         # FLC_IDX_BASE on a shared base
    assert call("randk", "diana", [5, 0, 3], diana_bits, counts=True) == _lib.FLC_ERR_ARG
    assert_same_bits(tS, S, "state after refusals")
    assert_same_bits(tG, G, "gradients after refusals")
    assert bool((out.view(torch.int32) == 0x7FC0ABCD).all())
    # and the same operands are accepted once the map is right
    assert call("randk", "diana", [5, 0, 3], diana_bits) == _lib.FLC_OK
    assert not bool((out.view(torch.int32) == 0x7FC0ABCD).any())


# ------------------------------------------------------------------------------------------------
# 8. the uplink helpers with clients=
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,d,kw", [("natural", D_EW, {}), ("qsgd:10", D_EW, {}), ("randk:83", D_RK, {"sparse": True}),
                                       ("topk:83", D_TK, {"batched": True}), ("topk:83", D_TK, {})])
def test_uplink_helpers_with_clients(ag, spec, d, kw):
    ids = (5, 0, 3)
    G, S, g, _ = state(ids, d)
    tg = cuda(g)

    def steps(step):
        """n in-place client steps under client CLIENT0 + ids[i], their messages folded by reduce_rows."""
        tG, tS = cuda(G), cuda(S)
        msgs = []
        for i, cid in enumerate(ids):
            c = ag.initCompressor(spec, d)
            c.device_rng = (SEED, CLIENT0 + cid)
            msgs.append(step(c, tG[i], tS[cid]))
        return ag.reduce_rows(tg, torch.stack(msgs), relative=False), tS

    kw = dict(kw, seed=SEED, client0=CLIENT0, clients=list(ids))
    # DIANA and COFIG
    want, wS = steps(lambda c, gi, hi: ag.dianaStep(c, gi, hi, ALPHA, in_place=True)[0])
    tS = cuda(S)
    out = ag.dianaUplink(ag.initCompressor(spec, d), cuda(G), tS, ALPHA, **kw)
    assert_same_bits(out, want, "dianaUplink out")
    assert_same_bits(tS, wS, "dianaUplink state")
    tS = cuda(S)
    out = ag.cofigUplink(ag.initCompressor(spec, d), cuda(G), tS, ALPHA, tg, **kw)
    assert_same_bits(out, want + tg, "cofigUplink out")
    assert_same_bits(tS, wS, "cofigUplink state")
    # EF21: the message is the new estimator
    want, wS = steps(lambda c, gi, hi: ag.ef21Step(c, gi, hi, in_place=True))
    tS = cuda(S)
    out = ag.ef21Uplink(ag.initCompressor(spec, d), cuda(G), tS, **kw)
    assert_same_bits(out, want, "ef21Uplink out")
    assert_same_bits(tS, wS, "ef21Uplink state")
    # PP-MARINA: fresh [n, D] previous gradients, keys only
    P = cuda(S[list(ids)])
    tG, msgs = cuda(G), []
    for i, cid in enumerate(ids):
        c = ag.initCompressor(spec, d)
        c.device_rng = (SEED, CLIENT0 + cid)
        msgs.append(ag.marinaStep(c, tG[i], P[i], tg))
    want = ag.reduce_rows(tg, torch.stack(msgs), relative=False)
    P2 = P.clone()
    out = ag.marinaUplink(ag.initCompressor(spec, d), tG, P2, tg, **kw)
    assert_same_bits(out, want, "marinaUplink out")
    assert_same_bits(P2, P, "marinaUplink previous gradients")


def test_wire_statistics_advance_per_participant(ag):
    ids = (5, 0, 3)
    d = D_EW
    G, S, _, _ = state(ids, d)
    fused = ag.initCompressor("natural", d)
    tS = cuda(S)
    ag.dianaUplink(fused, cuda(G), tS, ALPHA, seed=SEED, clients=list(ids))
    single = ag.initCompressor("natural", d)
    single.device_rng = (SEED, 0)
    tS2 = cuda(S)
    for i, cid in enumerate(ids):
        ag.dianaStep(single, cuda(G)[i], tS2[cid], ALPHA, in_place=True)
    for name in ("total_input_components", "really_need_to_send_components", "last_input_advance", "last_need_to_send_advance"):
        assert getattr(fused, name) == getattr(single, name), name
