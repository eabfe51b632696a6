"""GPU tests of the sparse in-place RandK round (flc_randk_shift_reduce, ShiftUplinkReducer(sparse=True)).

The yardstick is the general entry (flc_encode_shift_reduce, the reducer without ``sparse``) on cloned
inputs, compared as int32 views.  Inputs of every bitwise comparison are Gaussian rows with shifts built
from them, and each comparison first asserts that no in-place operand holds the bit pattern 0x80000000:
under that condition the dense path's x + 0 is the identity, so equality is required everywhere.

  shape A  DIANA in place   red(a, b, alpha, shift = shift_out = b)
  shape B  EF21 in place    red(a, b, scale = mult, base = msg_out = b)
  shape C  MARINA           red(a, b, base = g [D])
  shape D  C(a - b) fold    red(a, b)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import codecs as oc

pytestmark = pytest.mark.gpu

SEED, CLIENT0 = 2024, 3
ALPHA = 0.75
SHAPES = ("A", "B", "C", "D")
MODES = ("compat", "device")
NS = (1, 2, 5, 70)                 # 70 crosses the 64-row batch of the ring
DS = (7, 4096, 4099, 100003)       # one partial chunk; an exact chunk; a 3-element tail chunk; many chunks
NEG0 = np.uint32(0x80000000)


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def ks_of(d):
    """K = 1, 3 % of d (122 members in a 4096 chunk: the more-than-64-members path), d (everything)."""
    return sorted({1, max(1, int(0.03 * d)), d})


def i32(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def assert_same_bits(got, want, what=""):
    g, w = i32(got).ravel(), i32(want).ravel()
    if not np.array_equal(g, w):
        bad = np.nonzero(g != w)[0]
        raise AssertionError(f"{what}: {bad.size} of {g.size} elements differ; first {bad[:5]}: "
                             f"{g[bad[:5]].view(np.float32)} vs {w[bad[:5]].view(np.float32)}")


@functools.lru_cache(maxsize=None)
def inputs(n, d):
    """Gaussian a rows, shifts built from them, one shared vector — read-only, shared by the tests."""
    g = np.random.default_rng([n, d, 77])
    a = g.standard_normal((n, d)).astype(np.float32)
    b = (a + g.standard_normal((n, d))).astype(np.float32)
    b[:, ::13] = a[:, ::13]                         # zero differences at selected places too
    gp = g.standard_normal(d).astype(np.float32)
    for v in (a, b, gp):
        v.setflags(write=False)
    return a, b, gp


@functools.lru_cache(maxsize=None)
def compat_idx(n, d, k):
    """The reference's numpy stream: row i = RandomState(100 + i).choice(d, k, replace=False)."""
    from flpytorch_amd.aggregation.compressors import stream_choice
    idx = np.stack([stream_choice(np.random.RandomState(100 + i), d, k) for i in range(n)]).astype(np.int64)
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def device_idx(n, d, k):
    from flpytorch_amd import _lib
    idx = np.empty((n, k), dtype=np.int64)
    for i in range(n):
        assert _lib.load().flc_device_randk_indices(SEED, CLIENT0 + i, d, k, idx[i].ctypes.data) == 0
    idx.setflags(write=False)
    return idx


def index_sets(mode, n, d, k):
    return compat_idx(n, d, k) if mode == "compat" else device_idx(n, d, k)


def call_shape(red, comp, shape, ta, tb, tg, **kw):
    """One round of the shape on the given device tensors (tb updated in place in A and B); returns out."""
    if shape == "A":
        out, m, h = red(ta, tb, alpha=ALPHA, shift=tb, shift_out=tb, **kw)
        assert m is None and h is tb
    elif shape == "B":
        mult = 1.0 / (1.0 + comp.getW())                # RandK is unbiased: EF21's mult
        out, m, h = red(ta, tb, scale=mult, base=tb, msg_out=tb, **kw)
        assert m is tb and h is None
    elif shape == "C":
        out, m, h = red(ta, tb, base=tg, **kw)
        assert m is None and h is None
    else:
        out, m, h = red(ta, tb, scale=0.5, **kw)
        assert m is None and h is None
    return out


def pattern_kw(mode, n, d, k):
    kw = {"client0": CLIENT0}
    if mode == "compat":
        kw["randk_idx"] = torch.from_numpy(compat_idx(n, d, k).copy()).cuda()
    return kw


def both(ag, shape, mode, n, d, k, a=None, b=None, ld=None, check_neg0=True, **extra):
    """The sparse and the general round on cloned inputs: ((out, rows) sparse, (out, rows) general)."""
    a0, b0, gp = inputs(n, d)
    a = a0 if a is None else a
    b = b0 if b is None else b
    if check_neg0 and shape in "AB":
        assert not (b.view(np.uint32) == NEG0).any()     # the in-place operand holds no -0
    comp = ag.initCompressor(f"randk:{k}", d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    kw = pattern_kw(mode, n, d, k)
    kw.update(extra)
    res = []
    for sparse in (True, False):
        if ld is None:
            ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
        else:                                            # unaligned rows: views of [n, ld] storage
            sa, sb = (torch.full((n, ld), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
            ta, tb = sa[:, :d], sb[:, :d]
            ta.copy_(torch.from_numpy(a.copy()))
            tb.copy_(torch.from_numpy(b.copy()))
        tg = torch.from_numpy(gp.copy()).cuda()
        out = call_shape(red, comp, shape, ta, tb, tg, sparse=sparse, **kw)
        if ld is not None:
            assert bool((sb[:, d:] == 7.0).all()) and bool((sa[:, d:] == 7.0).all())   # nothing past a row's end
        res.append((out, tb))
    return res[0], res[1]


WEIGHTS = [1.0, 0.5, 2.0, 1.25, 3.0]


# ------------------------------------------------------------------------------------------------
# 1. parity with the general entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_general_entry(ag, shape, mode):
    for n in NS:
        for d in DS:
            for k in ks_of(d):
                for weighted in (False, True):
                    extra = {}
                    if weighted:
                        extra = {"weights": [WEIGHTS[i % 5] for i in range(n)], "divisor": 1.75}
                    (out, rows), (gout, grows) = both(ag, shape, mode, n, d, k, **extra)
                    what = f"shape {shape} {mode} n={n} d={d} K={k} weighted={weighted}"
                    assert_same_bits(out, gout, what + " out")
                    assert_same_bits(rows, grows, what + " rows")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_on_unaligned_row_views(ag, shape, mode):
    n, d = 5, 4099
    for k in ks_of(d):
        (out, rows), (gout, grows) = both(ag, shape, mode, n, d, k, ld=d + 3, weights=WEIGHTS)
        assert_same_bits(out, gout, f"shape {shape} {mode} K={k} out")
        assert_same_bits(rows, grows, f"shape {shape} {mode} K={k} rows")


# ------------------------------------------------------------------------------------------------
# 2. parity with the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_parity(ag, shape, mode):
    n, d, k = 5, 4099, 122
    a, b, gp = inputs(n, d)
    sets = index_sets(mode, n, d, k)
    msgs, hs = [], []
    for i in range(n):
        o = oc.OracleCompressor(f"randk:{k}", d)
        o.S = sets[i]
        if shape == "A":
            m, h = oc.shift_step(o, a[i], b[i], alpha=ALPHA, h=b[i])
        elif shape == "B":
            m, h = oc.shift_step(o, a[i], b[i], scale=1.0 / (1.0 + o.w), base=b[i])
        elif shape == "C":
            m, h = oc.shift_step(o, a[i], b[i], base=gp)
        else:
            m, h = oc.shift_step(o, a[i], b[i], scale=0.5)
        msgs.append(m)
        hs.append(h)
    want = oc.reduce_plain(msgs, WEIGHTS)
    (out, rows), _ = both(ag, shape, mode, n, d, k, weights=WEIGHTS)
    assert np.array_equal(i32(out), np.asarray(want, np.float32).view(np.int32))
    if shape == "A":
        assert np.array_equal(i32(rows), np.stack(hs).astype(np.float32).view(np.int32))
    elif shape == "B":
        assert np.array_equal(i32(rows), np.stack(msgs).astype(np.float32).view(np.int32))
    else:
        assert np.array_equal(i32(rows), b.view(np.int32))


# ------------------------------------------------------------------------------------------------
# 3. elements outside a row's index set are not written
# ------------------------------------------------------------------------------------------------
PLANTED = np.array([0x80000000, 0x00000001, 0x80000001, 0x7F7FFFFF, 0x007FFFFF], dtype=np.uint32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_untouched_elements(ag, shape, mode):
    n, d, k = 5, 100003, 3000
    a, b, _ = inputs(n, d)
    a, b = a.copy(), b.copy()
    sets = index_sets(mode, n, d, k)
    places = []                                          # per row: unselected places, a different column set per row
    for i in range(n):
        free = np.setdiff1d(np.arange(d), sets[i])
        free = free[(free % n) == i]                     # no column is planted in two rows: out stays comparable
        p = free[:: max(1, free.size // 50)][:50]
        a[i, p] = np.nan                                 # never read by a sparse round, never selected by the general one
        if shape in "AB":
            b.view(np.uint32)[i, p] = PLANTED[np.arange(p.size) % PLANTED.size]
        places.append(p)
    (out, rows), (gout, grows) = both(ag, shape, mode, n, d, k, a=a, b=b, check_neg0=False, weights=WEIGHTS)
    assert_same_bits(out, gout, "out")
    got, gen = i32(rows).view(np.uint32), i32(grows).view(np.uint32)
    for i in range(n):
        p = places[i]
        assert np.array_equal(got[i, p], b.view(np.uint32)[i, p])          # the stored bits, exactly
        assert np.array_equal(got[i, sets[i]], gen[i, sets[i]])            # the selected places: the general entry's
        if shape in "AB":
            z = p[b.view(np.uint32)[i, p] == NEG0]
            assert z.size > 0
            assert (got[i, z] == NEG0).all() and (gen[i, z] == 0).all()    # the documented difference: -0 kept / +0
            rest = np.ones(d, bool)
            rest[z] = False
            assert np.array_equal(got[i, rest], gen[i, rest])              # and it is the only one


# ------------------------------------------------------------------------------------------------
# 4. signed zeros at selected places (the -0 column rule of the fold)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_selected_signed_zeros(ag, shape, mode):
    n, d = 5, 4099
    a, b, _ = inputs(n, d)
    a, b = a.copy(), b.copy()
    a[:, 0:700] = -0.0                                   # a = -0, b = +0: v = -0 in every row
    b[:, 0:700] = 0.0
    a[:, 700:1400] = b[:, 700:1400]                      # a == b: v = +0
    a[1:, 1400:2000] = -0.0                              # -0 in every row but the first
    b[1:, 1400:2000] = 0.0
    for k in (122, d):
        for weights in (None, WEIGHTS, [1.0, -0.5, 2.0, -1.25, 3.0]):
            (out, rows), (gout, grows) = both(ag, shape, mode, n, d, k, a=a, b=b, weights=weights)
            assert_same_bits(out, gout, f"K={k} weights={weights} out")
            assert_same_bits(rows, grows, f"K={k} weights={weights} rows")
            if k == d and weights is None and shape in "AD":
                assert (i32(out)[:700].view(np.uint32) == NEG0).all()      # (the rule is exercised: -0 columns exist)


# ------------------------------------------------------------------------------------------------
# 5. one launch
# ------------------------------------------------------------------------------------------------
def test_one_launch(ag):
    from flpytorch_amd import _lib
    n, d, k = 5, 100003, 3000
    names = ("k_randk_shift", "k_randk_shift_lists")
    _lib.profile_enable(True)
    try:
        for name in names:
            _lib.profile_collect(name)
        a, b, gp = inputs(n, d)
        comp = ag.initCompressor(f"randk:{k}", d)
        red = ag.ShiftUplinkReducer(comp, seed=SEED)
        for sparse, launches in ((True, 1), (False, 0)):
            ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
            call_shape(red, comp, "A", ta, tb, None, sparse=sparse, client0=CLIENT0)
            torch.cuda.synchronize()
            assert _lib.profile_collect("k_randk_shift")[1] == launches
            assert _lib.profile_collect("k_randk_shift_lists")[1] == 0
        ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
        call_shape(red, comp, "A", ta, tb, None, sparse=True, **pattern_kw("compat", n, d, k))
        torch.cuda.synchronize()
        assert _lib.profile_collect("k_randk_shift_lists")[1] == 1
        assert _lib.profile_collect("k_randk_shift")[1] == 0
    finally:
        _lib.profile_enable(False)
        for name in names:
            _lib.profile_collect(name)


# ------------------------------------------------------------------------------------------------
# 6. refusals leave the outputs untouched
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched(ag):
    n, d, k = 5, 4099, 122
    a, b, gp = inputs(n, d)
    comp = ag.initCompressor(f"randk:{k}", d)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    ta = torch.from_numpy(a.copy()).cuda()

    def poisoned(shape):                                 # a NaN with a recognisable payload
        return torch.full(shape, 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)
    out, tb, other = poisoned((d,)), poisoned((n, d)), poisoned((n, d))
    refused = [
        dict(alpha=ALPHA, shift=tb, shift_out=other),                      # a dense shift matrix
        dict(alpha=ALPHA, shift=other, shift_out=tb),                      # a shift that is not b
        dict(alpha=ALPHA, shift=tb, shift_out=tb, msg_out=other),          # stored messages beside a shift
        dict(base=other, msg_out=tb),                                      # a per-row base that is not b
        dict(base=tb, msg_out=other),                                      # a dense message matrix
        dict(base=other),                                                  # a per-row base without a store
        dict(scale=-1.0),                                                  # a negative scale
        dict(alpha=0.0, shift=tb, shift_out=tb),                           # alpha == 0 with a shift
    ]
    for kw in refused:
        with pytest.raises(NotImplementedError):
            red(ta, tb, out=out, client0=CLIENT0, sparse=True, **kw)
    with pytest.raises(ValueError):
        red(ta, tb, out=out, sparse=True, pnorms_out=torch.empty(n, device="cuda"))
    torch.cuda.synchronize()
    for t in (out, tb, other):
        assert bool((t.view(torch.int32) == 0x7FC0BEEF).all())
    assert comp.total_input_components == 0                                # and no round was accounted


# ------------------------------------------------------------------------------------------------
# 7. the Python layer
# ------------------------------------------------------------------------------------------------
def stats(comp):
    return (comp.total_input_components, comp.really_need_to_send_components, comp.last_input_advance,
            comp.last_need_to_send_advance)


@pytest.mark.parametrize("mode", MODES)
def test_uplink_helpers(ag, mode):
    n, d, k = 5, 30011, 900
    a, b, gp = inputs(n, d)
    kw = pattern_kw(mode, n, d, k)

    def fresh():
        return (torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), torch.from_numpy(gp.copy()).cuda(),
                ag.initCompressor(f"randk:{k}", d))
    for algo in ("diana", "ef21", "marina"):
        res = []
        for sparse in (True, False):
            ta, tb, tg, comp = fresh()
            if algo == "diana":
                out = ag.dianaUplink(comp, ta, tb, ALPHA, seed=SEED, sparse=sparse, weights=WEIGHTS, **kw)
            elif algo == "ef21":
                out = ag.ef21Uplink(comp, ta, tb, seed=SEED, sparse=sparse, weights=WEIGHTS, **kw)
            else:
                out = ag.marinaUplink(comp, ta, tb, tg, seed=SEED, sparse=sparse, weights=WEIGHTS, **kw)
            res.append((out, tb, stats(comp)))
        assert_same_bits(res[0][0], res[1][0], algo + " out")
        assert_same_bits(res[0][1], res[1][1], algo + " rows")
        assert res[0][2] == res[1][2] and res[0][2][0] == n * d            # the wire statistics of N compressShift calls
        # ... and the reducer's own results
        ta, tb, tg, comp = fresh()
        shape = {"diana": "A", "ef21": "B", "marina": "C"}[algo]
        out = call_shape(ag.ShiftUplinkReducer(comp, seed=SEED), comp, shape, ta, tb, tg, sparse=True, weights=WEIGHTS, **kw)
        assert_same_bits(res[0][0], out, algo + " reducer out")
        assert_same_bits(res[0][1], tb, algo + " reducer rows")


def test_other_compressors_raise(ag):
    n, d = 3, 4099
    a, b, gp = inputs(n, d)
    ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    keep = tb.clone()
    for spec in ("topk:2%", "natural", "ident"):
        comp = ag.initCompressor(spec, d)
        with pytest.raises(NotImplementedError, match="RANDK"):
            ag.dianaUplink(comp, ta, tb, ALPHA, seed=SEED, sparse=True)
        assert comp.total_input_components == 0
    assert torch.equal(tb, keep)


@pytest.mark.parametrize("shape", SHAPES)
def test_side_stream(ag, shape):
    n, d, k = 5, 100003, 3000
    (out, rows), _ = both(ag, shape, "device", n, d, k, weights=WEIGHTS)
    side = torch.cuda.Stream()
    a, b, gp = inputs(n, d)
    ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a, b, gp))
    comp = ag.initCompressor(f"randk:{k}", d)
    torch.cuda.synchronize()
    sout = call_shape(ag.ShiftUplinkReducer(comp, seed=SEED), comp, shape, ta, tb, tg, sparse=True, weights=WEIGHTS,
                      client0=CLIENT0, stream=side)
    side.synchronize()
    assert_same_bits(sout, out, "out")
    assert_same_bits(tb, rows, "rows")


def test_workspace_bytes_switch(ag):
    comp = ag.initCompressor("randk:10000", 1000000)
    red = ag.ShiftUplinkReducer(comp, seed=SEED)
    dense = red.workspace_bytes(5, 1000000)
    assert dense > 12 * 1000000
    for compat in (False, True):
        assert 0 < red.workspace_bytes(5, 1000000, sparse=True, compat=compat) < 4 * 1000000


@pytest.mark.parametrize("shape", SHAPES)
def test_given_chunk_counts_are_honoured(ag, shape):
    """d_randk_counts from flc_device_randk_counts: the same round; counts of another K: another result."""
    n, d, k = 5, 100003, 3000
    (out, rows), _ = both(ag, shape, "device", n, d, k, weights=WEIGHTS)
    a, b, gp = inputs(n, d)
    for kk, same in ((k, True), (k // 2, False)):
        ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a, b, gp))
        comp = ag.initCompressor(f"randk:{k}", d)
        counts = ag.UplinkReducer(ag.initCompressor(f"randk:{kk}", d), seed=SEED).randk_counts(n, d, client0=CLIENT0)
        got = call_shape(ag.ShiftUplinkReducer(comp, seed=SEED), comp, shape, ta, tb, tg, sparse=True, weights=WEIGHTS,
                         client0=CLIENT0, randk_counts=counts)
        assert np.array_equal(i32(got), i32(out)) == same
        assert np.array_equal(i32(tb), i32(rows)) == (same or shape in "CD")
    with pytest.raises(ValueError):
        ag.ShiftUplinkReducer(comp, seed=SEED)(ta, tb, randk_counts=counts)
