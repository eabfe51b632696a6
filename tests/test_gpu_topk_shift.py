"""GPU tests of the batched TopK shifted round (flc_topk_shift_reduce, ShiftUplinkReducer(batched=True)).

The yardstick is the general entry (flc_encode_shift_reduce, the same reducer without ``batched``) on
cloned inputs, compared as int32 views.  Inputs of every bitwise comparison are Gaussian rows with shifts
built from them, and each comparison first asserts that no in-place operand holds the bit pattern
0x80000000: under that condition the dense path's x + 0 is the identity, so equality is required
everywhere.

  shape A  DIANA in place   red(a, b, alpha, shift = shift_out = b)
  shape B  EF21 in place    red(a, b, base = msg_out = b)          (TopK is contractive: mult = 1)
  shape C  MARINA           red(a, b, base = g [D])
  shape D  C(a - b) fold    red(a, b, scale = 0.5)
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import codecs as oc

pytestmark = pytest.mark.gpu

ALPHA = 0.75
SHAPES = ("A", "B", "C", "D")
TIES = ("lowest", "highest")
NS = (1, 2, 5, 17, 70)             # 17: the first many-row count (few rows: <= 16); 70 crosses the fold's 64-row batch
DS = (7, 4096, 4099, 100003)       # one partial chunk; an exact chunk; a 3-element tail chunk; many chunks
NEG0 = np.uint32(0x80000000)
WEIGHTS = [1.0, 0.5, 2.0, 1.25, 3.0]


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def ks_of(d):
    """K = 1, 2 % of d, both sides of the dense-K switch (K * 16 > d), d (the zero differences too)."""
    return sorted({min(d, max(1, k)) for k in (1, math.ceil(0.02 * d), d // 16, d // 16 + 1, d)})


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
    g = np.random.default_rng([n, d, 78])
    a = g.standard_normal((n, d)).astype(np.float32)
    b = (a + g.standard_normal((n, d))).astype(np.float32)
    b[:, ::13] = a[:, ::13]                         # zero differences
    gp = g.standard_normal(d).astype(np.float32)
    for v in (a, b, gp):
        v.setflags(write=False)
    return a, b, gp


def compressor(ag, d, k, tie="lowest"):
    comp = ag.initCompressor(f"topk:{k}", d)
    assert comp.K == k
    comp.tie_policy = tie
    return comp


def call_shape(red, shape, ta, tb, tg, **kw):
    """One round of the shape on the given device tensors (tb updated in place in A and B); returns out."""
    if shape == "A":
        out, m, h = red(ta, tb, alpha=ALPHA, shift=tb, shift_out=tb, **kw)
        assert m is None and h is tb
    elif shape == "B":
        out, m, h = red(ta, tb, base=tb, msg_out=tb, **kw)
        assert m is tb and h is None
    elif shape == "C":
        out, m, h = red(ta, tb, base=tg, **kw)
        assert m is None and h is None
    else:
        out, m, h = red(ta, tb, scale=0.5, **kw)
        assert m is None and h is None
    return out


def both(ag, shape, tie, n, d, k, a=None, b=None, ld=None, check_neg0=True, **extra):
    """The batched and the general round on cloned inputs: ((out, rows) batched, (out, rows) general)."""
    a0, b0, gp = inputs(n, d)
    a = a0 if a is None else a
    b = b0 if b is None else b
    if check_neg0 and shape in "AB":
        assert not (b.view(np.uint32) == NEG0).any()     # the in-place operand holds no -0
    red = ag.ShiftUplinkReducer(compressor(ag, d, k, tie))
    ha, hb, tg = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), torch.from_numpy(gp.copy()).cuda()
    res = []
    for batched in (True, False):
        if ld is None:
            ta, tb = ha.clone(), hb.clone()
        else:                                            # unaligned rows: views of [n, ld] storage
            sa, sb = (torch.full((n, ld), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
            ta, tb = sa[:, :d], sb[:, :d]
            ta.copy_(ha)
            tb.copy_(hb)
        out = call_shape(red, shape, ta, tb, tg, batched=batched, **extra)
        if ld is not None:
            assert bool((sb[:, d:] == 7.0).all()) and bool((sa[:, d:] == 7.0).all())   # nothing past a row's end
        res.append((out, tb))
    return res[0], res[1]


# ------------------------------------------------------------------------------------------------
# 1. parity with the general entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_general_entry(ag, shape, tie, n):
    for d in DS:
        for k in ks_of(d):
            for weighted in (False, True):
                extra = {}
                if weighted:
                    extra = {"weights": [WEIGHTS[i % 5] for i in range(n)], "divisor": 1.75}
                (out, rows), (gout, grows) = both(ag, shape, tie, n, d, k, **extra)
                what = f"shape {shape} tie={tie} n={n} d={d} K={k} weighted={weighted}"
                assert_same_bits(out, gout, what + " out")
                assert_same_bits(rows, grows, what + " rows")


# ------------------------------------------------------------------------------------------------
# 2. tied rows
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tied_inputs(n, d):
    """Differences that are multiples of 1/8 in [-4, 4] (a - b is exact): thousands of ties at any K-th key."""
    g = np.random.default_rng([n, d, 79])
    b = (np.round(g.standard_normal((n, d)) * 8.0) / 8.0 + 0.0).astype(np.float32)      # (+ 0.0: no -0)
    q = (g.integers(-32, 33, (n, d)) / 8.0).astype(np.float32)
    a = (b + q).astype(np.float32)
    assert np.array_equal(a - b, q)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_tied_rows(ag, shape, tie, n):
    d = 100003
    k = math.ceil(0.02 * d)
    a, b = tied_inputs(n, d)
    (out, rows), (gout, grows) = both(ag, shape, tie, n, d, k, a=a, b=b, weights=[WEIGHTS[i % 5] for i in range(n)])
    assert_same_bits(out, gout, "out")
    assert_same_bits(rows, grows, "rows")
    got, gen, was = i32(rows), i32(grows), b.view(np.int32)
    for i in range(n):
        sel = oc.topk_indices_fast(a[i] - b[i], k, tie)
        assert np.sum(oc.topk_keys(a[i] - b[i]) == oc.topk_keys(a[i] - b[i])[sel].min()) > k - np.sum(
            oc.topk_keys(a[i] - b[i]) > oc.topk_keys(a[i] - b[i])[sel].min())            # the tie rule decides
        changed = np.flatnonzero(got[i] != was[i])
        if shape in "AB":
            assert np.array_equal(changed, sel[gen[i, sel] != was[i, sel]])               # the oracle's set, minus no-ops
            assert changed.size > k // 2
        else:
            assert changed.size == 0


# ------------------------------------------------------------------------------------------------
# 3. parity with the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_parity(ag, shape, tie):
    n, d, k = 5, 4099, 82
    a, b, gp = inputs(n, d)
    msgs, hs, sets = [], [], []
    for i in range(n):
        o = oc.OracleCompressor(f"topk:{k}", d)
        o.tie = tie
        if shape == "A":
            m, h = oc.shift_step(o, a[i], b[i], alpha=ALPHA, h=b[i])
        elif shape == "B":
            m, h = oc.shift_step(o, a[i], b[i], base=b[i])
        elif shape == "C":
            m, h = oc.shift_step(o, a[i], b[i], base=gp)
        else:
            m, h = oc.shift_step(o, a[i], b[i], scale=0.5)
        msgs.append(m)
        hs.append(h)
        sets.append(oc.topk_indices(a[i] - b[i], k, tie))
    want = oc.reduce_plain(msgs, WEIGHTS)
    (out, rows), _ = both(ag, shape, tie, n, d, k, weights=WEIGHTS)
    assert np.array_equal(i32(out), np.asarray(want, np.float32).view(np.int32))
    got = i32(rows)
    if shape == "A":
        assert np.array_equal(got, np.stack(hs).astype(np.float32).view(np.int32))
    elif shape == "B":
        assert np.array_equal(got, np.stack(msgs).astype(np.float32).view(np.int32))
    for i in range(n):                                   # unselected in-place elements are unchanged
        rest = np.ones(d, bool)
        rest[sets[i]] = False
        assert np.array_equal(got[i, rest], b.view(np.int32)[i, rest])
        if shape in "CD":
            assert np.array_equal(got[i], b.view(np.int32)[i])


# ------------------------------------------------------------------------------------------------
# 4. unaligned views
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", TIES)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_on_unaligned_row_views(ag, shape, tie):
    n, d = 5, 4099
    for k in ks_of(d):
        (out, rows), (gout, grows) = both(ag, shape, tie, n, d, k, ld=d + 3, weights=WEIGHTS)
        assert_same_bits(out, gout, f"shape {shape} K={k} out")
        assert_same_bits(rows, grows, f"shape {shape} K={k} rows")


# ------------------------------------------------------------------------------------------------
# 5. unselected places keep their bits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B"])
def test_unselected_places_keep_their_bits(ag, shape):
    n, d, k = 5, 4099, 82
    a, b, _ = inputs(n, d)
    a, b = a.copy(), b.copy()
    zeros, dens = [], []
    for i in range(n):
        cols = np.flatnonzero(np.arange(d) % n == i)     # no column is planted in two rows
        z, q = cols[10:210:10], cols[215:415:10]
        assert z.size == 20 and q.size == 20
        a[i, z], b[i, z] = 0.0, -0.0                     # v = +0 - (-0) = +0
        a.view(np.uint32)[i, q] = 0x00000001 + np.arange(20, dtype=np.uint32)   # equal denormals: v = 0
        b.view(np.uint32)[i, q] = a.view(np.uint32)[i, q]
        zeros.append(z)
        dens.append(q)
    diff = a - b
    assert int((diff != 0).sum(axis=1).min()) > 40 * k   # zero differences are never selected
    (out, rows), (gout, grows) = both(ag, shape, "lowest", n, d, k, a=a, b=b, check_neg0=False, weights=WEIGHTS)
    assert_same_bits(out, gout, "out")
    got, gen, was = i32(rows).view(np.uint32), i32(grows).view(np.uint32), b.view(np.uint32)
    for i in range(n):
        z, q = zeros[i], dens[i]
        assert (got[i, z] == NEG0).all() and np.array_equal(got[i, q], was[i, q])      # the planted bits, exactly
        assert (gen[i, z] == 0).all()                                                  # the general entry: -0 -> +0
        rest = np.ones(d, bool)
        rest[z] = False
        assert np.array_equal(got[i, rest], gen[i, rest])                              # and that is the only difference


# ------------------------------------------------------------------------------------------------
# 6. non-finite differences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_non_finite_differences(ag, shape):
    n, d = 5, 4099
    a, b, _ = inputs(n, d)
    a = a.copy()
    a[2, [5, 1000, 4098]] = np.nan
    a[2, 77], a[2, 3000] = np.inf, -np.inf
    for k in (3, 82, d // 16 + 1):
        (out, rows), (gout, grows) = both(ag, shape, "lowest", n, d, k, a=a, weights=WEIGHTS)
        assert_same_bits(out, gout, f"K={k} out")
        assert_same_bits(rows, grows, f"K={k} rows")
        if shape == "A":
            assert np.isnan(rows[2, [5, 1000, 4098]].cpu().numpy()).all()      # NaN keys rank above inf: selected at K = 3


# ------------------------------------------------------------------------------------------------
# 7. the selection's paths (shape A with b = +0: the difference rows are the a rows)
# ------------------------------------------------------------------------------------------------
def paths_round(ag, rows, k, general=True):
    """A batched DIANA round of `rows` against +0 shifts; returns (row flags, batched (out, h), general (out, h))."""
    n, d = rows.shape
    comp = compressor(ag, d, k)
    red = ag.ShiftUplinkReducer(comp)
    ta = torch.from_numpy(rows).cuda()
    tb = torch.zeros((n, d), dtype=torch.float32, device="cuda")
    out = call_shape(red, "A", ta, tb, None, batched=True)
    fl = np.asarray(ag.select_row_flags(comp, n, d))
    if not general:
        return fl, (out, tb), None
    gb = torch.zeros((n, d), dtype=torch.float32, device="cuda")
    gout = call_shape(red, "A", ta, gb, None)
    return fl, (out, tb), (gout, gb)


def test_paths_overflow_inside_one_item(ag):
    from tests.test_gpu_parity import _FilterVariants
    from tests.test_gpu_wg_filter import GCAP, GROUP, SEAMS
    where = "g1+g3"
    n, d = 17, 4_000_000
    k = d // 100
    g = np.random.default_rng([len(where), 17, 3])
    rows = (g.uniform(1e-4, 1e-3, (n, d)) * np.where(g.random((n, d)) < 0.5, -1.0, 1.0)).astype(np.float32)
    rows[:, :4 * GROUP] = 0.0
    counts = [SEAMS[where][i % len(SEAMS[where])] for i in range(n)]
    for i in range(n):
        idx = [q * GROUP + g.choice(GROUP, size=m, replace=False) for q, m in enumerate(counts[i])]
        idx.append(4 * GROUP + g.choice(d - 4 * GROUP, size=k - sum(counts[i]), replace=False))
        idx = np.concatenate(idx)
        rows[i, idx] = ((np.abs(g.standard_normal(idx.size)) + 1.0) *
                        np.where(g.random(idx.size) < 0.5, -1.0, 1.0)).astype(np.float32)
    with _FilterVariants() as fv:
        fl, (out, h), _ = paths_round(ag, rows, k, general=False)
    assert fv.g4 >= 1 and fv.g2 == 0, f"filter variants g4={fv.g4} g2={fv.g2}: not the workgroup-item path"
    for i in range(n):
        over = max(counts[i]) > GCAP
        # (as the filter's own test: a row may also take the exact path for a short list, flag 2)
        assert bool(fl[i] & 1) == over and (not over or fl[i] & 8), f"row {i} {counts[i]}: flags {fl[i]}"
    ta = torch.from_numpy(rows).cuda()
    gb = torch.zeros((n, d), dtype=torch.float32, device="cuda")
    gout = call_shape(ag.ShiftUplinkReducer(compressor(ag, d, k)), "A", ta, gb, None)
    assert_same_bits(out, gout, "out")
    assert_same_bits(h, gb, "rows")


@pytest.mark.parametrize("n", [5, 17])
def test_paths_fast_on_gaussian_rows(ag, n):
    d = 100003
    a, _, _ = inputs(n, d)
    fl, (out, h), (gout, gh) = paths_round(ag, a.copy(), math.ceil(0.02 * d))
    assert not np.any(fl & 8), f"flags {fl}"
    assert_same_bits(out, gout, "out")
    assert_same_bits(h, gh, "rows")


def test_paths_dense_k_is_exact(ag):
    n, d = 5, 4099
    a, _, _ = inputs(n, d)
    fl, (out, h), (gout, gh) = paths_round(ag, a.copy(), d // 16 + 1)
    assert np.all(fl & 8), f"flags {fl}"
    assert_same_bits(out, gout, "out")
    assert_same_bits(h, gh, "rows")


# ------------------------------------------------------------------------------------------------
# 8. the launch shape: this is the test that shows the feature is what ran
# ------------------------------------------------------------------------------------------------
def test_launch_shape(ag):
    from flpytorch_amd import _lib
    n, d = 5, 100003
    k = math.ceil(0.02 * d)
    names = ("k_shift_sub_rows", "k_topk_shift_lists", "k_lone_resident")
    a, b, _ = inputs(n, d)
    red = ag.ShiftUplinkReducer(compressor(ag, d, k))
    _lib.profile_enable(True)
    try:
        for name in names:
            _lib.profile_collect(name)
        for batched, want in ((True, (1, 1, 0)), (False, (0, 0, n))):
            ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
            call_shape(red, "A", ta, tb, None, batched=batched)
            torch.cuda.synchronize()
            assert tuple(_lib.profile_collect(name)[1] for name in names) == want
    finally:
        _lib.profile_enable(False)
        for name in names:
            _lib.profile_collect(name)


# ------------------------------------------------------------------------------------------------
# 9. consecutive rounds on one workspace
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["ef21", "diana"])
def test_consecutive_rounds(ag, algo):
    n, d = 17, 100003
    k = math.ceil(0.02 * d)
    _, b, _ = inputs(n, d)
    assert not (b.view(np.uint32) == NEG0).any()
    tb, gb = torch.from_numpy(b.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    comp, gcomp = compressor(ag, d, k), compressor(ag, d, k)
    g = np.random.default_rng([n, d, 80])
    for r in range(3):
        ta = torch.from_numpy(g.standard_normal((n, d)).astype(np.float32)).cuda()
        if algo == "ef21":
            out = ag.ef21Uplink(comp, ta, tb, batched=True, weights=[WEIGHTS[i % 5] for i in range(n)])
            gout = ag.ef21Uplink(gcomp, ta, gb, weights=[WEIGHTS[i % 5] for i in range(n)])
        else:
            out = ag.dianaUplink(comp, ta, tb, ALPHA, batched=True)
            gout = ag.dianaUplink(gcomp, ta, gb, ALPHA)
        assert not bool((gb.view(torch.int32) == -2147483648).any())       # still no -0 in the operand
        assert_same_bits(out, gout, f"{algo} round {r} out")
        assert_same_bits(tb, gb, f"{algo} round {r} rows")


# ------------------------------------------------------------------------------------------------
# 10. refusals and the Python layer
# ------------------------------------------------------------------------------------------------
def poisoned(shape):                                     # a NaN with a recognisable payload
    return torch.full(shape, 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)


def test_refusals_leave_outputs_untouched(ag):
    n, d, k = 5, 4099, 82
    a, b, gp = inputs(n, d)
    comp = compressor(ag, d, k)
    red = ag.ShiftUplinkReducer(comp)
    ta = torch.from_numpy(a.copy()).cuda()
    out, tb, other = poisoned((d,)), poisoned((n, d)), poisoned((n, d))
    refused = [
        dict(alpha=ALPHA, shift=tb, shift_out=other),                      # a dense shift matrix
        dict(alpha=ALPHA, shift=other, shift_out=tb),                      # a shift that is not b
        dict(alpha=ALPHA, shift=tb, shift_out=tb, msg_out=other),          # stored messages beside a shift
        dict(base=other, msg_out=tb),                                      # a per-row base that is not b
        dict(base=tb, msg_out=other),                                      # a dense message matrix
        dict(base=other),                                                  # a per-row base without a store
        dict(scale=-1.0),                                                  # a negative scale
        dict(scale=float("inf")),
        dict(alpha=0.0, shift=tb, shift_out=tb),                           # alpha == 0 with a shift
        dict(alpha=ALPHA, shift=tb),                                       # not in place: a new shift matrix
    ]
    for kw in refused:
        with pytest.raises(NotImplementedError):
            red(ta, tb, out=out, batched=True, **kw)
    bad = compressor(ag, d, k)
    bad.tie_policy = "lowest"
    bad.K = d + 1                                                          # K > d: the library's FLC_ERR_ARG
    with pytest.raises(ValueError):
        ag.ShiftUplinkReducer(bad)(ta, tb, out=out, batched=True, alpha=ALPHA, shift=tb, shift_out=tb)
    for kw in (dict(sparse=True), dict(pnorms_out=torch.empty(n, device="cuda")),
               dict(randk_counts=torch.zeros((2, n), dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            red(ta, tb, out=out, batched=True, **kw)
    torch.cuda.synchronize()
    for t in (out, tb, other):
        assert bool((t.view(torch.int32) == 0x7FC0BEEF).all())
    assert comp.total_input_components == 0                                # and no round was accounted


def test_other_compressors_raise(ag):
    n, d = 3, 4099
    a, b, gp = inputs(n, d)
    ta, tb = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    keep = tb.clone()
    for spec in ("randk:2%", "natural", "ident"):
        comp = ag.initCompressor(spec, d)
        with pytest.raises(NotImplementedError, match="TOPK"):
            ag.dianaUplink(comp, ta, tb, ALPHA, seed=1, batched=True)
        with pytest.raises(NotImplementedError, match="TOPK"):             # before any operand is looked at
            ag.ShiftUplinkReducer(comp, seed=1)(None, None, batched=True)
        assert comp.total_input_components == 0
    comp = ag.initCompressor("topk:2%", d)                                 # sparse=True with TopK raises as before
    with pytest.raises(NotImplementedError):
        ag.dianaUplink(comp, ta, tb, ALPHA, sparse=True)
    assert comp.total_input_components == 0
    assert torch.equal(tb, keep)


def stats(comp):
    return (comp.total_input_components, comp.really_need_to_send_components, comp.last_input_advance,
            comp.last_need_to_send_advance)


def test_uplink_helpers_and_wire_statistics(ag):
    n, d, k = 5, 30011, 601
    a, b, gp = inputs(n, d)

    def fresh():
        return (torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), torch.from_numpy(gp.copy()).cuda(),
                compressor(ag, d, k))
    for algo in ("diana", "ef21", "marina"):
        res = []
        for batched in (True, False):
            ta, tb, tg, comp = fresh()
            if algo == "diana":
                out = ag.dianaUplink(comp, ta, tb, ALPHA, batched=batched, weights=WEIGHTS)
            elif algo == "ef21":
                out = ag.ef21Uplink(comp, ta, tb, batched=batched, weights=WEIGHTS)
            else:
                out = ag.marinaUplink(comp, ta, tb, tg, batched=batched, weights=WEIGHTS)
            res.append((out, tb, stats(comp)))
        assert_same_bits(res[0][0], res[1][0], algo + " out")
        assert_same_bits(res[0][1], res[1][1], algo + " rows")
        assert res[0][2] == res[1][2] and res[0][2][0] == n * d            # the wire statistics of N compressShift calls
        assert res[0][2][1] == n * k


@pytest.mark.parametrize("shape", SHAPES)
def test_side_stream(ag, shape):
    n, d = 5, 100003
    k = math.ceil(0.02 * d)
    (out, rows), _ = both(ag, shape, "lowest", n, d, k, weights=WEIGHTS)
    side = torch.cuda.Stream()
    a, b, gp = inputs(n, d)
    ta, tb, tg = (torch.from_numpy(v.copy()).cuda() for v in (a, b, gp))
    torch.cuda.synchronize()
    sout = call_shape(ag.ShiftUplinkReducer(compressor(ag, d, k)), shape, ta, tb, tg, batched=True, weights=WEIGHTS,
                      stream=side)
    side.synchronize()
    assert_same_bits(sout, out, "out")
    assert_same_bits(tb, rows, "rows")


def test_workspace_bytes_switch(ag):
    n, d = 5, 100003
    red = ag.ShiftUplinkReducer(compressor(ag, d, 2001))
    assert red.workspace_bytes(n, d, batched=True) >= 4 * n * d > red.workspace_bytes(n, d)
