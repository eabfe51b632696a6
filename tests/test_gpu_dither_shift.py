"""GPU tests of the one-read QSGD shifted round (flc_dither_shift_reduce, ShiftUplinkReducer(one_read=True)).

The yardstick is the general entry (flc_encode_shift_reduce, the same reducer without ``one_read``) on
cloned inputs, compared as int32 views (NaN positions, not payloads).  Each comparison first asserts that
the in-place operand holds no 0x80000000: under that condition the general entry's x + 0 is the identity,
so equality is required everywhere.  The compressor carries ``dither_path = "sparse"`` (the general entry
ignores the hint), the draws are the device's with a fixed seed.

  shape A  DIANA in place   red(a, b, alpha, shift = shift_out = b)
  shape B  EF21 in place    red(a, b, scale, base = msg_out = b)
  shape D  C(a - b) fold    red(a, b)
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import codecs as oc
from oracle import devrng
from test_gpu_dither_sparse import make_rows

pytestmark = pytest.mark.gpu

SEED = 20240607
ALPHA = 0.75
SCALE_B = 0.5
SHAPES = ("A", "B", "D")
SPECS = ("qsgd:4", "qsgd:16")
NS = (1, 2, 5, 17, 130)            # 17 crosses the filter's 16-row item block; 130: two row groups, the side stream
# the half-chunk, chunk and item boundaries; the last whole-row sample and the first sampled row; a ragged row
DS = (1, 7, 2048, 4099, 8192, 8193, 65_536, 65_537, 100_003)
NEG0 = np.uint32(0x80000000)
WEIGHTS = [1.0, 0.5, 2.0, 1.25, 3.0]


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def same_bits(got, want):
    """int32 views equal, or both NaN."""
    g, w = got.detach().contiguous(), want.detach().contiguous()
    eq = (g.view(torch.int32) == w.view(torch.int32)) | (torch.isnan(g) & torch.isnan(w))
    return eq


def assert_same_bits(got, want, what=""):
    if torch.is_tensor(want) is False:
        want = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    eq = same_bits(got, want.reshape(got.shape))
    if not bool(eq.all()):
        bad = torch.nonzero(~eq.reshape(-1))[:5, 0].cpu().numpy()
        g, w = got.reshape(-1)[bad].cpu().numpy(), want.reshape(-1)[bad].cpu().numpy()
        raise AssertionError(f"{what}: {int((~eq).sum())} of {eq.numel()} elements differ; first {bad}: {g} vs {w}")


@functools.lru_cache(maxsize=None)
def inputs(n, d):
    """Gaussian a rows, b = a + N(0, 1) with every 13th difference zero: host arrays (read-only) and their
    device copies (cloned by every user), shared by the tests."""
    g = np.random.default_rng([n, d, 78])
    a = g.standard_normal((n, d)).astype(np.float32)
    b = (a + g.standard_normal((n, d))).astype(np.float32)
    b[:, ::13] = a[:, ::13]
    assert not (b.view(np.uint32) == NEG0).any()        # the in-place operand holds no -0
    for v in (a, b):
        v.setflags(write=False)
    return a, b, torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()


def compressor(ag, spec, d):
    comp = ag.initCompressor(spec, d)
    comp.dither_path = "sparse"
    return comp


def reducer(ag, spec, d):
    return ag.ShiftUplinkReducer(compressor(ag, spec, d), seed=SEED)


def call_shape(red, shape, ta, tb, **kw):
    """One round of the shape on the given device tensors (tb updated in place in A and B); returns out."""
    if shape == "A":
        out, m, h = red(ta, tb, alpha=ALPHA, shift=tb, shift_out=tb, **kw)
        assert m is None and h is tb
    elif shape == "B":
        out, m, h = red(ta, tb, scale=SCALE_B, base=tb, msg_out=tb, **kw)
        assert m is tb and h is None
    else:
        out, m, h = red(ta, tb, **kw)
        assert m is None and h is None
    return out


def both(ag, shape, spec, ha, hb, ld=None, **extra):
    """The one-read and the general round on clones of the device matrices ha, hb:
    ((out, rows, norms) one-read, (out, rows, norms) general)."""
    n, d = ha.shape
    assert not bool((hb.view(torch.int32) == -2 ** 31).any())            # no 0x80000000 in the in-place operand
    red = reducer(ag, spec, d)
    res = []
    for one_read in (True, False):
        if ld is None:
            ta, tb = ha.clone(), hb.clone()
        else:                                            # unaligned rows: views of [n, ld] storage
            sa, sb = (torch.full((n, ld), 7.0, dtype=torch.float32, device="cuda") for _ in range(2))
            ta, tb = sa[:, :d], sb[:, :d]
            ta.copy_(ha)
            tb.copy_(hb)
        pn = torch.full((n,), -1.0, device="cuda")
        out = call_shape(red, shape, ta, tb, one_read=one_read, pnorms_out=pn, **extra)
        if ld is not None:
            assert bool((sb[:, d:] == 7.0).all()) and bool((sa[:, d:] == 7.0).all())   # nothing past a row's end
        res.append((out, tb, pn))
    return res[0], res[1]


def assert_round_equal(one, gen, what):
    for name, g, w in zip(("out", "rows", "norms"), one, gen):
        assert_same_bits(g, w, f"{what} {name}")


# ------------------------------------------------------------------------------------------------
# 1. parity with the general entry
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_general_entry(ag, shape, n):
    for d in DS:
        _, _, ha, hb = inputs(n, d)
        for spec in SPECS:
            for weighted in (False, True):
                for client0 in (0, 11):
                    extra = {"client0": client0}
                    if weighted:
                        extra.update(weights=[WEIGHTS[i % 5] for i in range(n)], divisor=1.75)
                    one, gen = both(ag, shape, spec, ha, hb, **extra)
                    assert_round_equal(one, gen, f"shape {shape} {spec} n={n} d={d} weighted={weighted} client0={client0}")


# ------------------------------------------------------------------------------------------------
# 2. against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_oracle(ag, shape, n):
    spec, client0 = "qsgd:16", 11
    for d in (7, 8193, 100_003):
        a, b, ha, hb = inputs(n, d)
        msgs, rows, norms = [], [], []
        for i in range(n):
            o = oc.OracleCompressor(spec, d)
            o.testp = devrng.uniforms(SEED, client0 + i, d)
            norms.append(o.norm((a[i] - b[i]).astype(np.float32)))
            if shape == "A":
                m, h2 = oc.shift_step(o, a[i], b[i], alpha=ALPHA, h=b[i])
                rows.append(h2)
            elif shape == "B":
                m, _ = oc.shift_step(o, a[i], b[i], scale=SCALE_B, base=b[i])
                rows.append(m)
            else:
                m, _ = oc.shift_step(o, a[i], b[i])
                rows.append(b[i])
            msgs.append(m)
        ta, tb = ha.clone(), hb.clone()
        pn = torch.empty(n, device="cuda")
        out = call_shape(reducer(ag, spec, d), shape, ta, tb, one_read=True, client0=client0, pnorms_out=pn)
        what = f"shape {shape} n={n} d={d}"
        assert_same_bits(out, oc.reduce_plain(msgs), what + " out")
        assert_same_bits(tb, np.stack(rows), what + " rows")
        assert_same_bits(pn, np.array(norms, dtype=np.float32), what + " norms")


# ------------------------------------------------------------------------------------------------
# 3. which path ran
# ------------------------------------------------------------------------------------------------
PROFILED = ("k_ds_shift_lists", "k_ds_shift_dense_rows", "k_norm_partials", "k_ew_shift_accum", "k_ds_filter")


def row_flags(n, d):
    """DsWs.flags of the workspace the last one-read call on the current stream left."""
    from flpytorch_amd import _lib
    lib = _lib.load()
    ws = _lib.WORKSPACE.get(torch.device("cuda", torch.cuda.current_device()), 0)
    fl = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = lib.flc_dither_row_flags(n, d, ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(fl.data_ptr()),
                                  _lib.stream_ptr())
    _lib.check(rc, "flc_dither_row_flags")
    return fl.cpu().numpy()


def profiled_one_read(ag, shape, spec, ta, tb, **kw):
    from flpytorch_amd import _lib
    n, d = ta.shape
    red = reducer(ag, spec, d)
    _lib.profile_enable(True)
    try:
        for name in PROFILED:
            _lib.profile_collect(name)
        out = call_shape(red, shape, ta, tb, one_read=True, **kw)
        torch.cuda.synchronize()
        counts = {name: _lib.profile_collect(name)[1] for name in PROFILED}
    finally:
        _lib.profile_enable(False)
    return out, counts, row_flags(n, d)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_gaussian_rows_stay_sparse(ag, shape):
    """qsgd:4 at d = 300 001: about 4 * 0.798 / sqrt(d) * 8192 + 0.003 * 8192 = 73 candidates per 8192-element
    item against the 512-entry staging: no row may be flagged dense."""
    n, d = 5, 300_001
    _, _, ha, hb = inputs(n, d)
    _, gen = both(ag, shape, "qsgd:4", ha, hb)
    ta, tb = ha.clone(), hb.clone()
    out, counts, flags = profiled_one_read(ag, shape, "qsgd:4", ta, tb)
    assert not (flags & 1).any(), f"dense-flagged rows: {flags}"
    assert counts["k_ds_shift_lists"] == 1 and counts["k_ds_shift_dense_rows"] == 1 and counts["k_ds_filter"] == 1
    assert counts["k_norm_partials"] == 0 and counts["k_ew_shift_accum"] == 0
    assert_same_bits(out, gen[0], "out")
    assert_same_bits(tb, gen[1], "rows")


@pytest.mark.parametrize("shape", ["A", "B"])
def test_overflowing_rows_take_the_dense_epilogue(ag, shape):
    """qsgd:127 at the same d, forced sparse: about 1500 candidates per item, every item overflows, EVERY row
    is flagged dense — and the result still equals the general entry's."""
    n, d = 5, 300_001
    _, _, ha, hb = inputs(n, d)
    _, gen = both(ag, shape, "qsgd:127", ha, hb)
    ta, tb = ha.clone(), hb.clone()
    out, counts, flags = profiled_one_read(ag, shape, "qsgd:127", ta, tb)
    assert (flags & 1).all(), f"rows not flagged dense: {flags}"
    assert counts["k_norm_partials"] == 0 and counts["k_ew_shift_accum"] == 0
    assert_same_bits(out, gen[0], "out")
    assert_same_bits(tb, gen[1], "rows")


def kind_inputs(kind, n, d):
    """Rows of test_gpu_dither_sparse.py's kinds as differences: b = k / 2, a = b + k (a - b has k's character)."""
    k = make_rows(kind, n, d, np.random.default_rng(zlib.crc32(f"shift{kind}".encode())))
    b = (k * np.float32(0.5) + np.float32(0.0)).astype(np.float32)
    a = (b + k).astype(np.float32)
    b[b.view(np.uint32) == NEG0] = 0.0
    return torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


@pytest.mark.parametrize("kind", ["clustered", "sparse"])
@pytest.mark.parametrize("shape", ["A", "B"])
def test_mixed_paths(ag, shape, kind):
    n, d = 5, 300_001
    ha, hb = kind_inputs(kind, n, d)
    _, gen = both(ag, shape, "qsgd:4", ha, hb)
    ta, tb = ha.clone(), hb.clone()
    out, _, flags = profiled_one_read(ag, shape, "qsgd:4", ta, tb)
    what = f"{kind}: dense-flagged rows {np.flatnonzero(flags & 1).tolist()}"
    assert_same_bits(out, gen[0], what + " out")
    assert_same_bits(tb, gen[1], what + " rows")


# ------------------------------------------------------------------------------------------------
# 4. row kinds as differences
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["heavy", "negative", "ones", "tiny", "equal", "nan", "inf"])
@pytest.mark.parametrize("shape", ["A", "B", "D"])
def test_row_kinds(ag, shape, kind):
    n, d = 5, 300_001
    if kind in ("equal", "nan", "inf"):
        _, _, ha, hb = inputs(n, d)
        ha, hb = ha.clone(), hb.clone()
        if kind == "equal":
            ha[3] = hb[3]                                # a_i == b_i everywhere: norm 0
        elif kind == "nan":
            ha[1, 777] = float("nan")
        else:
            ha[2, 31] = float("inf")
    else:
        ha, hb = kind_inputs(kind, n, d)
    one, gen = both(ag, shape, "qsgd:4", ha, hb, weights=WEIGHTS)
    assert_round_equal(one, gen, f"{kind} shape {shape}")


# ------------------------------------------------------------------------------------------------
# 5. the contract
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B"])
def test_untouched_elements(ag, shape):
    """Elements whose encoded value is +-0 are not written: a -0 there survives (the general entry turns it
    into +0), every other element has the general entry's bits, and the written set is exactly e != 0."""
    n, d, spec = 5, 100_003, "qsgd:4"
    a, b, _, _ = inputs(n, d)
    a, b = a.copy(), b.copy()
    a[:, ::13] = -0.0                                    # v = (-0) - (-0) = +0 there: e is zero
    b[:, ::13] = -0.0
    ha, hb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    red = reducer(ag, spec, d)
    # e itself, from a general call that stores the messages (no base, scale 1: m = e)
    e = torch.empty_like(ha)
    red(ha.clone(), hb.clone(), msg_out=e)
    nz = e != 0
    assert bool((~nz[:, ::13]).all()) and 0.001 < float(nz.float().mean()) < 0.2
    gb, tb = hb.clone(), hb.clone()
    gout = call_shape(red, shape, ha.clone(), gb)
    out = call_shape(red, shape, ha.clone(), tb, one_read=True)
    was, got, gen = hb.view(torch.int32), tb.view(torch.int32), gb.view(torch.int32)
    assert bool((got[~nz] == was[~nz]).all())            # e == 0: the stored bits, -0 included
    assert bool((got[:, ::13] == -2 ** 31).all()) and bool((gen[:, ::13] == 0).all())
    assert bool((got[nz] == gen[nz]).all())              # e != 0: the general entry's bits
    assert bool((got != was).sum() > 0.5 * nz.sum())     # ... and they were written
    if shape == "A":
        assert_same_bits(out, gout, "out")               # the fold of the messages does not see b's zeros' signs
    else:
        assert bool(((out == gout) | (torch.isnan(out) & torch.isnan(gout))).all())   # B: at most a zero's sign


@pytest.mark.parametrize("pad", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_unaligned_rows(ag, shape, pad):
    n, d = 5, 100_003
    _, _, ha, hb = inputs(n, d)
    one, gen = both(ag, shape, "qsgd:16", ha, hb, ld=d + pad, weights=WEIGHTS)
    assert_round_equal(one, gen, f"shape {shape} ld = d + {pad}")
    ref, _ = both(ag, shape, "qsgd:16", ha, hb, weights=WEIGHTS)
    assert_round_equal(one, ref, f"shape {shape} ld = d + {pad} vs contiguous")


# ------------------------------------------------------------------------------------------------
# 6. Python surface
# ------------------------------------------------------------------------------------------------
def stats(comp):
    return (comp.total_input_components, comp.really_need_to_send_components, comp.last_input_advance,
            comp.last_need_to_send_advance)


def test_uplink_helpers_and_wire_statistics(ag):
    n, d, spec = 5, 30_011, "qsgd:4"
    _, _, ha, hb = inputs(n, d)
    for algo in ("diana", "ef21"):
        res = []
        for one_read in (True, False):
            ta, tb, comp = ha.clone(), hb.clone(), compressor(ag, spec, d)
            if algo == "diana":
                out = ag.dianaUplink(comp, ta, tb, ALPHA, seed=SEED, one_read=one_read, weights=WEIGHTS)
            else:
                out = ag.ef21Uplink(comp, ta, tb, seed=SEED, one_read=one_read, weights=WEIGHTS)
            res.append((out, tb, stats(comp)))
        assert_same_bits(res[0][0], res[1][0], algo + " out")
        assert_same_bits(res[0][1], res[1][1], algo + " rows")
        assert res[0][2] == res[1][2] and res[0][2][0] == n * d            # the wire statistics of N compressShift calls
        # ... and the reducer's own result
        ta, tb = ha.clone(), hb.clone()
        red = reducer(ag, spec, d)
        if algo == "diana":
            out, _, _ = red(ta, tb, alpha=ALPHA, shift=tb, shift_out=tb, one_read=True, weights=WEIGHTS)
        else:
            comp = compressor(ag, spec, d)
            mult = 1.0 if comp.isContractionCompressor() else 1.0 / (1.0 + comp.getW())
            out, _, _ = red(ta, tb, scale=mult, base=tb, msg_out=tb, one_read=True, weights=WEIGHTS)
        assert_same_bits(res[0][0], out, algo + " reducer out")
        assert_same_bits(res[0][1], tb, algo + " reducer rows")
    with pytest.raises(NotImplementedError):
        ag.marinaUplink(compressor(ag, spec, d), ha.clone(), hb.clone(), ha[0].clone(), seed=SEED, one_read=True)


def test_refusals(ag):
    n, d = 5, 30_011
    _, _, ha, hb = inputs(n, d)
    for spec in ("topk:1%", "randk:1%", "natural", "qsgd:4"):
        comp = ag.initCompressor(spec, d)
        if spec == "qsgd:4":
            comp.p = 1                                   # standard dithering, but not p = 2
        with pytest.raises(NotImplementedError, match="QSGD"):
            ag.ShiftUplinkReducer(comp, seed=SEED)(None, None, one_read=True)      # before any operand is looked at
    red = reducer(ag, "qsgd:4", d)
    u = torch.zeros((n, d), dtype=torch.float64, device="cuda")
    for kw in ({"sparse": True}, {"batched": True}, {"uniforms": u}, {"randk_counts": u}):
        with pytest.raises(ValueError):
            red(ha, hb.clone(), one_read=True, **kw)
    for kw in ({"sparse": True}, {"batched": True}):     # QSGD keeps being refused there exactly as before
        with pytest.raises(NotImplementedError):
            red(ha, hb.clone(), **kw)
    # library refusals surface with the library's reason and leave b and the statistics untouched
    tb = hb.clone()
    with pytest.raises(NotImplementedError, match="MARINA"):
        red(ha, tb, base=ha[0].clone(), one_read=True)
    with pytest.raises(NotImplementedError, match="msg_scale"):
        red(ha, tb, alpha=ALPHA, shift=tb, shift_out=tb, scale=0.5, one_read=True)
    dense = compressor(ag, "qsgd:4", d)
    dense.dither_path = "dense"
    with pytest.raises(NotImplementedError, match="FLC_PATH_DENSE"):
        ag.ShiftUplinkReducer(dense, seed=SEED)(ha, tb, alpha=ALPHA, shift=tb, shift_out=tb, one_read=True)
    torch.cuda.synchronize()
    assert_same_bits(tb, hb, "b after refused calls")
    assert stats(red.comp) == stats(compressor(ag, "qsgd:4", d)) and stats(dense) == stats(compressor(ag, "qsgd:4", d))
    assert red.workspace_bytes(n, d, one_read=True) > red.workspace_bytes(n, d) > 0


@pytest.mark.parametrize("shape", SHAPES)
def test_side_stream(ag, shape):
    n, d = 130, 100_003                                  # two row groups: the library's own side stream as well
    _, _, ha, hb = inputs(n, d)
    one, _ = both(ag, shape, "qsgd:16", ha, hb, weights=[WEIGHTS[i % 5] for i in range(n)])
    side = torch.cuda.Stream()
    ta, tb = ha.clone(), hb.clone()
    torch.cuda.synchronize()
    sout = call_shape(reducer(ag, "qsgd:16", d), shape, ta, tb, one_read=True, weights=[WEIGHTS[i % 5] for i in range(n)],
                      stream=side)
    side.synchronize()
    assert_same_bits(sout, one[0], "out")
    assert_same_bits(tb, one[1], "rows")
