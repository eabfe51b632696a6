"""The oracle against the REAL reference at IEEE edge values (CPU only).

Fixtures: tests/golden/edges.{npz,json}, made by tests/golden/make_golden_edges.py from the
reference's own compressVector (torch CPU) on the rows of tests/edge_rows.py: subnormals, every
power of two with its neighbours, FLT_MAX, +-inf, NaN, norms that are subnormal, inf or NaN, elements on
and next to every dithering level, draws on and next to every probability.  The rows and uniforms are
regenerated here and checked against the recorded digests first.

Bar: NaN positions equal, every other element equal as uint32.  Dithering is compared given the
reference's norm (torch's CPU norm is not the exactly rounded one; tests/test_gpu_rows_ref.py).
Two things this file caught in oracle/codecs.py: np.exp2 is one ulp off at some integral exponents
(2^127 -> 0x7F000001; natural on `span`), and np.sign(NaN) is NaN where torch.sign gives 0 (a NaN
element under a given finite norm: the levels rows).
"""
import math

import numpy as np
import pytest

from oracle import codecs as oc
from oracle import wire
from tests import edge_rows as er
from tests.golden_io import load

META, ARR = load("edges")
CASES = META["cases"]
ORACLE_ONLY_KINDS = er.KINDS + list(er.LEVEL_KINDS)


def assert_same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ at {np.flatnonzero(gn != wn)[:8]}"
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero((g != w) & ~gn)
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} elements differ; first {bad[:5]}: "
                           f"{[hex(v) for v in g[bad[:5]]]} vs {[hex(v) for v in w[bad[:5]]]}")


def oracle_case(key):
    """(compressor with the case's pattern, row, the reference's norm or None) of a fixture case, the
    regenerated inputs checked against the fixture's digests."""
    m = CASES[key]
    x = er.row(m["kind"], m["spec"])
    assert er.sha(x) == m["x_sha"], "row regeneration differs from the fixture's"
    o = oc.OracleCompressor(m["spec"], er.D)
    if "u_sha" in m:
        o.testp = er.uniforms(m["kind"], m["spec"], x)
        assert er.sha(o.testp) == m["u_sha"], "uniform regeneration differs from the fixture's"
    if "lazy_u" in m:
        o.testp = m["lazy_u"]
    pn = np.uint32(m["pnorm_bits"]).view(np.float32) if "pnorm_bits" in m else None
    return o, x, pn


def test_edge_rows_hold_what_they_claim():
    v = er.edge_values()
    b = v.view(np.uint32)
    for pat in (1, 2, 0x007FFFFF, 0x00800000, 0x00800001, 0x7F7FFFFE, 0x7F7FFFFF):
        assert pat in b and (pat | 0x80000000) in b
    for k in (-149, -127, -126, -80, -40, 0, 80, 127):
        p = int(np.ldexp(np.float32(1), k).astype(np.float32).view(np.uint32))
        assert {p - 1, p, p + 1} <= set(b.tolist())
    assert np.all(np.isfinite(v)) and v.size == 2 * (7 + 3 * 277 + 1500)
    mid = er.mid_values()
    assert mid.size > 500 and np.abs(mid).min() > 2.0 ** -20 and np.abs(mid).max() < 2.0 ** 20
    for kind in er.KINDS:
        assert er.row(kind).shape == (er.D,)
    # the regimes the kinds exist for
    n2 = oc.OracleCompressor("qsgd:8", er.D).norm
    assert np.isinf(n2(er.row("span"))) and np.all(np.isfinite(er.row("span")))
    assert 0 < n2(er.row("mid-100")) < 2.0 ** -40 and n2(er.row("mid+90")) > 2.0 ** 80
    m140 = er.row("mid-140")
    assert 0 < n2(m140) < 2.0 ** -100 and np.sum((m140 != 0) & (np.abs(m140) < 2.0 ** -126)) > 100
    assert 0 < n2(er.row("mid-160")) < 2.0 ** -126
    t = er.row("tinyone")
    assert 2.0 ** -40 <= n2(t) <= 2.0 ** 80 and np.sum((t != 0) & (np.abs(t) < 2.0 ** -80)) == 1
    assert np.isnan(n2(er.row("nan+"))) and np.isinf(n2(er.row("inf")))
    assert np.signbit(er.row("nan-")[1]) and not np.signbit(er.row("nan+")[1])
    assert np.count_nonzero(er.row("one")) == 1


@pytest.mark.parametrize("key", sorted(CASES))
def test_oracle_vs_reference_edges(key):
    o, x, pn = oracle_case(key)
    m = CASES[key]
    out = o.compress(x, pnorm=pn)
    if m["spec"] == "ident":
        assert er.sha(out) == m["out_sha"]
    else:
        assert_same(out, ARR[key], key)


@pytest.mark.parametrize("kind", er.KINDS)
@pytest.mark.parametrize("p", [1, 2, math.inf])
def test_oracle_norm_edges(kind, p):
    """oc.norm == the float64 restatement, rounded once: sums of at most 8195 fp32 values (squares)
    neither overflow nor lose a bit that matters in float64 except by the final rounding; the p = 2
    sum is done here in exact integer arithmetic to say so without relying on float64 at all."""
    from fractions import Fraction
    x = er.row(kind)
    o = oc.OracleCompressor("std.dithering:8:%s" % ("inf" if p == math.inf else p), er.D)
    got = o.norm(x)
    if np.isnan(x).any():
        assert np.isnan(got)
        return
    if np.isinf(x).any():
        assert got == np.inf
        return
    ax = [Fraction(float(v)) for v in np.abs(x)]
    if p == math.inf:
        exact = max(ax)
    elif p == 1:
        exact = sum(ax)
    else:
        exact = sum(v * v for v in ax)
    with np.errstate(all="ignore"):
        if p == 2:
            # RN32(sqrt(RN64(exact))): the oracle's definition; the exact sum rounds to float64 once
            want = np.float32(np.sqrt(np.float64(float(exact)) if exact < Fraction(2) ** 1024 else np.inf))
        else:
            want = np.float32(np.float64(float(exact)))
    assert got.view(np.uint32) == want.view(np.uint32), (kind, p, got, want)


WIRE_SPECS = ["natural", "qsgd:8", "std.dithering:300:2", "std.dithering:8:1", "terngrad", "ident"]


@pytest.mark.parametrize("key", sorted(k for k in CASES if CASES[k]["spec"] in WIRE_SPECS))
def test_oracle_wire_round_trip_edges(key):
    """oracle.wire.unpack(pack(out)) == out on every oracle output of these rows: NaN by position
    (the level codes and NAT16 carry "a NaN", not its bits), everything else bit for bit, no element
    without a code (hdr.bad == 0) — the subnormal-norm rows included, where several levels give the
    same product and any of their codes decodes to the same bits."""
    o, x, pn = oracle_case(key)
    if pn is None and hasattr(o, "p"):
        pn = o.norm(x)
    out = o.compress(x, pnorm=pn)
    buf = wire.pack(o, out, pnorm=pn)
    if wire.payload_format(o) in (wire.Q8, wire.Q16):
        assert buf[12:16].view(np.uint32)[0] == 0, "elements without a level code"
    assert_same(wire.unpack(o, buf, er.D), out, key)


SHIFT_SPECS = ["natural", "qsgd:8", "std.dithering:5", "nat.dithering:6:2"]


@pytest.mark.parametrize("kind", ORACLE_ONLY_KINDS)
@pytest.mark.parametrize("spec", SHIFT_SPECS)
def test_oracle_shift_step_edges(spec, kind):
    """shift_step(a, b) == compress(a - b) where a - b IS the edge row (exact fp32 difference)."""
    if kind in er.LEVEL_KINDS and not er.dither_spec(spec):
        kind = "span"
    x = er.row(kind, spec)
    a, b = er.shift_operands(x)
    o = oc.OracleCompressor(spec, er.D)
    o.testp = er.uniforms(kind, spec, x)
    pn = er.given_norm(kind)
    want = o.compress(x, pnorm=pn)
    msg, h2 = oc.shift_step(o, a, b, scale=1.0, alpha=1.0, h=np.zeros(er.D, dtype=np.float32), pnorm=pn)
    assert_same(msg, want, f"{spec} {kind} msg")
    with np.errstate(all="ignore"):
        assert_same(h2, (np.float32(0) + want).astype(np.float32), f"{spec} {kind} shift")
