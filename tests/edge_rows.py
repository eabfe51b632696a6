"""Shared rows of the edge-value tests (tests/test_oracle_edges.py, tests/test_gpu_edges.py) and of
tests/golden/make_golden_edges.py, which records the reference's outputs on them in
tests/golden/edges.{npz,json}.  Everything is seeded; the fixture holds a sha256 of every row and
uniform vector, and the tests check the regenerated ones against it first.

Every row has D = 8195 elements: two 4096-element norm partials, four 2048-element tiles of the
tile-owner kernels and a three-element scalar tail.  The special elements of a kind sit in the first
float4 group, across index 4095 / 4096 and in the tail.

Row kinds (KINDS, and LEVEL_KINDS for the dithering codecs, encoded with the GIVEN norm 2^m):
  span      edge_values() cycled: subnormals, every 2^k with its neighbours, FLT_MAX, random bits
            (p = 1 and p = 2 norms overflow to inf from finite elements)
  mid       the values with 2^-20 < |x| < 2^20, cycled
  mid-100 / mid+90 / mid-140   mid * 2^m: norm below / above the fast-division window, and
            subnormal elements under a small normal norm
  mid-160   every element and the norm subnormal: level * norm products that collide
  tinyone   mid with one element 2^-100: norm inside the window, a nonzero element below 2^-80
  nan+ / nan-   mid with 0x7FC00000 / 0xFFC00000;   inf: mid with +inf and -inf
  zeros     +0 with some -0;   one: a single nonzero element (y == 1)
  lev0 / lev-60   levels(spec, m): +-lv[k] * 2^m with its two neighbouring floats for every level
            of the codec, three elements above 2^m (y > 1), a NaN of each sign and -0
"""
import hashlib

import numpy as np

from oracle import codecs as oc

D = 8195
KINDS = ["span", "mid", "mid-100", "mid+90", "mid-140", "mid-160", "tinyone", "nan+", "nan-", "inf", "zeros", "one"]
LEVEL_KINDS = {"lev0": 0, "lev-60": -60}
SPECIAL = (1, 4095, 4096, 8193)          # first float4 group, both sides of the partial seam, the tail
_F = np.float32


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(_F)


def edge_values():
    """The bit patterns of the issue, each with both signs, shuffled by a fixed seed."""
    pats = [0x00000001, 0x00000002, 0x007FFFFF, 0x00800000, 0x00800001, 0x7F7FFFFE, 0x7F7FFFFF]
    for k in range(-149, 128):
        b = int(np.ldexp(_F(1), k).astype(_F).view(np.uint32))
        pats += [b - 1, b, b + 1]
    g = np.random.default_rng(20250)
    pats = np.concatenate([np.array(pats, dtype=np.uint32), g.integers(0, 0x7F800000, 1500, dtype=np.uint32)])
    pats = np.concatenate([pats, pats | np.uint32(0x80000000)])
    g.shuffle(pats)
    return f32(pats).copy()


def mid_values():
    v = edge_values()
    a = np.abs(v)
    return v[(a > _F(2.0 ** -20)) & (a < _F(2.0 ** 20))].copy()


def _cycle(v, d=D):
    return np.resize(v, d).astype(_F)


def dither_spec(spec):
    return spec.split(":")[0] in ("qsgd", "std.dithering", "terngrad", "nat.dithering")


def levels_row(spec, m):
    lv = oc.OracleCompressor(spec, D).levels
    with np.errstate(all="ignore"):
        base = np.ldexp(lv, m).astype(_F)                       # exact: 2^m scales no level into the subnormals
    b = base.view(np.uint32).astype(np.int64)
    mag = np.concatenate([np.maximum(b - 1, 0), b, b + 1]).astype(np.uint32)
    vals = np.concatenate([mag, mag | np.uint32(0x80000000)])
    np.random.default_rng([7, abs(m), len(lv)]).shuffle(vals)
    x = _cycle(f32(vals))
    one = np.ldexp(_F(1), m)
    x[0], x[4095], x[8194] = np.nextafter(one, _F(np.inf)), -_F(1.5) * one, _F(3.0) * one     # y > 1
    x[1], x[4096] = f32(0x7FC00000), f32(0xFFC00000)
    x[2], x[8193] = _F(-0.0), _F(-0.0)
    return x


def row(kind, spec=None):
    if kind in LEVEL_KINDS:
        return levels_row(spec, LEVEL_KINDS[kind])
    if kind == "span":
        return _cycle(edge_values())
    if kind == "zeros":
        x = np.zeros(D, dtype=_F)
        x[[0, 3, 4095, 4096, 8192, 8194]] = _F(-0.0)
        x[np.random.default_rng(11).integers(0, D, 500)] = _F(-0.0)
        return x
    if kind == "one":
        x = np.zeros(D, dtype=_F)
        x[4096] = _F(-0.1875)
        return x
    x = _cycle(mid_values())
    if kind == "mid":
        return x
    if kind.startswith("mid"):
        with np.errstate(all="ignore"):
            return np.ldexp(x, int(kind[3:])).astype(_F)
    if kind == "tinyone":
        x[4095] = _F(2.0 ** -100)
    elif kind == "nan+":
        x[list(SPECIAL)] = f32(0x7FC00000)
    elif kind == "nan-":
        x[list(SPECIAL)] = f32(0xFFC00000)
    elif kind == "inf":
        x[[1, 4096]] = _F(np.inf)
        x[[4095, 8193]] = _F(-np.inf)
    else:
        raise ValueError(kind)
    return x


def given_norm(kind):
    """The norm a levels row is encoded with (None: the codec's own)."""
    return _F(2.0 ** LEVEL_KINDS[kind]) if kind in LEVEL_KINDS else None


def uniforms(kind, spec, x=None):
    """Compat draws of a row: a seeded rand(D) whose first 50 draws are 0.0; on the levels rows, and
    on span for natural, a third each of the draws are p, nextafter(p, 0) and nextafter(p, 1) for the
    element's fp32 probability p (the `testp < p` compare at and next to equality), wherever p is
    a number in [0, 1]."""
    g = np.random.default_rng([99, (list(LEVEL_KINDS) + KINDS).index(kind)])
    u = g.random(D)
    sel = g.integers(0, 3, D)
    if kind in LEVEL_KINDS or (kind == "span" and spec == "natural"):
        x = row(kind, spec) if x is None else x
        p = oc.OracleCompressor(spec, D).probability(x, given_norm(kind)).astype(np.float64)
        ok = (p >= 0.0) & (p <= 1.0)
        alt = np.where(sel == 0, p, np.where(sel == 1, np.nextafter(p, 0.0), np.nextafter(p, 1.0)))
        u = np.where(ok, alt, u)
    u[:50] = 0.0
    return u


def shift_operands(x):
    """(a, b) with fl(a - b) == x bit for bit: b = c, a = x + c with, per element,
    c = -sign(x) * 2^floor(log2 |x|).  |x| / 2 < |c| <= |x|, so x + c is exact (Sterbenz, subnormals
    included) and a - c gives x back exactly.  Zeros, infinities and NaN get c = 0."""
    x = np.asarray(x, dtype=_F)
    with np.errstate(all="ignore"):
        fin = np.isfinite(x) & (x != 0)
        _, e = np.frexp(np.where(fin, x, _F(1)))
        c = -np.copysign(np.ldexp(_F(1), (e - 1).astype(np.int32)), x).astype(_F)
        c = np.where(fin, c, _F(0)).astype(_F)
        a = np.where(fin, x + c, x).astype(_F)
        assert np.array_equal((a - c).astype(_F).view(np.uint32), x.view(np.uint32))
    return a, c
