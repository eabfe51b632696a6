"""The elementwise codecs at IEEE edge values on every kernel path, against the pinned oracle.

The rows are those of tests/edge_rows.py (D = 8195: two norm partials, four 2048-element tiles, a
three-element tail): subnormals, every power of two with its neighbours, FLT_MAX, +-inf, NaN, norms
below and above the fast-division window [2^-40, 2^80], a subnormal norm, an inf and a NaN norm, a
lone element below 2^-80 (rowfast == 0: the guarded division, the F = false instantiation of every
kernel), and — with a GIVEN norm — elements on and next to every level with draws on and next to
every probability.  The oracle is pinned to the reference's own outputs on exactly these rows by
tests/test_oracle_edges.py (tests/golden/edges.*), so it is the reference here.

The standing rule of every test: NaN positions equal, every other element equal as uint32, norms
(pnorm_out / pnorms_out) equal in the same sense.  No element is left out.  Each test stacks the 12
row kinds as the rows of one call (fused entries) or walks them one call each (lone entries); every
test therefore runs rows with rowfast == 0 (span, mid-100, mid+90, mid-140, mid-160, tinyone, nan,
inf) next to rows on the fast path (mid, one).  Mismatches are collected over all rows of a test and
reported together.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import codecs as oc
from oracle import devrng
from oracle import wire
from tests import edge_rows as er
from tests.golden_io import load

pytestmark = pytest.mark.gpu

D, KINDS = er.D, er.KINDS
N = len(KINDS)
LD = 8196                                    # row stride of the vector path (a multiple of 4)
SEED, CLIENT0 = 20250, 5
ALPHA, SCALE = 0.75, 0.25
WEIGHTS = [1.0, -0.75, 0.0, 3.3333333333333335, 0.5, 2.0, 1.25, 1.0, 0.125, 1.5, 0.25, 2.5]
LAZY_U = [0.25, 0.75] * (N // 2)
STD = ["qsgd:8", "std.dithering:8:1", "std.dithering:5", "terngrad"]          # p = 2, 1, inf, inf
EDGE_META = load("edges")[0]["cases"]


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
class Errs(list):
    """Collects the mismatches of one test; `done()` asserts there are none."""

    def same(self, got, want, what):
        got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
        got = np.asarray(got, dtype=np.float32).reshape(-1)
        want = np.asarray(want, dtype=np.float32).reshape(-1)
        gn, wn = np.isnan(got), np.isnan(want)
        g, w = got.view(np.uint32), want.view(np.uint32)
        bad = np.flatnonzero((gn != wn) | ((g != w) & ~gn & ~wn))
        if bad.size:
            self.append(f"{what}: {bad.size} of {g.size} differ; first {bad[:4].tolist()}: "
                        f"{[hex(v) for v in g[bad[:4]]]} vs {[hex(v) for v in w[bad[:4]]]}")

    def true(self, cond, what):
        if not cond:
            self.append(what)

    def done(self):
        assert not self, "\n".join(self[:40])


class Ran:
    """Launch counts of named kernels over a block (flc_profile_collect), as _FilterVariants in
    tests/test_gpu_parity.py."""

    def __init__(self, *names):
        self.names, self.count = names, {}

    def __enter__(self):
        from flpytorch_amd import _lib
        self._lib = _lib
        _lib.profile_enable(True)
        for k in self.names:
            _lib.profile_collect(k)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.count = {k: self._lib.profile_collect(k)[1] for k in self.names}
        self._lib.profile_enable(False)
        return False

    def check(self):
        for k in self.names:
            assert self.count[k] >= 1, f"{k} did not run ({self.count})"


def otype(spec):
    return oc.OracleCompressor(spec, D).type


def drawn(spec):
    return otype(spec) in (oc.NATURAL, oc.STD_DITHERING)          # natural dithering ignores its draws


def dithering(spec):
    return otype(spec) in (oc.STD_DITHERING, oc.NAT_DITHERING)


def modes_of(spec):
    return ("compat", "device") if drawn(spec) else ("compat",)


@functools.lru_cache(maxsize=None)
def rows_of(spec=None, levels=False):
    """The edge rows (read-only), checked against the fixture's digests where it holds them."""
    kinds = list(er.LEVEL_KINDS) if levels else KINDS
    xs = [er.row(k, spec) for k in kinds]
    for k, x in zip(kinds, xs):
        for m in EDGE_META.values():
            if m["kind"] == k and (not levels or m["spec"] == spec):
                assert er.sha(x) == m["x_sha"], f"row {k} differs from the fixture's"
                break
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def ref(spec, mode="compat", levels=False):
    """Per row: (x, draws, norm used, oracle output).  compat: the seeded uniforms of edge_rows
    (draws at 0.0 and, on the levels rows and natural's span, on and next to each probability);
    device: the host mirror of the kernels' counter-based draws of client CLIENT0 + i."""
    kinds = list(er.LEVEL_KINDS) if levels else KINDS
    out = []
    for i, (k, x) in enumerate(zip(kinds, rows_of(spec if levels else None, levels))):
        o = oc.OracleCompressor(spec, D)
        u = None
        if o.type == oc.LAZY:
            u = o.testp = LAZY_U[i]
        elif o.type in (oc.NATURAL, oc.STD_DITHERING, oc.NAT_DITHERING):
            u = o.testp = er.uniforms(k, spec, x) if mode == "compat" else devrng.uniforms(SEED, CLIENT0 + i, D)
        pn = None
        if dithering(spec):
            pn = er.given_norm(k) if levels else o.norm(x)
        e = o.compress(x, pnorm=pn)
        e.setflags(write=False)
        out.append((x, u, pn, e))
    return out


def comp_for(ag, spec, mode, i, u):
    c = ag.initCompressor(spec, D)
    if mode == "device":
        c.device_rng = (SEED, CLIENT0 + i)
    elif otype(spec) == oc.LAZY:
        c.testp = u
    elif u is not None:
        c.testp = torch.from_numpy(u.copy())
    if dithering(spec) and getattr(c, "p", None) == 2:
        c.dither_path = "dense"              # the elementwise fold, never the sparse QSGD pipeline
    return c


def gpu(x, off=0):
    """The row on the device: 16-byte aligned (off = 0) or a view `off` floats past alignment."""
    buf = torch.empty(D + 4, dtype=torch.float32, device="cuda")
    v = buf[off:off + D]
    v.copy_(torch.from_numpy(np.array(x, dtype=np.float32)))       # (a writable copy: the rows are read-only)
    assert v.data_ptr() % 16 == 4 * off
    return v


def matrix(rows, off=0, ld=LD):
    """[n, D] device matrix with row stride ld, its first row `off` floats past 16-byte alignment."""
    n = len(rows)
    buf = torch.zeros(n * ld + 4, dtype=torch.float32, device="cuda")
    m = buf[off:off + n * ld].view(n, ld)[:, :D]
    m.copy_(torch.from_numpy(np.stack(rows)))
    assert m.data_ptr() % 16 == 4 * off and m.stride(0) == ld
    return m


def pattern_kw(spec, mode, rs):
    """UplinkReducer / ShiftUplinkReducer pattern keywords of the stacked rows."""
    if otype(spec) == oc.LAZY:
        return {"lazy_u": torch.tensor([r[1] for r in rs], dtype=torch.float64, device="cuda")}
    if mode == "compat" and otype(spec) in (oc.NATURAL, oc.STD_DITHERING, oc.NAT_DITHERING):
        return {"uniforms": torch.from_numpy(np.stack([r[1] for r in rs])).cuda()}
    return {"client0": CLIENT0}


def fold(encs, w=None):
    with np.errstate(all="ignore"):
        return oc.reduce_plain(list(encs), w)


# ------------------------------------------------------------------------------------------------
# k_ew_dense: compressVector of natural / lazy / ident / natural dithering; standard dithering with a
# given norm; standard dithering on a 4-byte-offset view (which bypasses k_lone_dither)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["natural", "bernulli:0.5", "ident", "nat.dithering:6:2"])
def test_dense_encode_edges(ag, spec):
    errs = Errs()
    for mode in modes_of(spec):
        for i, (x, u, pn, e) in enumerate(ref(spec, mode)):
            for off in (0, 1):
                c = comp_for(ag, spec, mode, i, u)
                got = c.compressVector(gpu(x, off))
                errs.same(got, e, f"{spec} {mode} {KINDS[i]} off{off}")
            if dithering(spec):
                pno = torch.empty(1, device="cuda")
                got = comp_for(ag, spec, mode, i, u)._encode_gpu(gpu(x), pnorm_out=pno)
                errs.same(got, e, f"{spec} {mode} {KINDS[i]} own norm")
                errs.same(pno, [pn], f"{spec} {KINDS[i]} pnorm_out")
    errs.done()


@pytest.mark.parametrize("spec", STD + ["std.dithering:300:2", "nat.dithering:6:2"])
def test_dense_encode_given_norm_edges(ag, spec):
    """flc_encode with d_pnorm_in: the 12 kinds under the oracle's own norm (finite, subnormal, inf
    and NaN norms), and the levels rows under 2^0 and 2^-60: elements on and next to every level
    ("later interval wins on a boundary"), y > 1 ("lies in no interval"), draws on and next to every
    probability (`testp < p` at equality), a NaN of each sign under a finite norm (+0, the
    reference's bits) and -0."""
    errs = Errs()
    for mode in modes_of(spec):
        for levels in (False, True):
            kinds = list(er.LEVEL_KINDS) if levels else KINDS
            for i, (x, u, pn, e) in enumerate(ref(spec, mode, levels)):
                pin = torch.tensor([pn], dtype=torch.float32, device="cuda")
                pno = torch.empty(1, device="cuda")
                got = comp_for(ag, spec, mode, i, u)._encode_gpu(gpu(x), pnorm_in=pin, pnorm_out=pno)
                errs.same(got, e, f"{spec} {mode} {kinds[i]}")
                errs.same(pno, [pn], f"{spec} {mode} {kinds[i]} pnorm_out")
                if levels:
                    nanpos = np.flatnonzero(np.isnan(x))
                    errs.true(nanpos.size == 2 and np.all(got.cpu().numpy().view(np.uint32)[nanpos] == 0)
                              or otype(spec) == oc.NAT_DITHERING, f"{spec} {kinds[i]}: NaN under a finite norm is not +0")
    errs.done()


@pytest.mark.parametrize("spec", STD)
def test_dense_encode_unaligned_own_norm_edges(ag, spec):
    """Standard dithering with its own norm on a view 4 bytes past alignment: the scalar norm
    partials and k_ew_dense, not k_lone_dither."""
    errs = Errs()
    with Ran("k_norm_partials") as ran:
        for mode in modes_of(spec):
            for i, (x, u, pn, e) in enumerate(ref(spec, mode)):
                pno = torch.empty(1, device="cuda")
                got = comp_for(ag, spec, mode, i, u)._encode_gpu(gpu(x, 1), pnorm_out=pno)
                errs.same(got, e, f"{spec} {mode} {KINDS[i]}")
                errs.same(pno, [pn], f"{spec} {mode} {KINDS[i]} pnorm_out")
    ran.check()
    errs.done()


# ------------------------------------------------------------------------------------------------
# k_lone_dither: compressVector of standard dithering with its own norm, aligned
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", STD)
def test_lone_dither_edges(ag, spec):
    errs = Errs()
    with Ran("k_norm_partials") as ran:
        for mode in modes_of(spec):
            for i, (x, u, pn, e) in enumerate(ref(spec, mode)):
                c = comp_for(ag, spec, mode, i, u)
                errs.same(c.compressVector(gpu(x)), e, f"{spec} {mode} {KINDS[i]} compressVector")
                pno = torch.empty(1, device="cuda")
                got = comp_for(ag, spec, mode, i, u)._encode_gpu(gpu(x), pnorm_out=pno)
                errs.same(got, e, f"{spec} {mode} {KINDS[i]}")
                errs.same(pno, [pn], f"{spec} {mode} {KINDS[i]} pnorm_out")
    ran.check()
    errs.done()


# ------------------------------------------------------------------------------------------------
# k_ew_accum_vec + k_ew_accum_scalar: the fused uplink over the 12 kinds
# ------------------------------------------------------------------------------------------------
UPLINK = ["natural", "qsgd:8", "std.dithering:8:1", "std.dithering:5", "terngrad", "nat.dithering:6:2", "ident",
          "bernulli:0.5"]


@pytest.mark.parametrize("spec", UPLINK)
def test_uplink_edges(ag, spec):
    """UplinkReducer on the matrix (vector tiles + scalar tail), on the pointer list and on unaligned
    row views (the scalar kernel only); weights None and mixed with one negative and one zero.
    Compat uniforms with dither_path = "dense" keep qsgd on the elementwise fold (asserted: the
    tile-owner kernel ran); device draws likewise."""
    errs = Errs()
    for mode in modes_of(spec):
        rs = ref(spec, mode)
        xs, encs = [r[0] for r in rs], [r[3] for r in rs]
        kw = pattern_kw(spec, mode, rs)
        red = ag.UplinkReducer(comp_for(ag, spec, "compat", 0, None), seed=SEED if mode == "device" else None)
        aligned = matrix(xs)
        # (ident is the plain fold of the rows: flc_reduce_matrix's kernel, no codec pass)
        names = (("k_ew_accum_vec",) if spec != "ident" else ()) + (("k_norm_partials",) if dithering(spec) else ())
        for w in (None, WEIGHTS):
            want = fold(encs, w)
            with Ran(*names) as ran:
                pno = torch.empty(N, device="cuda")
                got = red(aligned, weights=w, pnorms_out=pno if dithering(spec) else None, **kw)
            ran.check()
            errs.same(got, want, f"{spec} {mode} matrix w={w is not None}")
            if dithering(spec):
                errs.same(pno, [r[2] for r in rs], f"{spec} {mode} pnorms_out")
            errs.same(red([gpu(x) for x in xs], weights=w, **kw), want, f"{spec} {mode} pointers w={w is not None}")
            for m in (matrix(xs, off=1), matrix(xs, ld=D)):          # 4 bytes past alignment; ld % 4 != 0
                errs.same(red(m, weights=w, **kw), want, f"{spec} {mode} unaligned w={w is not None}")
    errs.done()


@pytest.mark.parametrize("spec", STD + ["nat.dithering:6:2"])
def test_uplink_given_norms_edges(ag, spec):
    """pnorms_in: the 12 kinds under the oracle's norms stacked with the two levels rows under 2^0 and
    2^-60 (n = 14).  Given norms take the guarded division on every row."""
    errs = Errs()
    for mode in modes_of(spec):
        rs = ref(spec, mode) + ref(spec, mode, True)
        if mode == "device":          # the levels rows are clients CLIENT0 + 12, + 13 of the stacked call
            rs = list(rs)
            for j, k in enumerate(er.LEVEL_KINDS):
                x, _, pn, _ = rs[N + j]
                o = oc.OracleCompressor(spec, D)
                o.testp = devrng.uniforms(SEED, CLIENT0 + N + j, D)
                rs[N + j] = (x, o.testp, pn, o.compress(x, pnorm=pn))
        xs, encs = [r[0] for r in rs], [r[3] for r in rs]
        pin = torch.tensor([float(r[2]) for r in rs], dtype=torch.float32, device="cuda")
        kw = pattern_kw(spec, mode, rs)
        red = ag.UplinkReducer(comp_for(ag, spec, "compat", 0, None), seed=SEED if mode == "device" else None)
        w = WEIGHTS + [1.0, 0.5]
        with Ran("k_ew_accum_vec") as ran:
            pno = torch.empty(len(rs), device="cuda")
            got = red(matrix(xs), weights=w, pnorms_in=pin, pnorms_out=pno, **kw)
        ran.check()
        errs.same(got, fold(encs, w), f"{spec} {mode} matrix")
        errs.same(pno, [r[2] for r in rs], f"{spec} {mode} pnorms_out")
        errs.same(red(matrix(xs, ld=D), pnorms_in=pin, **kw), fold(encs), f"{spec} {mode} scalar kernel")
        # the levels rows by themselves (one row, divisor 1: the encode itself, NaN -> +0 included)
        for j, k in enumerate(er.LEVEL_KINDS):
            x, u, pn, e = ref(spec, "compat", True)[j]
            one = red(matrix([x]), uniforms=torch.from_numpy(u.copy()).cuda().view(1, -1) if drawn(spec) else None,
                      pnorms_in=pin[N + j:N + j + 1]) if mode == "compat" else None
            if one is not None:
                errs.same(one, fold([e]), f"{spec} {k} one row")
    errs.done()


# ------------------------------------------------------------------------------------------------
# k_ew_shift: compressShift whose difference a - b IS the edge row (exact in fp32)
# ------------------------------------------------------------------------------------------------
SHIFT = ["natural", "qsgd:8", "std.dithering:8:1", "std.dithering:5", "nat.dithering:6:2", "bernulli:0.5"]


@functools.lru_cache(maxsize=None)
def shift_inputs():
    """Per kind (a, b) with fl(a - b) == the edge row, and one shared base vector."""
    ab = [er.shift_operands(x) for x in rows_of()]
    gp = np.random.default_rng(77).standard_normal(D).astype(np.float32)
    gp[[0, 4095, 8194]] = [-0.0, np.inf, 0.0]
    gp.setflags(write=False)
    return ab, gp


def shift_want(spec, mode, i, a, b, **kw):
    x, u, pn, e = ref(spec, mode)[i]
    o = oc.OracleCompressor(spec, D)
    o.testp = u
    return oc.shift_step(o, a, b, pnorm=pn, **kw)


@pytest.mark.parametrize("spec", SHIFT)
def test_shift_edges(ag, spec):
    """DIANA in place, EF21 in place and MARINA's base; operands aligned and 4 bytes past alignment."""
    errs = Errs()
    ab, gp = shift_inputs()
    with Ran("k_ew_shift", *(("k_norm_partials",) if dithering(spec) else ())) as ran:
        for mode in modes_of(spec):
            for i, (x, u, pn, e) in enumerate(ref(spec, mode)):
                a, b = ab[i]
                for off in (0, 1):
                    tag = f"{spec} {mode} {KINDS[i]} off{off}"
                    ta = gpu(a, off)
                    # DIANA: h = b updated in place, the message returned
                    tb = gpu(b, off)
                    pno = torch.empty(1, device="cuda")
                    msg, h = comp_for(ag, spec, mode, i, u).compressShift(ta, tb, alpha=ALPHA, shift=tb, shift_out=tb,
                                                                          pnorm_out=pno if dithering(spec) else None)
                    wm, wh = shift_want(spec, mode, i, a, b, alpha=ALPHA, h=b)
                    errs.same(msg, wm, tag + " diana msg")
                    errs.same(tb, wh, tag + " diana shift")
                    if dithering(spec):
                        errs.same(pno, [pn], tag + " pnorm_out")
                    # EF21: g_prev = b updated in place
                    tb = gpu(b, off)
                    comp_for(ag, spec, mode, i, u).compressShift(ta, tb, scale=SCALE, base=tb, out=tb)
                    wm, _ = shift_want(spec, mode, i, a, b, scale=SCALE, base=b)
                    errs.same(tb, wm, tag + " ef21")
                    # MARINA: a shared base, a new message
                    msg, _ = comp_for(ag, spec, mode, i, u).compressShift(ta, gpu(b, off), base=gpu(gp, off))
                    wm, _ = shift_want(spec, mode, i, a, b, base=gp)
                    errs.same(msg, wm, tag + " marina")
    ran.check()
    errs.done()


# ------------------------------------------------------------------------------------------------
# k_ew_shift_accum (+ scalar): ShiftUplinkReducer's general entry, shapes A, B and C of the header
# ------------------------------------------------------------------------------------------------
def shift_round_want(spec, mode, w, **kw):
    ab, gp = shift_inputs()
    msgs, hs = [], []
    for i in range(N):
        a, b = ab[i]
        kk = dict(kw)
        if kk.get("base") == "b":
            kk["base"] = b
        elif kk.get("base") == "gp":
            kk["base"] = gp
        if "alpha" in kk:
            kk["h"] = b
        m, h = shift_want(spec, mode, i, a, b, **kk)
        msgs.append(m)
        hs.append(h)
    return fold(msgs, w), msgs, hs


@pytest.mark.parametrize("spec", SHIFT)
def test_shift_uplink_edges(ag, spec):
    errs = Errs()
    ab, gp = shift_inputs()
    A, B = [p[0] for p in ab], [p[1] for p in ab]
    for mode in modes_of(spec):
        rs = ref(spec, mode)
        kw = pattern_kw(spec, mode, rs)
        red = ag.ShiftUplinkReducer(comp_for(ag, spec, "compat", 0, None), seed=SEED if mode == "device" else None)
        names = ("k_ew_shift_accum",) + (("k_norm_partials",) if dithering(spec) else ())
        for off in (0, 1):
            tag = f"{spec} {mode} off{off}"
            ta = matrix(A, off)
            with Ran(*names) as ran:
                # A: DIANA in place (no base, no msg, shift == shift_out == b)
                tb = matrix(B, off)
                pno = torch.empty(N, device="cuda")
                out, _, _ = red(ta, tb, alpha=ALPHA, shift=tb, shift_out=tb, weights=WEIGHTS,
                                pnorms_out=pno if dithering(spec) else None, **kw)
            if off == 0:
                ran.check()
            want, _, hs = shift_round_want(spec, mode, WEIGHTS, alpha=ALPHA)
            errs.same(out, want, tag + " A out")
            errs.same(tb, np.stack(hs), tag + " A shifts")
            if dithering(spec):
                errs.same(pno, [r[2] for r in rs], tag + " pnorms_out")
            # B: EF21 in place (base == msg == b)
            tb = matrix(B, off)
            out, _, _ = red(ta, tb, scale=SCALE, base=tb, msg_out=tb, **kw)
            want, msgs, _ = shift_round_want(spec, mode, None, scale=SCALE, base="b")
            errs.same(out, want, tag + " B out")
            errs.same(tb, np.stack(msgs), tag + " B rows")
            # C: MARINA (one shared base, nothing stored)
            out, _, _ = red(ta, matrix(B, off), base=gpu(gp, off), weights=WEIGHTS, **kw)
            want, _, _ = shift_round_want(spec, mode, WEIGHTS, base="gp")
            errs.same(out, want, tag + " C out")
    errs.done()


# ------------------------------------------------------------------------------------------------
# k_ew_code and the payload decoders: Q8, Q16, NAT16, F32
# ------------------------------------------------------------------------------------------------
WIRE = ["qsgd:8", "std.dithering:300:2", "natural", "ident"]


def collide(pn):
    """A subnormal norm: several levels give the same product level * norm."""
    return pn is not None and 0 < abs(float(pn)) < 2.0 ** -126


def header(pl):
    h = pl[:16].cpu().numpy()
    return h.view(np.uint32)


@pytest.mark.parametrize("spec", WIRE)
def test_wire_edges(ag, spec):
    """compressPayload == oracle.wire.pack bytes; decompressPayload and PayloadReducer == the oracle
    outputs and their fold.  hdr.bad == 0 on every row.  On the rows whose norm is subnormal several
    levels give the same product level * norm, and any code that decodes to the same bits is
    correct: there the decodes are compared, not the code bytes (header and padding still are)."""
    errs = Errs()
    for mode in modes_of(spec):
        rs = ref(spec, mode)
        o = oc.OracleCompressor(spec, D)
        pls = []
        for i, (x, u, pn, e) in enumerate(rs):
            tag = f"{spec} {mode} {KINDS[i]}"
            c = comp_for(ag, spec, mode, i, u)
            pl = c.compressPayload(gpu(x))
            want = wire.pack(o, e, pn)
            got = pl.cpu().numpy()
            errs.true(got.size == want.size, tag + " payload size")
            errs.true(header(pl)[3] == 0, tag + f" hdr.bad = {header(pl)[3]}")
            errs.true(np.array_equal(header(pl)[[0, 1, 3]], want[:16].view(np.uint32)[[0, 1, 3]]), tag + " header")
            errs.same(got[8:12].view(np.float32), want[8:12].view(np.float32), tag + " header norm")
            if not collide(pn):
                errs.true(np.array_equal(got[16:], want[16:]), tag + f" code bytes ({int(np.sum(got != want))} differ)")
            errs.same(c.decompressPayload(pl, D), e, tag + " decode")
            errs.same(wire.unpack(o, got, D), e, tag + " oracle decode of the kernel's bytes")
            pls.append(pl)
        red = ag.PayloadReducer(comp_for(ag, spec, "compat", 0, None))
        for w in (None, WEIGHTS):
            errs.same(red(pls, D, weights=w), fold([r[3] for r in rs], w), f"{spec} {mode} PayloadReducer w={w is not None}")
    errs.done()


# ------------------------------------------------------------------------------------------------
# k_ew_shift_code and k_unpack_shift_accum: the shifted round on the wire against the general round
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["qsgd:8", "natural"])
def test_shift_wire_edges(ag, spec):
    errs = Errs()
    ab, gp = shift_inputs()
    A, B = [p[0] for p in ab], [p[1] for p in ab]
    o = oc.OracleCompressor(spec, D)
    for mode in modes_of(spec):
        rs = ref(spec, mode)
        pls = []
        with Ran("k_ew_shift_code") as ran:
            for i, (x, u, pn, e) in enumerate(rs):
                tag = f"{spec} {mode} {KINDS[i]}"
                tb = gpu(B[i])
                pl, _, h = comp_for(ag, spec, mode, i, u).compressShiftPayload(gpu(A[i]), tb, alpha=ALPHA, shift=tb,
                                                                               shift_out=tb)
                _, wh = shift_want(spec, mode, i, A[i], B[i], alpha=ALPHA, h=B[i])
                errs.same(tb, wh, tag + " shift in place")
                errs.true(header(pl)[3] == 0, tag + f" hdr.bad = {header(pl)[3]}")
                errs.same(wire.unpack(o, pl.cpu().numpy(), D), e, tag + " oracle decode of the payload")
                if not collide(pn):                                               # (colliding products: decodes only)
                    errs.true(np.array_equal(pl.cpu().numpy()[16:], wire.pack(o, e, pn)[16:]), tag + " code bytes")
                pls.append(pl)
        ran.check()
        # the server: EF21's mirror in place and MARINA's shared base, against the general round
        kw = pattern_kw(spec, mode, rs)
        gen = ag.ShiftUplinkReducer(comp_for(ag, spec, "compat", 0, None), seed=SEED if mode == "device" else None)
        srv = ag.ShiftPayloadReducer(comp_for(ag, spec, "compat", 0, None))
        with Ran("k_unpack_shift_accum") as ran:
            mirror = matrix(B)
            got = srv(pls, D, scale=SCALE, base=mirror, msg_out=mirror, weights=WEIGHTS)
            got_c = srv(pls, D, base=gpu(gp))
        ran.check()
        tb = matrix(B)
        want, _, _ = gen(matrix(A), tb, scale=SCALE, base=tb, msg_out=tb, weights=WEIGHTS, **kw)
        errs.same(got, want.cpu().numpy(), f"{spec} {mode} server out")
        errs.same(mirror, tb.cpu().numpy(), f"{spec} {mode} server mirror rows")
        want_o, msgs, _ = shift_round_want(spec, mode, WEIGHTS, scale=SCALE, base="b")
        errs.same(got, want_o, f"{spec} {mode} server out vs oracle")
        errs.same(mirror, np.stack(msgs), f"{spec} {mode} server mirror rows vs oracle")
        want_c, _, _ = gen(matrix(A), matrix(B), base=gpu(gp), **kw)
        errs.same(got_c, want_c.cpu().numpy(), f"{spec} {mode} server shared base")
    errs.done()
