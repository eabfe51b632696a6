"""The fused uplink in the reference's norm bits: UplinkReducer with Compressor.norm_mode =
"torch_cpu" (flc_encode_reduce_ex, FLC_NORMMODE_TORCH_CPU) and with the caller's norms (pnorms_in).

Bar: BIT-EXACT (uint32 compare).  The expectation for row i is the oracle's encode with
pnorm = orc_torch_norm2(row_i) — oracle/torch_norm.c, torch.norm(x, p=2) on a CPU fp32 tensor in
torch's reduction order (compressors.py:272 / 303), itself pinned against the reference's recorded
norms — with the device draws of oracle/devrng.py or the caller's float64 uniforms, folded by
oracle.codecs.reduce_plain.  Where a case takes pnorms_out it must be orc_torch_norm2 bit for bit.
The last two tests run the reference's own 25 M-element rows (tests/golden/rows.{json,npz}).
"""
import ctypes
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import codecs as oc
from oracle import devrng
from tests.test_gpu_dither_sparse import compat_uniforms, make_rows

pytestmark = pytest.mark.gpu

SEED = 20240607
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def assert_bitexact(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    g, w = bits(got), bits(want)
    # NaN results must sit at the same positions; their payload / sign bit is not compared
    # (numpy on x86 and the GPU propagate different NaN encodings)
    same = (g == w) | (np.isnan(np.asarray(got, np.float32)).ravel() & np.isnan(np.asarray(want, np.float32)).ravel())
    if not same.all():
        bad = np.nonzero(~same)[0]
        raise AssertionError(f"{bad.size} of {g.size} elements differ; first {bad[:5]}: "
                             f"{np.asarray(got).ravel()[bad[:5]]} vs {np.asarray(want).ravel()[bad[:5]]}")


_TN = []


def torch_norm2(x):
    """oracle/torch_norm.c: the fp32 2-norm in torch's CPU reduction order."""
    if not _TN:
        from oracle import rng  # (builds oracle/_build on first use)
        lib = ctypes.CDLL(rng._LIB_PATH)
        lib.orc_torch_norm2.restype = ctypes.c_float
        lib.orc_torch_norm2.argtypes = [ctypes.c_void_p, ctypes.c_int64]
        _TN.append(lib)
    x = np.ascontiguousarray(x, dtype=np.float32)
    return np.float32(_TN[0].orc_torch_norm2(x.ctypes.data, x.size))


def torch_norms(rows):
    return np.array([torch_norm2(rows[i]) for i in range(rows.shape[0])], dtype=np.float32)


def oracle_uplink(spec, rows, client0, weights=None, uniforms=None, pnorms=None):
    """reduce_plain of the oracle's encodes with the given norms (default: torch's order)."""
    d = rows.shape[1]
    pnorms = torch_norms(rows) if pnorms is None else pnorms
    enc = []
    for i in range(rows.shape[0]):
        o = oc.OracleCompressor(spec, d)
        o.testp = devrng.uniforms(SEED, client0 + i, d) if uniforms is None else uniforms[i]
        enc.append(o.compress(rows[i], pnorm=pnorms[i]))
    return oc.reduce_plain(enc, weights), pnorms


def compressor(ag, spec, d, path="sparse", mode="torch_cpu", groups=None):
    c = ag.initCompressor(spec, d)
    c.dither_path = path
    c.norm_mode = mode
    if groups:
        c.row_groups = groups
    return c


# 1. row kinds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "heavy", "sparse", "negative", "clustered", "ones", "tiny"])
@pytest.mark.parametrize("spec", ["qsgd:4", "qsgd:127"])
def test_row_kinds(ag, kind, spec):
    """A lane has 37 500 steps at this d and crosses several binades; the heavy and sparse kinds
    make the float64 prediction wrong, so the walk's exact pass runs."""
    n, d, client0 = 5, 300_001, 11
    rows = make_rows(kind, n, d, np.random.default_rng(zlib.crc32(f"tn{kind}{spec}".encode())))
    want, wn = oracle_uplink(spec, rows, client0)
    red = ag.UplinkReducer(compressor(ag, spec, d), seed=SEED)
    pn = torch.empty(n, device="cuda")
    got = red(torch.from_numpy(rows).cuda(), client0=client0, pnorms_out=pn)
    assert_bitexact(pn, wn)
    assert_bitexact(got, want)


# 2. shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 7, 8, 9, 4096, 4097, 8191, 8192, 8193, 24_581, 32_768, 32_769, 65_536, 65_537,
                               100_003])
def test_shapes(ag, d):
    """D % 8 tails, item (8192) and part (32 768) boundaries, a last part with fewer than 4 items,
    the whole-row sample (d <= 65 536); the matrix and the pointer-array entry."""
    n, client0 = 3, 0
    rows = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    want, wn = oracle_uplink("qsgd:16", rows, client0)
    red = ag.UplinkReducer(compressor(ag, "qsgd:16", d), seed=SEED)
    rt = torch.from_numpy(rows).cuda()
    pn = torch.empty(n, device="cuda")
    assert_bitexact(red(rt, client0=client0, pnorms_out=pn), want)
    assert_bitexact(pn, wn)
    pn.zero_()
    assert_bitexact(red([rt[i].clone() for i in range(n)], client0=client0, pnorms_out=pn), want)
    assert_bitexact(pn, wn)


# 3. non-finite values and weights ----------------------------------------------------------------
def test_nonfinite_and_weights(ag):
    n, d, client0 = 6, 120_000, 5
    g = np.random.default_rng(3)
    rows = make_rows("negative", n, d, g)
    rows[1] = g.standard_normal(d).astype(np.float32)
    rows[0, 777] = np.nan
    rows[2, 31] = np.inf
    rows[4, ::3] = 3e19                      # the squares overflow fp32: torch's norm is inf
    rows[5] = 0.0
    w = [0.5, -2.0, 1.0, 0.0, 3.0, 1.25]
    want, wn = oracle_uplink("qsgd:8", rows, client0, weights=w)
    assert np.isnan(wn[0]) and np.isinf(wn[2]) and np.isinf(wn[4]) and wn[5] == 0
    red = ag.UplinkReducer(compressor(ag, "qsgd:8", d), seed=SEED)
    pn = torch.empty(n, device="cuda")
    got = red(torch.from_numpy(rows).cuda(), client0=client0, weights=w, pnorms_out=pn)
    assert_bitexact(pn, wn)
    assert_bitexact(got, want)


# 4. row groups -----------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", [2, 3])
def test_row_groups(ag, groups):
    n, d, client0 = 7, 150_001, 3
    g = np.random.default_rng(groups)
    rows = make_rows("normal", n, d, g)
    rows[2] = make_rows("negative", 1, d, g)[0]
    rows[5] = make_rows("clustered", 1, d, g)[0]          # a dense-folded row inside a group
    w = [1.0, -0.5, 2.0, 1.5, 0.25, 1.0, 3.0]
    want, wn = oracle_uplink("qsgd:16", rows, client0, weights=w)
    red = ag.UplinkReducer(compressor(ag, "qsgd:16", d, groups=groups), seed=SEED)
    pn = torch.empty(n, device="cuda")
    got = red(torch.from_numpy(rows).cuda(), client0=client0, weights=w, pnorms_out=pn)
    torch.cuda.synchronize()
    assert_bitexact(pn, wn)
    assert_bitexact(got, want)


def test_default_row_groups(ag):
    """161 rows take the default two row groups: group 0's maps, walk, final, resolve and fold on
    the side stream under group 1's filter.  Once through the pointer entry."""
    n, d, client0 = 161, 40_003, 11
    g = np.random.default_rng(161)
    rows = make_rows("normal", n, d, g)
    for i, kind in ((0, "negative"), (79, "clustered"), (80, "clustered"), (81, "sparse"), (120, "heavy"), (160, "ones")):
        rows[i] = make_rows(kind, 1, d, g)[0]
    want, wn = oracle_uplink("qsgd:16", rows, client0)
    red = ag.UplinkReducer(compressor(ag, "qsgd:16", d), seed=SEED)
    x = torch.from_numpy(rows).cuda()
    pn = torch.empty(n, device="cuda")
    got = red(x, client0=client0, pnorms_out=pn)
    torch.cuda.synchronize()
    assert_bitexact(pn, wn)
    assert_bitexact(got, want)
    from flpytorch_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_collect("k_ds_filter")
    again = red([x[i] for i in range(n)], client0=client0)
    torch.cuda.synchronize()
    launches = _lib.profile_collect("k_ds_filter")[1]
    _lib.profile_enable(False)
    assert launches == 2
    assert_bitexact(again, want)


# 5. compat uniforms on the sparse path -----------------------------------------------------------
def test_compat_uniforms_sparse(ag):
    n, d, client0 = 4, 150_001, 0
    g = np.random.default_rng(55)
    rows = make_rows("normal", n, d, g)
    rows[3] = make_rows("heavy", 1, d, g)[0]
    uni = compat_uniforms(n, d, g)
    want, wn = oracle_uplink("qsgd:127", rows, client0, uniforms=uni)
    red = ag.UplinkReducer(compressor(ag, "qsgd:127", d))
    pad = torch.zeros((n, d + 3), dtype=torch.float64, device="cuda")   # uniforms_ld = d + 3
    pad[:, :d] = torch.from_numpy(uni)
    pn = torch.empty(n, device="cuda")
    got = red(torch.from_numpy(rows).cuda(), pnorms_out=pn, uniforms=pad[:, :d])
    assert_bitexact(pn, wn)
    assert_bitexact(got, want)


# 6. the dense path and the other codecs ----------------------------------------------------------
@pytest.mark.parametrize("spec", ["qsgd:16", "nat.dithering:8:2", "std.dithering:16:2"])
@pytest.mark.parametrize("entry", ["matrix", "pointers"])
def test_dense_path(ag, spec, entry):
    n, d, client0 = 4, 200_003, 2
    g = np.random.default_rng(zlib.crc32(spec.encode()))
    rows = make_rows("normal", n, d, g)
    rows[1] = make_rows("heavy", 1, d, g)[0]
    want, wn = oracle_uplink(spec, rows, client0)
    red = ag.UplinkReducer(compressor(ag, spec, d, path="dense"), seed=SEED)
    x = torch.from_numpy(rows).cuda()
    pn = torch.empty(n, device="cuda")
    got = red(x if entry == "matrix" else [x[i] for i in range(n)], client0=client0, pnorms_out=pn)
    assert_bitexact(pn, wn)
    assert_bitexact(got, want)


def test_p_inf_is_exact_and_p1_refused(ag):
    n, d = 3, 50_001
    rows = np.random.default_rng(9).standard_normal((n, d)).astype(np.float32)
    x = torch.from_numpy(rows).cuda()
    outs = []
    for mode in ("exact", "torch_cpu"):
        red = ag.UplinkReducer(compressor(ag, "std.dithering:16:inf", d, path=None, mode=mode), seed=SEED)
        pn = torch.empty(n, device="cuda")
        outs.append((red(x, pnorms_out=pn).cpu().numpy(), pn.cpu().numpy()))
    assert_bitexact(outs[1][0], outs[0][0])
    assert_bitexact(outs[1][1], outs[0][1])
    red = ag.UplinkReducer(compressor(ag, "nat.dithering:4:1", d, path=None), seed=SEED)
    with pytest.raises(NotImplementedError):
        red(x)


# 7. pnorms_in ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["sparse", "dense"])
def test_pnorms_in(ag, path):
    n, d, client0 = 5, 150_001, 7
    g = np.random.default_rng(71)
    rows = make_rows("normal", n, d, g)
    rows[3] = make_rows("negative", 1, d, g)[0]
    x = torch.from_numpy(rows).cuda()
    # the pnorms_out of an exact-mode run reproduce that run
    red = ag.UplinkReducer(compressor(ag, "qsgd:16", d, path=path, mode="exact"), seed=SEED)
    pn = torch.empty(n, device="cuda")
    own = red(x, client0=client0, pnorms_out=pn).cpu().numpy()
    pn2 = torch.empty(n, device="cuda")
    assert_bitexact(red(x, client0=client0, pnorms_in=pn, pnorms_out=pn2), own)
    assert_bitexact(pn2, pn.cpu().numpy())
    # the oracle's torch-order norms reproduce mode 1
    want, wn = oracle_uplink("qsgd:16", rows, client0)
    assert_bitexact(red(x, client0=client0, pnorms_in=torch.from_numpy(wn).cuda()), want)
    red1 = ag.UplinkReducer(compressor(ag, "qsgd:16", d, path=path), seed=SEED)
    assert_bitexact(red1(x, client0=client0), want)
    # a norm outside the sampled bounds: the row folds dense, with that norm
    far = wn.copy()
    far[1] = np.float32(far[1] * np.float32(1.5))
    want_far, _ = oracle_uplink("qsgd:16", rows, client0, pnorms=far)
    assert_bitexact(red(x, client0=client0, pnorms_in=torch.from_numpy(far).cuda(), pnorms_out=pn2), want_far)
    assert_bitexact(pn2, far)


@pytest.mark.parametrize("path", ["sparse", "dense"])
def test_ex_abi_errors(ag, path):
    from flpytorch_amd import _lib
    lib = _lib.load()
    n, d = 4, 100_003
    comp = compressor(ag, "qsgd:16", d, path=path)
    prm, keep = comp.codec_params(torch.device("cuda", torch.cuda.current_device()))
    prm.seed = SEED
    pat = _lib.FlcPattern()
    x = torch.randn(n, d, device="cuda")
    out = torch.full((d,), 7.0, device="cuda")
    pin = torch.ones(n, device="cuda")
    plain = lib.flc_encode_reduce_workspace_size(ctypes.byref(prm), n, d)
    assert plain == lib.flc_encode_reduce_ex_workspace_size(ctypes.byref(prm), n, d, 0, _lib.FLC_NORMMODE_EXACT)
    ex = lib.flc_encode_reduce_ex_workspace_size(ctypes.byref(prm), n, d, 0, _lib.FLC_NORMMODE_TORCH_CPU)
    assert ex > plain
    ws = torch.empty(ex, dtype=torch.uint8, device="cuda")

    def call(pin_ptr, mode, nbytes):
        return lib.flc_encode_reduce_ex(ctypes.byref(prm), ctypes.byref(pat), ctypes.c_void_p(x.data_ptr()), d, None, n, d,
                                        None, ctypes.c_float(n), ctypes.c_void_p(pin_ptr), mode, None,
                                        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                        _lib.stream_ptr())
    assert call(pin.data_ptr(), _lib.FLC_NORMMODE_TORCH_CPU, ex) == _lib.FLC_ERR_ARG
    assert call(None, 2, ex) == _lib.FLC_ERR_ARG
    assert call(None, _lib.FLC_NORMMODE_TORCH_CPU, plain) == _lib.FLC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call launched something"
    prm.norm = _lib.FLC_NORM_L1
    assert call(None, _lib.FLC_NORMMODE_TORCH_CPU, ex) == _lib.FLC_ERR_UNSUPPORTED
    prm.norm = _lib.FLC_NORM_L2
    assert call(None, _lib.FLC_NORMMODE_TORCH_CPU, ex) == _lib.FLC_OK
    torch.cuda.synchronize()
    assert not bool((out == 7.0).all())


# 8. the reference's own rows ---------------------------------------------------------------------
META = {m["name"]: m for m in json.load(open(os.path.join(HERE, "golden", "rows.json")))}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


@pytest.fixture(scope="module")
def c4(ag):
    """The two recorded C4 rows (D = 25 M) regenerated from their seeds as test_gpu_rows_ref.py does,
    with the reference's numpy-stream uniforms, on the device."""
    from tests.test_gpu_rows_ref import row
    got = {}
    for name in ("qsgd_c4", "qsgd_c4_heavy"):
        m = META[name]
        x = row(m["seed"], m["D"], m["dist"])
        assert sha(x) == m["x_sha"], "row regeneration differs from the fixture's"
        c = ag.initCompressor(m["spec"], m["D"])
        c.generateCompressPattern(np.random.RandomState(m["pattern_seed"]), "cuda", 0, None)
        assert sha(c.testp.numpy()) == m["testp_sha"], "numpy-stream uniforms differ from the reference's"
        got[name] = (torch.from_numpy(x).cuda(), c.testp.cuda(), m)
    return got


@pytest.mark.parametrize("name", ["qsgd_c4", "qsgd_c4_heavy"])
def test_reference_row(ag, c4, name):
    """One row, divisor 1: the reference's recorded output digest and norm bits."""
    x, u, m = c4[name]
    c = ag.initCompressor(m["spec"], m["D"])
    c.norm_mode = "torch_cpu"
    pn = torch.empty(1, device="cuda")
    out = ag.UplinkReducer(c)(x.view(1, -1), uniforms=u.view(1, -1), divisor=1.0, pnorms_out=pn).cpu().numpy()
    assert int(pn.cpu().numpy().view(np.uint32)[0]) == m["pnorm_bits"]
    assert sha(out) == m["out_sha"]


def test_reference_rows_fused(ag, c4):
    """Both rows and the first again through the sparse single pass, each with its own uniforms:
    reduce_plain of the three compressVector(norm_mode="torch_cpu") outputs, which
    test_gpu_rows_ref.py pins to the reference."""
    names = ["qsgd_c4", "qsgd_c4_heavy", "qsgd_c4"]
    m = c4[names[0]][2]
    enc = {}
    for name in set(names):
        x, u, _ = c4[name]
        c = ag.initCompressor(m["spec"], m["D"])
        c.norm_mode = "torch_cpu"
        c.testp = u
        enc[name] = c.compressVector(x).cpu().numpy()
    want = oc.reduce_plain([enc[k] for k in names])
    c = ag.initCompressor(m["spec"], m["D"])
    c.norm_mode = "torch_cpu"
    rows = [c4[k][0] for k in names]
    uni = torch.stack([c4[k][1] for k in names])
    pn = torch.empty(3, device="cuda")
    got = ag.UplinkReducer(c)(rows, uniforms=uni, pnorms_out=pn)
    assert [int(v) for v in pn.cpu().numpy().view(np.uint32)] == [c4[k][2]["pnorm_bits"] for k in names]
    assert_bitexact(got, want)
