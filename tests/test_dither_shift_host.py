"""Host side of the one-read QSGD shifted round (flc_dither_shift_reduce): the exported symbols and
every answer the entry gives before it needs a device — refusals are decided by codec, norm, path
hint, (s, d), pointer, leading dimension and scale alone, so made-up device addresses are enough
here (nothing is launched)."""
import ctypes
import os
import re

import pytest

from flpytorch_amd import _lib

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADER = os.path.join(ROOT, "include", "flcodec.h")
NAMES = ("flc_dither_shift_reduce_workspace_size", "flc_dither_shift_reduce", "flc_dither_row_flags")
A, B, BASE, OTHER, OUT, WS, LEV, U = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000,
                                     0x78000000)
D = 100_003          # qsgd:4 stays on the sparse path in auto mode from about d = 12 000 on


def params(codec=None, s=4, norm=None, path=_lib.FLC_PATH_AUTO):
    prm = _lib.FlcCodecParams()
    prm.codec = _lib.FLC_STD_DITHERING if codec is None else codec
    prm.s = s
    prm.norm = _lib.FLC_NORM_L2 if norm is None else norm
    prm.flags = path
    prm.k = 10
    prm.d_levels = LEV
    prm.seed = 7
    return prm


def diana_rows(d):
    r = _lib.FlcShiftRows()
    r.d_a, r.lda, r.d_b, r.ldb = A, d, B, d
    r.d_shift_in, r.ldin, r.d_shift_out, r.ldout = B, d, B, d
    r.msg_scale, r.shift_alpha = 1.0, 0.5
    return r


def ef21_rows(d):
    r = _lib.FlcShiftRows()
    r.d_a, r.lda, r.d_b, r.ldb = A, d, B, d
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = B, d, B, d
    r.msg_scale = 0.25
    return r


def fold_rows(d):
    r = _lib.FlcShiftRows()
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale = A, d, B, d, 1.0
    return r


def call(lib, prm, n, d, rows=None, out=OUT, ws=WS, ws_bytes=1 << 40, pat=None):
    return lib.flc_dither_shift_reduce(ctypes.byref(prm), ctypes.byref(pat) if pat is not None else None,
                                       ctypes.byref(rows) if rows is not None else None, n, d, None, ctypes.c_float(1.0),
                                       None, ctypes.c_void_p(out), ctypes.c_void_p(ws), ws_bytes, None)


def size(lib, prm, n, d):
    return lib.flc_dither_shift_reduce_workspace_size(ctypes.byref(prm), n, d)


def unsupported(rows, prm=None, n=2, d=D, pat=None):
    lib = _lib.load()
    assert call(lib, prm or params(), n, d, rows, pat=pat) == _lib.FLC_ERR_UNSUPPORTED
    msg = lib.flc_last_error_string()
    assert len(msg) > 0
    return msg


def accepted(rows, prm=None, n=2, d=D):
    """Taken up to the workspace check, the last one before the first launch."""
    assert call(_lib.load(), prm or params(), n, d, rows, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE


def test_symbols_exported_and_declared():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert name in declared
        assert hasattr(lib, name), name
    assert lib.flc_version() == 104                     # additive: the ABI version does not move
    assert lib.flc_dither_shift_reduce_workspace_size.restype is ctypes.c_size_t


def test_empty_calls_need_no_device():
    lib = _lib.load()
    prm = params()
    rows = _lib.FlcShiftRows()
    assert call(lib, prm, 0, 1000, rows) == _lib.FLC_OK
    assert call(lib, prm, 5, 0, rows) == _lib.FLC_OK
    assert call(lib, prm, 0, 0) == _lib.FLC_OK
    assert size(lib, prm, 0, 1000) == 0 and size(lib, prm, 5, 0) == 0
    assert lib.flc_dither_row_flags(0, 100, None, 0, None, None) == _lib.FLC_OK
    assert lib.flc_dither_row_flags(3, 100, None, 0, None, None) == _lib.FLC_ERR_ARG


def test_argument_errors():
    lib = _lib.load()
    prm = params()
    rows = _lib.FlcShiftRows()
    assert call(lib, prm, -1, 4, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 4, -1, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 65536, 8, rows) == _lib.FLC_ERR_ARG            # n > FLC_MAX_ROWS
    assert call(lib, prm, 2, 8, rows) == _lib.FLC_ERR_ARG                # null a / b
    assert call(lib, prm, 2, 8) == _lib.FLC_ERR_ARG                      # null rows
    for field in ("d_a", "d_b"):
        r = diana_rows(D)
        setattr(r, field, None)
        assert call(lib, prm, 2, D, r) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 2, D, diana_rows(D), out=None) == _lib.FLC_ERR_ARG
    r = diana_rows(D)
    r.d_shift_in = None
    assert call(lib, prm, 2, D, r) == _lib.FLC_ERR_ARG                 # shift_out without shift_in
    big = 0x7FFFFFFF                                                     # 32-bit offsets of the sparse pipeline
    assert call(lib, params(path=_lib.FLC_PATH_SPARSE), 1, big, diana_rows(big)) == _lib.FLC_ERR_ARG
    for rows in (diana_rows(D), ef21_rows(D)):                       # in-place rows that overlap
        rows.ldb = D - 1
        if rows.d_shift_out:
            rows.ldin = rows.ldout = D - 1
        else:
            rows.ldbase = rows.ldmsg = D - 1
        assert call(lib, params(), 2, D, rows) == _lib.FLC_ERR_ARG
        assert b"overlap" in lib.flc_last_error_string()
        assert call(lib, params(), 1, D, rows, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE   # one row cannot overlap


@pytest.mark.parametrize("codec", [_lib.FLC_IDENT, _lib.FLC_LAZY, _lib.FLC_RANDK, _lib.FLC_NATURAL, _lib.FLC_NAT_DITHERING,
                                   _lib.FLC_TOPK, _lib.FLC_RANK_K, 99])
def test_other_codecs_are_unsupported(codec):
    lib = _lib.load()
    prm = params(codec)
    assert b"FLC_STD_DITHERING" in unsupported(diana_rows(D), prm)
    assert size(lib, prm, 2, D) == 0


@pytest.mark.parametrize("norm", [_lib.FLC_NORM_LINF, _lib.FLC_NORM_L1])
def test_other_norms_are_unsupported(norm):
    prm = params(norm=norm)
    assert b"FLC_NORM_L2" in unsupported(diana_rows(D), prm)
    assert size(_lib.load(), prm, 2, D) == 0


def test_compat_uniforms_are_unsupported():
    pat = _lib.FlcPattern()
    pat.d_uniforms, pat.uniforms_ld = U, D
    assert b"compat" in unsupported(diana_rows(D), pat=pat)
    pat.d_uniforms = None                                                # a pattern with only client0 is taken
    pat.client0 = 11
    assert call(_lib.load(), params(), 2, D, diana_rows(D), ws_bytes=0, pat=pat) == _lib.FLC_ERR_WORKSPACE


def test_the_sparse_path_must_be_eligible():
    d = 300_001
    assert b"FLC_PATH_DENSE" in unsupported(diana_rows(d), params(path=_lib.FLC_PATH_DENSE), d=d)
    assert b"staging" in unsupported(diana_rows(d), params(s=127), d=d)          # auto mode, qsgd:127: share too high
    accepted(diana_rows(d), params(s=127, path=_lib.FLC_PATH_SPARSE), d=d)       # forced as it is today
    accepted(diana_rows(d), params(s=4), d=d)
    prm = params()
    prm.d_levels = None
    unsupported(diana_rows(D), prm)


def test_shapes():
    d = D
    for ok in (diana_rows(d), ef21_rows(d), fold_rows(d)):                # A, B, D
        accepted(ok)
    r = fold_rows(d)                                                      # C: one shared base
    r.d_base, r.ldbase = BASE, 0
    assert b"MARINA" in unsupported(r)
    r = diana_rows(d)
    r.d_shift_out = OTHER                                                 # a shift not in place
    assert b"shift" in unsupported(r)
    r = diana_rows(d)
    r.ldout = d + 4
    assert b"shift" in unsupported(r)
    r = diana_rows(d)
    r.d_shift_in = OTHER
    assert b"shift" in unsupported(r)
    r = diana_rows(d)                                                     # a shift together with a base
    r.d_base, r.ldbase = BASE, 0
    assert b"shift" in unsupported(r)
    r = fold_rows(d)                                                      # a per-row base that is not d_msg == d_b
    r.d_base, r.ldbase = BASE, d
    assert b"base" in unsupported(r)
    r = ef21_rows(d)
    r.d_msg = OTHER                                                       # a dense message matrix
    assert b"d_msg" in unsupported(r)
    r = fold_rows(d)                                                      # a stored message without a base
    r.d_msg, r.ldmsg = B, d
    assert b"d_msg" in unsupported(r)


def test_scales():
    d = D
    for rows in (diana_rows(d), fold_rows(d)):                            # A and D fold the messages: scale 1 only
        rows.msg_scale = 0.5
        assert b"msg_scale" in unsupported(rows)
    for bad in (-1.0, 0.0, float("inf"), float("nan")):
        for rows in (diana_rows(d), ef21_rows(d), fold_rows(d)):
            rows.msg_scale = bad
            assert b"msg_scale" in unsupported(rows)
        r = diana_rows(d)
        r.shift_alpha = bad
        assert b"shift_alpha" in unsupported(r)
    r = ef21_rows(d)                                                      # B takes any finite scale > 0
    r.msg_scale = 3.5
    accepted(r)
    r = fold_rows(d)                                                      # without a shift, shift_alpha is not looked at
    r.shift_alpha = 0.0
    accepted(r)


def test_workspace():
    lib = _lib.load()
    n, d = 5, 100_003
    prm = params()
    need = size(lib, prm, n, d)
    assert need > 0
    assert call(lib, prm, n, d, diana_rows(d), ws_bytes=need - 1) == _lib.FLC_ERR_WORKSPACE
    assert b"workspace" in lib.flc_last_error_string()
    # the sparse pipeline's state and nothing else: no [n][d] matrix, no [d] message row
    sparse = params(path=_lib.FLC_PATH_SPARSE)
    ds = lib.flc_encode_reduce_workspace_size(ctypes.byref(sparse), n, d)
    assert 0 < need <= ds + 1024
    assert lib.flc_dither_row_flags(n, d, ctypes.c_void_p(WS), need - 1, ctypes.c_void_p(OUT), None) == _lib.FLC_ERR_WORKSPACE


def test_sibling_entries_are_what_they_were():
    lib = _lib.load()
    n, d = 5, 100_003
    prm = params()
    # the general entry sizes the dense two-pass form; the RandK and TopK entries keep refusing QSGD
    assert lib.flc_encode_shift_reduce_workspace_size(ctypes.byref(prm), n, d) < size(lib, prm, n, d)
    rc = lib.flc_randk_shift_reduce(ctypes.byref(prm), None, ctypes.byref(diana_rows(d)), n, d, None, ctypes.c_float(1.0),
                                    ctypes.c_void_p(OUT), ctypes.c_void_p(WS), 1 << 40, None)
    assert rc == _lib.FLC_ERR_UNSUPPORTED
    rc = lib.flc_topk_shift_reduce(ctypes.byref(prm), ctypes.byref(diana_rows(d)), n, d, None, ctypes.c_float(1.0),
                                   ctypes.c_void_p(OUT), ctypes.c_void_p(WS), 1 << 40, None)
    assert rc == _lib.FLC_ERR_UNSUPPORTED
