"""Host side of the sparse in-place RandK round (flc_randk_shift_reduce): the exported symbols and
every answer the entry gives before it needs a device — refusals are decided by pointer, leading
dimension and scale alone, so made-up device addresses are enough here (nothing is launched)."""
import ctypes
import re
import os

import pytest

from flpytorch_amd import _lib

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADER = os.path.join(ROOT, "include", "flcodec.h")
NAMES = ("flc_randk_shift_reduce_workspace_size", "flc_randk_shift_reduce")
A, B, BASE, OTHER, OUT, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000


def params(codec=None, k=10):
    prm = _lib.FlcCodecParams()
    prm.codec = _lib.FLC_RANDK if codec is None else codec
    prm.k = k
    prm.randk_scale = 2.0
    return prm


def pattern(compat):
    pat = _lib.FlcPattern()
    pat.d_randk_idx = 0x70000000 if compat else None
    return pat


def diana_rows(d):
    r = _lib.FlcShiftRows()
    r.d_a, r.lda, r.d_b, r.ldb = A, d, B, d
    r.d_shift_in, r.ldin, r.d_shift_out, r.ldout = B, d, B, d
    r.msg_scale, r.shift_alpha = 1.0, 0.5
    return r


def call(lib, prm, n, d, rows=None, pat=None, out=OUT, ws=WS, ws_bytes=1 << 40):
    return lib.flc_randk_shift_reduce(ctypes.byref(prm), ctypes.byref(pat) if pat is not None else None,
                                      ctypes.byref(rows) if rows is not None else None, n, d, None, ctypes.c_float(1.0),
                                      ctypes.c_void_p(out), ctypes.c_void_p(ws), ws_bytes, None)


def size(lib, prm, compat, n, d):
    return lib.flc_randk_shift_reduce_workspace_size(ctypes.byref(prm), ctypes.byref(pattern(compat)), n, d)


def test_symbols_exported_and_declared():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert name in declared
        assert hasattr(lib, name), name
    assert lib.flc_version() == 104                     # additive: the ABI version does not move
    assert lib.flc_randk_shift_reduce_workspace_size.restype is ctypes.c_size_t


def test_empty_calls_need_no_device():
    lib = _lib.load()
    prm = params()
    rows = _lib.FlcShiftRows()
    assert call(lib, prm, 0, 1000, rows) == _lib.FLC_OK
    assert call(lib, prm, 5, 0, rows) == _lib.FLC_OK
    assert call(lib, prm, 0, 0) == _lib.FLC_OK
    assert call(lib, prm, -1, 4, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 4, -1, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 65536, 8, rows) == _lib.FLC_ERR_ARG            # n > FLC_MAX_ROWS
    assert call(lib, prm, 2, 8, rows) == _lib.FLC_ERR_ARG                # null a / b
    assert call(lib, prm, 2, 8) == _lib.FLC_ERR_ARG                      # null rows
    assert call(lib, prm, 2, 100, diana_rows(100), out=None) == _lib.FLC_ERR_ARG
    assert call(lib, params(k=0), 2, 100, diana_rows(100)) == _lib.FLC_ERR_ARG      # K < 1
    assert call(lib, params(k=101), 2, 100, diana_rows(100)) == _lib.FLC_ERR_ARG    # K > d


@pytest.mark.parametrize("codec", [_lib.FLC_IDENT, _lib.FLC_LAZY, _lib.FLC_NATURAL, _lib.FLC_STD_DITHERING,
                                   _lib.FLC_NAT_DITHERING, _lib.FLC_TOPK, _lib.FLC_RANK_K, 99])
def test_other_codecs_are_unsupported(codec):
    lib = _lib.load()
    prm = params(codec)
    assert call(lib, prm, 2, 100, diana_rows(100)) == _lib.FLC_ERR_UNSUPPORTED
    assert len(lib.flc_last_error_string()) > 0
    assert size(lib, prm, False, 2, 100) == 0


def unsupported(rows, compat=False):
    lib = _lib.load()
    assert call(lib, params(), 2, 100, rows, pattern(compat)) == _lib.FLC_ERR_UNSUPPORTED
    msg = lib.flc_last_error_string()
    assert len(msg) > 0
    return msg


@pytest.mark.parametrize("compat", [False, True])
def test_shapes_outside_a_to_d_are_unsupported(compat):
    d = 100
    r = diana_rows(d)
    r.d_shift_out = OTHER                                # shift_out rows that are not the b rows
    unsupported(r, compat)
    r = diana_rows(d)
    r.ldout = d + 4                                      # ... or with another leading dimension
    unsupported(r, compat)
    r = diana_rows(d)
    r.d_shift_in = OTHER
    unsupported(r, compat)
    r = _lib.FlcShiftRows()                              # a per-row base that is not d_msg == d_b
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale = A, d, B, d, 1.0
    r.d_base, r.ldbase = BASE, d
    unsupported(r, compat)
    r.d_msg, r.ldmsg = BASE, d
    unsupported(r, compat)
    r.d_base, r.d_msg = B, OTHER                         # a dense message matrix
    unsupported(r, compat)
    r = _lib.FlcShiftRows()                              # a stored message without a base
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale = A, d, B, d, 1.0
    r.d_msg, r.ldmsg = B, d
    unsupported(r, compat)


def test_scales_must_be_finite_and_positive():
    d = 100
    for bad in (-1.0, 0.0, float("inf"), float("nan")):
        r = diana_rows(d)
        r.msg_scale = bad
        assert b"msg_scale" in unsupported(r)
        r = diana_rows(d)
        r.shift_alpha = bad
        assert b"shift_alpha" in unsupported(r)
    r = _lib.FlcShiftRows()                              # without a shift, shift_alpha is not looked at
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale, r.shift_alpha = A, d, B, d, 1.0, 0.0
    lib = _lib.load()
    assert call(lib, params(), 2, d, r, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE     # accepted (shape D) up to the workspace


@pytest.mark.parametrize("compat", [False, True])
def test_workspace_one_byte_short(compat):
    lib = _lib.load()
    n, d = 5, 100003
    prm = params(k=3000)
    need = size(lib, prm, compat, n, d)
    assert need > 0
    assert call(lib, prm, n, d, diana_rows(d), pattern(compat), ws_bytes=need - 1) == _lib.FLC_ERR_WORKSPACE
    assert b"workspace" in lib.flc_last_error_string()


def test_workspace_holds_no_dense_row():
    lib = _lib.load()
    n, d = 5, 1000000
    prm = params(k=10000)
    for compat in (False, True):
        assert 0 < size(lib, prm, compat, n, d) < 4 * d
    assert lib.flc_randk_shift_reduce_workspace_size(ctypes.byref(prm), None, n, d) == size(lib, prm, False, n, d)
    # against the general entry, which keeps a message row, a difference row and an encoded row
    assert lib.flc_encode_shift_reduce_workspace_size(ctypes.byref(prm), n, d) > 12 * d


def test_general_entry_sizes_are_what_they_were():
    """The shapes tests/test_shift_uplink_host.py pins, and the RandK size in bytes."""
    lib = _lib.load()
    gsize = lib.flc_encode_shift_reduce_workspace_size
    n, d = 5, 100003
    assert gsize(ctypes.byref(params(_lib.FLC_IDENT)), n, d) == 0
    assert gsize(ctypes.byref(params(_lib.FLC_NATURAL)), n, d) > 0
    prm = params(_lib.FLC_TOPK, k=2001)
    one = lib.flc_encode_shift_workspace_size(ctypes.byref(prm), d)
    assert gsize(ctypes.byref(prm), n, d) == gsize(ctypes.byref(prm), 1, d)
    assert one + 4 * d <= gsize(ctypes.byref(prm), n, d) <= one + 4 * d + 512
    assert lib.flc_encode_shift_workspace_size(ctypes.byref(params(_lib.FLC_IDENT)), d) == 0
    prm = params(k=3000)
    one = lib.flc_encode_shift_workspace_size(ctypes.byref(prm), d)
    assert gsize(ctypes.byref(prm), n, d) == gsize(ctypes.byref(prm), 1, d)
    assert one + 4 * d <= gsize(ctypes.byref(prm), n, d) <= one + 4 * d + 512
    assert 8 * d <= one <= 8 * d + 1024 + 4 * 25 + 8         # two rows + one row's chunk counts and key
