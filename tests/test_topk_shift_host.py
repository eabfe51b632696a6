"""Host side of the batched TopK shifted round (flc_topk_shift_reduce): the exported symbols and every
answer the entry gives before it needs a device — refusals are decided by codec, pointer, leading
dimension, K, tie rule and scale alone, so made-up device addresses are enough here (nothing is
launched)."""
import ctypes
import re
import os

import pytest

from flpytorch_amd import _lib

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADER = os.path.join(ROOT, "include", "flcodec.h")
NAMES = ("flc_topk_shift_reduce_workspace_size", "flc_topk_shift_reduce")
A, B, BASE, OTHER, OUT, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000


def params(codec=None, k=10, tie=0):
    prm = _lib.FlcCodecParams()
    prm.codec = _lib.FLC_TOPK if codec is None else codec
    prm.k = k
    prm.randk_scale = 2.0
    prm.tie = tie
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
    r.msg_scale = 1.0
    return r


def call(lib, prm, n, d, rows=None, out=OUT, ws=WS, ws_bytes=1 << 40):
    return lib.flc_topk_shift_reduce(ctypes.byref(prm), ctypes.byref(rows) if rows is not None else None, n, d, None,
                                     ctypes.c_float(1.0), ctypes.c_void_p(out), ctypes.c_void_p(ws), ws_bytes, None)


def size(lib, prm, n, d):
    return lib.flc_topk_shift_reduce_workspace_size(ctypes.byref(prm), n, d)


def test_symbols_exported_and_declared():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert name in declared
        assert hasattr(lib, name), name
    assert lib.flc_version() == 104                     # additive: the ABI version does not move
    assert lib.flc_topk_shift_reduce_workspace_size.restype is ctypes.c_size_t


def test_empty_calls_need_no_device():
    lib = _lib.load()
    prm = params()
    rows = _lib.FlcShiftRows()
    assert call(lib, prm, 0, 1000, rows) == _lib.FLC_OK
    assert call(lib, prm, 5, 0, rows) == _lib.FLC_OK
    assert call(lib, prm, 0, 0) == _lib.FLC_OK
    assert size(lib, prm, 0, 1000) == 0 and size(lib, prm, 5, 0) == 0


def test_argument_errors():
    lib = _lib.load()
    prm = params()
    rows = _lib.FlcShiftRows()
    assert call(lib, prm, -1, 4, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 4, -1, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 65536, 8, rows) == _lib.FLC_ERR_ARG            # n > FLC_MAX_ROWS
    assert call(lib, prm, 2, 8, rows) == _lib.FLC_ERR_ARG                # null a / b
    assert call(lib, prm, 2, 8) == _lib.FLC_ERR_ARG                      # null rows
    r = diana_rows(100)
    r.d_a = None
    assert call(lib, prm, 2, 100, r) == _lib.FLC_ERR_ARG
    r = diana_rows(100)
    r.d_b = None
    assert call(lib, prm, 2, 100, r) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 2, 100, diana_rows(100), out=None) == _lib.FLC_ERR_ARG
    assert call(lib, params(k=0), 2, 100, diana_rows(100)) == _lib.FLC_ERR_ARG      # K < 1
    assert call(lib, params(k=101), 2, 100, diana_rows(100)) == _lib.FLC_ERR_ARG    # K > d
    assert call(lib, params(k=100), 2, 100, diana_rows(100), ws_bytes=0) == _lib.FLC_ERR_WORKSPACE   # K == d: accepted
    assert call(lib, params(tie=7), 2, 100, diana_rows(100)) == _lib.FLC_ERR_ARG    # an unknown tie rule
    assert b"tie" in lib.flc_last_error_string()
    assert call(lib, params(tie=1), 2, 100, diana_rows(100), ws_bytes=0) == _lib.FLC_ERR_WORKSPACE
    big = 0xFFFFFFFF                                                       # d >= 2^32 - 1: 32-bit entry indices
    assert call(lib, params(), 1, big, diana_rows(big)) == _lib.FLC_ERR_ARG
    for rows in (diana_rows(100), ef21_rows(100)):                         # in-place rows that overlap
        rows.ldb = 99
        if rows.d_shift_out:
            rows.ldin = rows.ldout = 99
        else:
            rows.ldbase = rows.ldmsg = 99
        assert call(lib, params(), 2, 100, rows) == _lib.FLC_ERR_ARG
        assert b"overlap" in lib.flc_last_error_string()
        assert call(lib, params(), 1, 100, rows, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE   # one row cannot overlap


@pytest.mark.parametrize("codec", [_lib.FLC_IDENT, _lib.FLC_LAZY, _lib.FLC_RANDK, _lib.FLC_NATURAL, _lib.FLC_STD_DITHERING,
                                   _lib.FLC_NAT_DITHERING, _lib.FLC_RANK_K, 99])
def test_other_codecs_are_unsupported(codec):
    lib = _lib.load()
    prm = params(codec)
    assert call(lib, prm, 2, 100, diana_rows(100)) == _lib.FLC_ERR_UNSUPPORTED
    assert b"FLC_TOPK" in lib.flc_last_error_string()
    assert size(lib, prm, 2, 100) == 0


def unsupported(rows):
    lib = _lib.load()
    assert call(lib, params(), 2, 100, rows) == _lib.FLC_ERR_UNSUPPORTED
    msg = lib.flc_last_error_string()
    assert len(msg) > 0
    return msg


def test_shapes_outside_a_to_d_are_unsupported():
    d = 100
    r = diana_rows(d)
    r.d_shift_out = OTHER                                # shift_out rows that are not the b rows
    assert b"shift" in unsupported(r)
    r = diana_rows(d)
    r.ldout = d + 4                                      # ... or with another leading dimension
    assert b"shift" in unsupported(r)
    r = diana_rows(d)
    r.d_shift_in = OTHER
    assert b"shift" in unsupported(r)
    r = diana_rows(d)                                    # a shift together with a base
    r.d_base, r.ldbase = BASE, 0
    assert b"shift" in unsupported(r)
    r = _lib.FlcShiftRows()                              # a per-row base that is not d_msg == d_b
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale = A, d, B, d, 1.0
    r.d_base, r.ldbase = BASE, d
    assert b"base" in unsupported(r)
    r.d_msg, r.ldmsg = BASE, d
    assert b"d_msg" in unsupported(r)
    r.d_base, r.d_msg = B, OTHER                         # a dense message matrix
    assert b"d_msg" in unsupported(r)
    r = _lib.FlcShiftRows()                              # a stored message without a base
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale = A, d, B, d, 1.0
    r.d_msg, r.ldmsg = B, d
    assert b"d_msg" in unsupported(r)
    for ok in (diana_rows(d), ef21_rows(d)):             # A and B themselves pass the shape check
        assert call(_lib.load(), params(), 2, d, ok, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE
    r = _lib.FlcShiftRows()                              # C: one shared base
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale = A, d, B, d, 1.0
    r.d_base, r.ldbase = BASE, 0
    assert call(_lib.load(), params(), 2, d, r, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE


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


def test_workspace_one_byte_short():
    lib = _lib.load()
    n, d = 5, 100003
    prm = params(k=2001)
    need = size(lib, prm, n, d)
    assert need > 0
    assert call(lib, prm, n, d, diana_rows(d), ws_bytes=need - 1) == _lib.FLC_ERR_WORKSPACE
    assert b"workspace" in lib.flc_last_error_string()


def test_workspace_is_the_selection_state_and_the_difference_matrix():
    lib = _lib.load()
    n, d = 5, 100003
    prm = params(k=2001)
    sel = lib.flc_encode_reduce_workspace_size(ctypes.byref(prm), n, d)
    assert sel > 0
    assert 4 * n * d <= size(lib, prm, n, d) <= sel + 4 * n * (d + 3) + 1024
    assert size(lib, prm, n, d) >= sel + 4 * n * d


def test_general_entry_and_randk_entry_are_what_they_were():
    lib = _lib.load()
    gsize = lib.flc_encode_shift_reduce_workspace_size
    n, d = 5, 100003
    prm = params(k=2001)
    one = lib.flc_encode_shift_workspace_size(ctypes.byref(prm), d)
    assert gsize(ctypes.byref(prm), n, d) == gsize(ctypes.byref(prm), 1, d)
    assert one + 4 * d <= gsize(ctypes.byref(prm), n, d) <= one + 4 * d + 512
    # the sparse RandK entry keeps refusing TopK
    rc = lib.flc_randk_shift_reduce(ctypes.byref(prm), None, ctypes.byref(diana_rows(d)), n, d, None, ctypes.c_float(1.0),
                                    ctypes.c_void_p(OUT), ctypes.c_void_p(WS), 1 << 40, None)
    assert rc == _lib.FLC_ERR_UNSUPPORTED
    assert lib.flc_randk_shift_reduce_workspace_size(ctypes.byref(prm), None, n, d) == 0
