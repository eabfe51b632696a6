"""Host side of FRECON's two-message uplink (flc_frecon_reduce, aggregation.FreconUplinkReducer):
the exported symbols, the flc_frecon_rows / flc_frecon_server layouts against the C header, and the
answers the entry gives before it needs a device.  Every refused call below is refused on the host,
before any launch: the operand addresses are never dereferenced."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from flpytorch_amd import _lib

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADER = os.path.join(ROOT, "include", "flcodec.h")
NAMES = ("flc_frecon_reduce_workspace_size", "flc_frecon_reduce")
N, D = 3, 64
BASE = 1 << 20                       # operand addresses for the checks (16-byte aligned, never read)


def params(codec):
    prm = _lib.FlcCodecParams()
    prm.codec = codec
    return prm


def make_rows(ldh=D):
    fr = _lib.FlcFreconRows()
    fr.d_a, fr.lda = BASE, D
    fr.d_h, fr.ldh = BASE + 4 * N * D, ldh
    fr.d_p, fr.ldp = BASE + 8 * N * D, D
    fr.shift_alpha = 0.5
    return fr


OUT_U, OUT_Q, VEC = BASE + 12 * N * D, BASE + 12 * N * D + 4 * D, BASE + 12 * N * D + 8 * D


def make_server(result=VEC, h_prev_out=None):
    srv = _lib.FlcFreconServer()
    srv.d_g_server_prev, srv.d_h_prev = VEC + 4 * D, VEC + 8 * D
    srv.lambda_, srv.one_minus_lambda = 0.25, 0.75
    srv.d_result = result
    srv.alpha_update, srv.d_h_prev_out = 0.5, h_prev_out
    return srv


def call(lib, prm, n, d, rows=None, u=None, q=None, srv=None, ws_bytes=0):
    return lib.flc_frecon_reduce(ctypes.byref(prm), None, ctypes.byref(rows) if rows is not None else None, n, d,
                                 None, ctypes.c_float(1.0), None, None, u, q,
                                 ctypes.byref(srv) if srv is not None else None, None, ws_bytes, None)


def test_symbols_exported_and_declared():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert name in declared
        assert hasattr(lib, name), name
    assert lib.flc_version() == 104                     # additive: the ABI version does not move
    assert lib.flc_frecon_reduce_workspace_size.restype is ctypes.c_size_t


@pytest.mark.parametrize("ctype, cname", [(_lib.FlcFreconRows, "flc_frecon_rows"),
                                          (_lib.FlcFreconServer, "flc_frecon_server")])
def test_structs_match_the_header(tmp_path, ctype, cname):
    """ctypes.sizeof and every field offset equal the C struct's (C99 program built against
    include/flcodec.h)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in ctype._fields_]
    cfields = ["lambda" if f == "lambda_" else f for f in fields]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "flcodec.h"\n'
                   f'int main(void) {{ printf("%zu", sizeof({cname}));\n'
                   + "".join(f'printf(" %zu", offsetof({cname}, {f}));\n' for f in cfields)
                   + "return 0; }\n")
    exe = str(tmp_path / "layout")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                         str(src), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(ctype)
    assert got[1:] == [getattr(ctype, f).offset for f in fields]


@pytest.mark.parametrize("codec", [_lib.FLC_IDENT, _lib.FLC_LAZY, _lib.FLC_NATURAL, _lib.FLC_STD_DITHERING,
                                   _lib.FLC_NAT_DITHERING])
def test_empty_calls_need_no_device(codec):
    lib = _lib.load()
    prm = params(codec)
    rows = _lib.FlcFreconRows()
    assert call(lib, prm, 0, 1000, rows) == _lib.FLC_OK
    assert call(lib, prm, 5, 0, rows) == _lib.FLC_OK
    assert call(lib, prm, 0, 0) == _lib.FLC_OK
    assert call(lib, prm, -1, 4, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 4, -1, rows) == _lib.FLC_ERR_ARG


@pytest.mark.parametrize("codec", [_lib.FLC_RANDK, _lib.FLC_TOPK, _lib.FLC_RANK_K, 99])
def test_selection_codecs_are_refused_before_anything_else(codec):
    lib = _lib.load()
    prm = params(codec)
    prm.k = 4
    assert call(lib, prm, N, D, make_rows(), OUT_U, OUT_Q, ws_bytes=1 << 30) == _lib.FLC_ERR_UNSUPPORTED
    assert len(lib.flc_last_error_string()) > 0
    assert call(lib, prm, 0, 0) == _lib.FLC_ERR_UNSUPPORTED              # (even the empty call)
    assert lib.flc_frecon_reduce_workspace_size(ctypes.byref(prm), N, D) == 0


def test_host_side_refusals():
    lib = _lib.load()
    prm = params(_lib.FLC_NATURAL)
    big = 1 << 30
    assert call(lib, prm, 65536, 8, make_rows(), OUT_U, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG   # n > FLC_MAX_ROWS
    assert b"65535" in lib.flc_last_error_string()
    assert call(lib, prm, N, D, None, OUT_U, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG               # null rows
    for field in ("d_a", "d_h", "d_p"):                                                             # a null operand
        rows = make_rows()
        setattr(rows, field, None)
        assert call(lib, prm, N, D, rows, OUT_U, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG, field
    # without a server tail both averages are required; with one they are optional but its operands are not
    assert call(lib, prm, N, D, make_rows(), OUT_U, None, ws_bytes=big) == _lib.FLC_ERR_ARG
    assert call(lib, prm, N, D, make_rows(), None, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG
    for field in ("d_g_server_prev", "d_h_prev", "d_result"):
        srv = make_server()
        setattr(srv, field, None)
        assert call(lib, prm, N, D, make_rows(), None, None, srv, ws_bytes=big) == _lib.FLC_ERR_ARG, field
    # the h rows are written in place: they must not overlap each other
    assert call(lib, prm, N, D, make_rows(ldh=D - 1), OUT_U, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG
    assert b"overlap" in lib.flc_last_error_string()
    assert call(lib, prm, N, D, make_rows(ldh=0), OUT_U, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG
    # the tail's outputs may not lie over any row operand (first, middle and last row of each)
    rows = make_rows()
    for base in (rows.d_a, rows.d_h, rows.d_p):
        for off in (0, 4 * D, 4 * (N * D - 1)):
            assert call(lib, prm, N, D, rows, None, None, make_server(result=base + off), ws_bytes=big) == _lib.FLC_ERR_ARG
            assert b"overlaps" in lib.flc_last_error_string()
            assert call(lib, prm, N, D, rows, None, None, make_server(h_prev_out=base + off), ws_bytes=big) == _lib.FLC_ERR_ARG
    # lazy without its draws, dithering without levels: refused with the operands in order
    assert call(lib, params(_lib.FLC_LAZY), N, D, make_rows(), OUT_U, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG
    assert call(lib, params(_lib.FLC_STD_DITHERING), N, D, make_rows(), OUT_U, OUT_Q, ws_bytes=big) == _lib.FLC_ERR_ARG


@pytest.mark.parametrize("with_tail", [False, True])
def test_short_workspace_is_refused(with_tail):
    lib = _lib.load()
    prm = params(_lib.FLC_NATURAL)
    need = lib.flc_frecon_reduce_workspace_size(ctypes.byref(prm), N, D)
    assert need > 0
    srv = make_server(h_prev_out=VEC + 8 * D) if with_tail else None     # (h_prev' over h_prev is allowed)
    for short in (0, need - 1):
        assert call(lib, prm, N, D, make_rows(), OUT_U, OUT_Q, srv, ws_bytes=short) == _lib.FLC_ERR_WORKSPACE
    assert b"workspace" in lib.flc_last_error_string()


def test_workspace_size_is_monotone():
    lib = _lib.load()
    size = lib.flc_frecon_reduce_workspace_size
    for codec in (_lib.FLC_IDENT, _lib.FLC_LAZY):
        assert size(ctypes.byref(params(codec)), 5, 100003) == 0
    for codec in (_lib.FLC_NATURAL, _lib.FLC_STD_DITHERING, _lib.FLC_NAT_DITHERING):
        prm = params(codec)
        ns, ds = (1, 2, 5, 128, 4096), (1, 7, 4099, 100003, 25_000_000)
        grid = [[size(ctypes.byref(prm), n, d) for d in ds] for n in ns]
        assert all(v > 0 for row in grid for v in row)
        for i in range(len(ns)):
            for j in range(len(ds)):
                assert i == 0 or grid[i][j] >= grid[i - 1][j], (codec, ns[i], ds[j])
                assert j == 0 or grid[i][j] >= grid[i][j - 1], (codec, ns[i], ds[j])
        # two sets of the shifted fold's row tables: one per message
        assert grid[2][3] == 2 * lib.flc_encode_shift_reduce_workspace_size(ctypes.byref(prm), 5, 100003)
    assert size(ctypes.byref(params(_lib.FLC_NATURAL)), -1, 8) == 0


def test_reducer_and_helpers_are_exported():
    import torch

    from flpytorch_amd import aggregation as ag
    for name in ("FreconUplinkReducer", "freconStep", "cofigStep", "freconUplink", "cofigUplink"):
        assert callable(getattr(ag, name)), name
    comp = ag.initCompressor("natural", 16)
    if torch.cuda.is_available():
        assert ag.FreconUplinkReducer(comp, seed=1).comp is comp
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.FreconUplinkReducer(comp)
