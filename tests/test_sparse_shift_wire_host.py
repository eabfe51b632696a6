"""Host side of the sparse shifted-wire fold (flc_unpack_shift_reduce_sparse): the exported symbols
and the answers the entry gives before it needs a device (made-up device addresses are enough:
nothing is launched), from Python and from the C program tests/c/sparse_shift_refusals.c."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from flpytorch_amd import _lib
from tests.test_shift_wire_host import BASE, D, HEADER, MSG, OUT, ROOT, WS, params, payload_rows

NAMES = ("flc_unpack_shift_reduce_sparse_workspace_size", "flc_unpack_shift_reduce_sparse")
SPARSE = (_lib.FLC_RANDK, _lib.FLC_TOPK)


def fold(prm, rows, n=2, d=D, out=OUT, ws_bytes=1 << 40):
    return _lib.load().flc_unpack_shift_reduce_sparse(ctypes.byref(prm), ctypes.byref(rows), None, n, d, None,
                                                      ctypes.c_float(1.0), ctypes.c_void_p(out), ctypes.c_void_p(WS), ws_bytes,
                                                      None)


def rows_with(prm, scale=1.0, **fields):
    r = payload_rows(prm)
    r.msg_scale = scale
    for k, v in fields.items():
        setattr(r, k, v)
    return r


def test_symbols_and_size_query():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared and hasattr(lib, name), name
    size = lib.flc_unpack_shift_reduce_sparse_workspace_size
    assert size.restype is ctypes.c_size_t and lib.flc_version() == 104
    for codec in range(0, 10):                               # the tile table alone: 8 n ceil(d / 4096) bytes
        assert size(ctypes.byref(params(codec)), 3, D) == (256 if codec in SPARSE else 0), codec
        assert fold(params(codec), payload_rows(params(_lib.FLC_TOPK)), ws_bytes=0) == (
            _lib.FLC_ERR_WORKSPACE if codec in SPARSE else _lib.FLC_ERR_UNSUPPORTED), codec
    assert size(ctypes.byref(params(_lib.FLC_TOPK)), -1, D) == 0 and size(ctypes.byref(params(_lib.FLC_TOPK)), 3, -1) == 0


@pytest.mark.parametrize("codec", SPARSE)
def test_refusals_and_accepted_shapes(codec):
    lib = _lib.load()
    prm = params(codec)
    pb = lib.flc_payload_bytes(ctypes.byref(prm), D)
    mirror = dict(d_base=BASE, ldbase=D + 1, d_msg=BASE, ldmsg=D + 1)
    for r in (rows_with(prm), rows_with(prm, d_base=BASE, ldbase=0), rows_with(prm, **mirror)):   # D, C, B
        assert fold(prm, r, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE                # taken up to the last check
    assert fold(prm, rows_with(prm, d_base=BASE, ldbase=D, d_msg=MSG, ldmsg=D)) == _lib.FLC_ERR_UNSUPPORTED
    assert fold(prm, rows_with(prm, d_base=BASE, ldbase=D)) == _lib.FLC_ERR_UNSUPPORTED
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        assert fold(prm, rows_with(prm, scale, **mirror)) == _lib.FLC_ERR_UNSUPPORTED
        assert b"msg_scale" in lib.flc_last_error_string()
    for ld in (pb - 16, pb + 8):
        assert fold(prm, payload_rows(prm, ld=ld)) == _lib.FLC_ERR_ARG
    assert fold(prm, rows_with(prm, d_base=BASE, ldbase=D - 1, d_msg=BASE, ldmsg=D - 1)) == _lib.FLC_ERR_ARG
    assert b"overlap" in lib.flc_last_error_string()
    assert fold(prm, payload_rows(prm), d=0, out=None) == _lib.FLC_OK


def test_c_program_of_the_refusals(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "sparse_shift_refusals")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "c", "sparse_shift_refusals.c"), "-L" + libdir, "-lflcodec",
                         "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "OK" in run.stdout, run.stdout + run.stderr
