"""Host side of the fused shifted uplink (flc_encode_shift_reduce, aggregation.ShiftUplinkReducer):
the exported symbols, the flc_shift_rows layout against the C header, and the answers the entry
gives before it needs a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from flpytorch_amd import _lib

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADER = os.path.join(ROOT, "include", "flcodec.h")
NAMES = ("flc_encode_shift_reduce_workspace_size", "flc_encode_shift_reduce")


def params(codec):
    prm = _lib.FlcCodecParams()
    prm.codec = codec
    return prm


def call(lib, prm, n, d, rows=None):
    return lib.flc_encode_shift_reduce(ctypes.byref(prm), None, ctypes.byref(rows) if rows is not None else None, n, d,
                                       None, ctypes.c_float(1.0), None, None, None, 0, None)


def test_symbols_exported_and_declared():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert name in declared
        assert hasattr(lib, name), name
    assert lib.flc_version() == 104                     # additive: the ABI version does not move
    assert lib.flc_encode_shift_reduce_workspace_size.restype is ctypes.c_size_t


def test_shift_rows_struct_matches_the_header(tmp_path):
    """ctypes.sizeof(FlcShiftRows) and every field offset equal the C struct's (C99 program built
    against include/flcodec.h)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    fields = [f[0] for f in _lib.FlcShiftRows._fields_]
    src = tmp_path / "rows_layout.c"
    src.write_text('#include <stdio.h>\n#include "flcodec.h"\n'
                   'int main(void) { printf("%zu", sizeof(flc_shift_rows));\n'
                   + "".join(f'printf(" %zu", offsetof(flc_shift_rows, {f}));\n' for f in fields)
                   + "return 0; }\n")
    exe = str(tmp_path / "rows_layout")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                         str(src), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.FlcShiftRows)
    assert got[1:] == [getattr(_lib.FlcShiftRows, f).offset for f in fields]


@pytest.mark.parametrize("codec", [_lib.FLC_IDENT, _lib.FLC_NATURAL, _lib.FLC_STD_DITHERING, _lib.FLC_TOPK, _lib.FLC_RANK_K])
def test_empty_calls_need_no_device(codec):
    lib = _lib.load()
    prm = params(codec)
    rows = _lib.FlcShiftRows()
    assert call(lib, prm, 0, 1000, rows) == _lib.FLC_OK
    assert call(lib, prm, 5, 0, rows) == _lib.FLC_OK
    assert call(lib, prm, 0, 0) == _lib.FLC_OK
    assert call(lib, prm, -1, 4, rows) == _lib.FLC_ERR_ARG
    assert call(lib, prm, 4, -1, rows) == _lib.FLC_ERR_ARG


def test_host_side_refusals():
    lib = _lib.load()
    prm = params(99)
    assert call(lib, prm, 0, 0) == _lib.FLC_ERR_UNSUPPORTED
    assert len(lib.flc_last_error_string()) > 0
    assert lib.flc_encode_shift_reduce_workspace_size(ctypes.byref(prm), 4, 1000) == 0
    prm = params(_lib.FLC_NATURAL)
    rows = _lib.FlcShiftRows()
    assert call(lib, prm, 65536, 8, rows) == _lib.FLC_ERR_ARG            # n > FLC_MAX_ROWS
    assert b"65535" in lib.flc_last_error_string()
    assert call(lib, prm, 2, 8, rows) == _lib.FLC_ERR_ARG                # null a / b / out
    assert call(lib, prm, 2, 8) == _lib.FLC_ERR_ARG                      # null rows
    prm = params(_lib.FLC_TOPK)
    prm.tie = 7
    assert call(lib, prm, 0, 0) == _lib.FLC_ERR_ARG                      # unknown tie rule, before anything else


def test_workspace_sizes():
    lib = _lib.load()
    size = lib.flc_encode_shift_reduce_workspace_size
    n, d = 5, 100003
    assert size(ctypes.byref(params(_lib.FLC_IDENT)), n, d) == 0
    assert size(ctypes.byref(params(_lib.FLC_NATURAL)), n, d) > 0
    # RandK / TopK / Rank-K: one message row on top of flc_encode_shift's own workspace, whatever n is
    prm = params(_lib.FLC_TOPK)
    prm.k = 2001
    one = lib.flc_encode_shift_workspace_size(ctypes.byref(prm), d)
    assert size(ctypes.byref(prm), n, d) == size(ctypes.byref(prm), 1, d)
    assert one + 4 * d <= size(ctypes.byref(prm), n, d) <= one + 4 * d + 512
    # the existing entries' sizes are what they were
    assert lib.flc_encode_shift_workspace_size(ctypes.byref(params(_lib.FLC_IDENT)), d) == 0


def test_reducer_needs_a_gpu():
    import torch

    from flpytorch_amd import aggregation as ag
    assert ag.ShiftUplinkReducer is not None and ag.dianaUplink and ag.ef21Uplink and ag.marinaUplink
    comp = ag.initCompressor("natural", 16)
    if torch.cuda.is_available():
        assert ag.ShiftUplinkReducer(comp, seed=1).comp is comp
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.ShiftUplinkReducer(comp)
