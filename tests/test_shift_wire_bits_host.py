"""Host side of the bit-packed shifted steps (flc_pack_shift_bits / flc_unpack_shift_reduce_bits): the
exported symbols and prototypes, the size queries, and every refusal that needs no device (made-up
device addresses: nothing is launched)."""
import ctypes
import re

import pytest

from flpytorch_amd import _lib
from flpytorch_amd import aggregation as ag
from tests.test_shift_wire_host import A, B, BASE, D, HEADER, MSG, OUT, PAY, WS, params

NAMES = ("flc_pack_shift_bits_workspace_size", "flc_pack_shift_bits", "flc_unpack_shift_reduce_bits_workspace_size",
         "flc_unpack_shift_reduce_bits")
NO_BITS = [(_lib.FLC_STD_DITHERING, 127), (_lib.FLC_NAT_DITHERING, 4), (_lib.FLC_TOPK, 4), (_lib.FLC_RANDK, 4),
           (_lib.FLC_IDENT, 4), (_lib.FLC_RANK_K, 4), (99, 4)]


def pack(prm, d=D, a=A, b=B, base=None, msg=None, shift_out=None, payload=PAY, ws_bytes=1 << 40):
    vp = ctypes.c_void_p
    return _lib.load().flc_pack_shift_bits(ctypes.byref(prm), None, vp(a), vp(b), d, ctypes.c_float(1.0), vp(base), vp(msg),
                                           ctypes.c_float(0.5), None, vp(shift_out), vp(payload), vp(WS), ws_bytes, None)


def fold(prm, n=2, d=D, out=OUT, ld=None, base=None, ldbase=0, msg=None, ldmsg=0):
    r = _lib.FlcPayloadRows()
    r.d_payloads, r.msg_scale = PAY, 1.0
    r.ld_bytes = _lib.load().flc_payload_bits_bytes(ctypes.byref(prm), d) if ld is None else ld
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = base, ldbase, msg, ldmsg
    return _lib.load().flc_unpack_shift_reduce_bits(ctypes.byref(prm), ctypes.byref(r), n, d, None, ctypes.c_float(1.0),
                                                    ctypes.c_void_p(out), None, 0, None)


def test_symbols_prototypes_and_sizes():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS and name in declared and hasattr(lib, name), name
    assert lib.flc_version() == 104                     # additive: the ABI version does not move
    assert lib.flc_pack_shift_bits.argtypes == lib.flc_pack_shift.argtypes
    assert lib.flc_unpack_shift_reduce_bits.argtypes == lib.flc_unpack_shift_reduce.argtypes
    for name in NAMES[::2]:
        assert getattr(lib, name).restype is ctypes.c_size_t
    for prm in (params(s=7), params(_lib.FLC_NATURAL)):
        assert lib.flc_pack_shift_bits_workspace_size(ctypes.byref(prm), D) == lib.flc_pack_bits_workspace_size(ctypes.byref(prm), D) > 0
        assert lib.flc_pack_shift_bits_workspace_size(ctypes.byref(prm), -1) == 0
        assert lib.flc_unpack_shift_reduce_bits_workspace_size(ctypes.byref(prm), 128, D) == 0    # registers only


@pytest.mark.parametrize("codec,s", NO_BITS)
def test_codecs_without_a_bit_packed_form(codec, s):
    lib = _lib.load()
    prm = params(codec, s)
    assert lib.flc_pack_shift_bits_workspace_size(ctypes.byref(prm), D) == 0
    assert pack(prm) == _lib.FLC_ERR_UNSUPPORTED and len(lib.flc_last_error_string()) > 0
    assert fold(prm, ld=1 << 20) == _lib.FLC_ERR_UNSUPPORTED and len(lib.flc_last_error_string()) > 0


def test_argument_errors():
    prm = params(s=7)
    for kw in ({"d": -1}, {"a": None}, {"b": None}, {"payload": None}, {"payload": PAY + 8}, {"shift_out": B}, {"base": BASE}):
        assert pack(prm, **kw) == _lib.FLC_ERR_ARG, kw
    # taken up to the workspace check, the last one before the first launch: every operand shape
    for kw in ({}, {"msg": MSG}, {"base": B, "msg": B}, {"base": BASE, "msg": MSG}, {"a": A + 4, "b": B + 4}):
        assert pack(prm, ws_bytes=0, **kw) == _lib.FLC_ERR_WORKSPACE, kw
    pb = _lib.load().flc_payload_bits_bytes(ctypes.byref(prm), D)
    for kw in ({"n": -1}, {"d": -1}, {"out": None}, {"ld": pb - 16}, {"ld": pb + 8},
               {"msg": MSG, "ldmsg": D - 1},                                     # msg rows overlap each other
               {"base": BASE, "msg": BASE},                                      # msg over the shared base
               {"base": BASE, "ldbase": D, "msg": BASE + 4 * D, "ldmsg": D}):    # msg row i is base row i + 1
        assert fold(prm, **kw) == _lib.FLC_ERR_ARG, kw
    assert fold(prm, n=65536) == _lib.FLC_ERR_UNSUPPORTED          # n > FLC_MAX_ROWS
    assert fold(prm, d=0) == _lib.FLC_OK                # nothing to do: the device is not touched


def test_python_refusals_need_no_device():
    for spec in ("qsgd:127", "topk:1%", "rank_k:2"):
        c = ag.initCompressor(spec, 4096)
        with pytest.raises(NotImplementedError):
            c.compressShiftPayload(None, None, bits=True)
        with pytest.raises(NotImplementedError):
            c.decompressShiftPayload(None, 4096, bits=True)
        with pytest.raises(NotImplementedError):
            ag.ShiftPayloadReducer(c, bits=True)
    assert ag.initCompressor("qsgd:7", 4096).payloadBytes(bits=True) * 2 == ag.initCompressor("qsgd:7", 4096).payloadBytes() + 16
