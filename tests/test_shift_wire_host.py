"""Host side of the shifted steps on the wire (flc_pack_shift / flc_unpack_shift_reduce): the exported
symbols, every answer the entries give before they need a device (made-up device addresses are enough:
nothing is launched), and the harness's ``shift_wire`` plumbing through a compressor double built on
the oracle (shift_step + wire.pack on the client side, wire.unpack on the server's)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from flpytorch_amd import _lib
from oracle import codecs as oc
from oracle import wire
from tests.harness_cases import META, RUN_NAMES, check_history, simulation
from tests.test_harness import (OracleCompressorDouble, oracle_diana_step, oracle_ef21_step, oracle_marina_step,
                                oracle_server_gradient, oracle_server_gradient_diana, oracle_simulation)

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADER = os.path.join(ROOT, "include", "flcodec.h")
NAMES = ("flc_pack_shift_workspace_size", "flc_pack_shift", "flc_unpack_shift_reduce_workspace_size",
         "flc_unpack_shift_reduce")
A, B, BASE, MSG, OUT, WS, LEV, PAY, PTRS = (0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000,
                                            0x70000000, 0x78000000, 0x7C000000)
D = 4099
CODECS = (_lib.FLC_IDENT, _lib.FLC_LAZY, _lib.FLC_RANDK, _lib.FLC_NATURAL, _lib.FLC_STD_DITHERING,
          _lib.FLC_NAT_DITHERING, _lib.FLC_TOPK)


def params(codec=_lib.FLC_STD_DITHERING, s=4):
    prm = _lib.FlcCodecParams()
    prm.codec = codec
    prm.s = s
    prm.norm = _lib.FLC_NORM_L2
    prm.k = 10
    prm.randk_scale = D / 10
    prm.d_levels = LEV
    prm.seed = 7
    return prm


def pack(prm, d=D, a=A, b=B, base=None, msg=None, shift_in=None, shift_out=None, payload=PAY, ws_bytes=1 << 40):
    vp = ctypes.c_void_p
    return _lib.load().flc_pack_shift(ctypes.byref(prm), None, vp(a), vp(b), d, ctypes.c_float(1.0), vp(base), vp(msg),
                                      ctypes.c_float(0.5), vp(shift_in), vp(shift_out), vp(payload), vp(WS), ws_bytes, None)


def payload_rows(prm, d=D, ld=None):
    r = _lib.FlcPayloadRows()
    r.d_payloads = PAY
    r.ld_bytes = _lib.load().flc_payload_bytes(ctypes.byref(prm), d) if ld is None else ld
    r.msg_scale = 1.0
    return r


def unpack(prm, rows, n=2, d=D, out=OUT, ws_bytes=1 << 40):
    return _lib.load().flc_unpack_shift_reduce(ctypes.byref(prm), ctypes.byref(rows) if rows is not None else None, n, d,
                                               None, ctypes.c_float(1.0), ctypes.c_void_p(out), ctypes.c_void_p(WS),
                                               ws_bytes, None)


def test_symbols_exported_and_declared():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert name in declared
        assert hasattr(lib, name), name
    assert lib.flc_version() == 104                     # additive: the ABI version does not move
    assert lib.flc_pack_shift_workspace_size.restype is ctypes.c_size_t
    assert lib.flc_unpack_shift_reduce_workspace_size.restype is ctypes.c_size_t


def test_size_queries():
    lib = _lib.load()
    for codec in CODECS:
        prm = params(codec)
        assert lib.flc_pack_shift_workspace_size(ctypes.byref(prm), D) > 0
        assert lib.flc_pack_shift_workspace_size(ctypes.byref(prm), -1) == 0
        assert lib.flc_unpack_shift_reduce_workspace_size(ctypes.byref(prm), 2, -1) == 0
        assert lib.flc_unpack_shift_reduce_workspace_size(ctypes.byref(prm), -2, D) == 0
        sparse = codec in (_lib.FLC_RANDK, _lib.FLC_TOPK)
        assert (lib.flc_unpack_shift_reduce_workspace_size(ctypes.byref(prm), 2, D) > 0) == sparse
    for codec in (_lib.FLC_RANK_K, 0, 99):              # Rank-K and unknown codecs
        prm = params(codec)
        assert lib.flc_pack_shift_workspace_size(ctypes.byref(prm), D) == 0
        assert lib.flc_unpack_shift_reduce_workspace_size(ctypes.byref(prm), 2, D) == 0


@pytest.mark.parametrize("codec", [_lib.FLC_RANK_K, 0, 99])
def test_unsupported_codecs(codec):
    lib = _lib.load()
    prm = params(codec)
    assert pack(prm) == _lib.FLC_ERR_UNSUPPORTED
    assert len(lib.flc_last_error_string()) > 0
    assert unpack(prm, payload_rows(params())) == _lib.FLC_ERR_UNSUPPORTED
    assert len(lib.flc_last_error_string()) > 0
    if codec == _lib.FLC_RANK_K:
        assert b"Rank-K" in lib.flc_last_error_string()


@pytest.mark.parametrize("codec", CODECS)
def test_pack_shift_argument_errors(codec):
    prm = params(codec)
    assert pack(prm, d=-1) == _lib.FLC_ERR_ARG
    assert pack(prm, a=None) == _lib.FLC_ERR_ARG
    assert pack(prm, b=None) == _lib.FLC_ERR_ARG
    assert pack(prm, payload=None) == _lib.FLC_ERR_ARG
    assert pack(prm, d=0, payload=None) == _lib.FLC_ERR_ARG          # d == 0 still writes the empty header
    assert pack(prm, payload=PAY + 8) == _lib.FLC_ERR_ARG            # not 16-byte aligned
    assert pack(prm, shift_out=B) == _lib.FLC_ERR_ARG                # shift_out without shift_in
    assert pack(prm, base=BASE) == _lib.FLC_ERR_ARG                  # base without msg
    # taken up to the workspace check, the last one before the first launch: every operand shape
    for kw in ({}, {"msg": MSG}, {"base": B, "msg": B}, {"shift_in": B, "shift_out": B}, {"base": BASE, "msg": MSG},
               {"shift_in": B}, {"a": A + 4, "b": B + 4}):
        assert pack(prm, ws_bytes=0, **kw) == _lib.FLC_ERR_WORKSPACE, kw
    assert b"workspace" in _lib.load().flc_last_error_string()


@pytest.mark.parametrize("codec", CODECS)
def test_unpack_shift_reduce_argument_errors(codec):
    lib = _lib.load()
    prm = params(codec)
    pb = lib.flc_payload_bytes(ctypes.byref(prm), D)
    assert pb > 16 and pb % 16 == 0
    ok = payload_rows(prm)
    assert unpack(prm, ok, n=-1) == _lib.FLC_ERR_ARG
    assert unpack(prm, ok, d=-1) == _lib.FLC_ERR_ARG
    assert unpack(prm, ok, out=None) == _lib.FLC_ERR_ARG
    assert unpack(prm, None) == _lib.FLC_ERR_ARG                     # null rows with work to do
    assert unpack(prm, _lib.FlcPayloadRows()) == _lib.FLC_ERR_ARG    # neither payload rows nor pointers
    assert unpack(prm, ok, n=65536) == _lib.FLC_ERR_UNSUPPORTED      # n > FLC_MAX_ROWS, as flc_unpack_reduce
    assert b"65535" in lib.flc_last_error_string()
    r = payload_rows(prm)
    r.d_payloads = PAY + 4
    assert unpack(prm, r) == _lib.FLC_ERR_ARG                        # payload rows not 16-byte aligned
    assert unpack(prm, payload_rows(prm, ld=pb - 16)) == _lib.FLC_ERR_ARG     # ld_bytes < flc_payload_bytes
    assert unpack(prm, payload_rows(prm, ld=pb + 8)) == _lib.FLC_ERR_ARG      # ld_bytes % 16 != 0
    r = payload_rows(prm)
    r.d_msg, r.ldmsg = MSG, D - 1
    assert unpack(prm, r) == _lib.FLC_ERR_ARG                        # the d_msg rows overlap
    assert b"overlap" in lib.flc_last_error_string()
    r.ldmsg = -(D - 1)
    assert unpack(prm, r) == _lib.FLC_ERR_ARG
    r = payload_rows(prm)
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = BASE, 0, BASE - 4 * D, D  # msg row 1 is the shared base
    assert unpack(prm, r) == _lib.FLC_ERR_ARG
    assert b"shared base" in lib.flc_last_error_string()
    assert unpack(prm, ok, d=0) == _lib.FLC_OK                       # d == 0: nothing to do, no device
    assert unpack(prm, None, n=0, d=0) == _lib.FLC_OK
    assert unpack(prm, ok, n=5, d=0, out=None) == _lib.FLC_OK


def test_unpack_shift_reduce_accepted_shapes():
    """Taken up to the workspace check (the last one before the first launch) — with a SPARSE codec,
    whose server fold needs a workspace."""
    prm = params(_lib.FLC_TOPK)
    shapes = []
    shapes.append(payload_rows(prm))                                 # no base: flc_unpack_reduce's fold
    r = payload_rows(prm)
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = BASE, D, MSG, D           # per-row base, stored out of place
    shapes.append(r)
    r = payload_rows(prm)
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = BASE, D + 1, BASE, D + 1  # the EF21 mirror in place (odd ld)
    shapes.append(r)
    r = payload_rows(prm)
    r.d_base, r.ldbase = BASE, 0                                     # MARINA's shared base
    shapes.append(r)
    r = payload_rows(prm, ld=_lib.load().flc_payload_bytes(ctypes.byref(prm), D) + 32)
    shapes.append(r)
    r = _lib.FlcPayloadRows()
    r.d_payload_ptrs, r.msg_scale = PTRS, 0.25                       # a device pointer list
    shapes.append(r)
    for r in shapes:
        assert unpack(prm, r, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE
    r = payload_rows(prm)
    r.d_msg, r.ldmsg = MSG, D - 1
    assert unpack(prm, r, n=1, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE  # one row cannot overlap
    r = payload_rows(prm)
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = BASE, 0, BASE, D
    assert unpack(prm, r, n=1, ws_bytes=0) == _lib.FLC_ERR_WORKSPACE  # one row over its base: in place


# ---- the harness's shift_wire plumbing through a double -------------------------------------------
class WireDouble(OracleCompressorDouble):
    """compressShiftPayload / decompressShiftPayload over the oracle: the client packs the oracle's
    C(a - b), the server unpacks it and applies base + dec * scale in fp32."""
    payloads = 0

    def compressShiftPayload(self, a, b, *, scale=1.0, base=None, out=None, alpha=None, shift=None, shift_out=None,
                             message=False, payload_out=None):
        an, bn = a.detach().cpu().numpy(), b.detach().cpu().numpy()
        o = self.o
        pn = o.norm((an - bn).astype(np.float32)) if o.type in (oc.STD_DITHERING, oc.NAT_DITHERING) else None
        e, _ = oc.shift_step(o, an, bn)
        msg, h2 = oc.shift_step(o, an, bn, scale=scale, base=None if base is None else base.numpy(), alpha=alpha,
                                h=None if shift is None else shift.numpy())
        self.last_need_to_send_advance = o.last_need_to_send_advance
        payload = torch.from_numpy(wire.pack(o, e, pn))
        WireDouble.payloads += 1
        return (payload, torch.from_numpy(msg) if (message or out is not None) else None,
                None if h2 is None else torch.from_numpy(h2))

    def decompressShiftPayload(self, payload, d=None, *, scale=1.0, base=None, out=None):
        dec = wire.unpack(self.o, payload.numpy(), int(d))
        t = (dec * np.float32(scale)).astype(np.float32)
        return torch.from_numpy(t if base is None else (base.numpy() + t).astype(np.float32))


def first_run(algorithm):
    return next(n for n in RUN_NAMES if META[n]["algorithm"] == algorithm)


@pytest.mark.parametrize("algorithm", ["diana", "ef21", "marina"])
def test_shift_wire_plumbing_matches_the_plain_oracle_run(algorithm):
    name = first_run(algorithm)
    plain = oracle_simulation(name, record_iterates=True)
    Hp = plain.run()
    WireDouble.payloads = 0
    fold = oracle_server_gradient_diana if algorithm == "diana" else oracle_server_gradient
    sim = simulation(name, "cpu", init_compressor=WireDouble, server_gradient=fold, diana_step=oracle_diana_step,
                     ef21_step=oracle_ef21_step, marina_step=oracle_marina_step, record_iterates=True, shift_wire=True)
    Hw = sim.run()
    check_history(name, Hw)
    assert WireDouble.payloads > 0
    shipped = 0
    for r in Hp["history"]:
        for k in ("grad_sgd_server_l2", "x_before_round", "approximate_f_avg_value"):
            assert Hp["history"][r][k] == Hw["history"][r][k] or (np.isnan(Hp["history"][r][k]) and np.isnan(Hw["history"][r][k]))
        for c, st in Hw["history"][r]["client_states"].items():
            want = Hp["history"][r]["client_states"][c]["client_state"]["stats"]["send_scalars_to_master"]
            assert st["client_state"]["stats"]["send_scalars_to_master"] == want
            shipped += st["client_state"]["stats"].get("payload_bytes", 0)
    assert shipped > 0
    for a, b in zip(plain.iterates, sim.iterates):
        assert np.array_equal(a.numpy().view(np.uint32), b.numpy().view(np.uint32))


def test_shift_wire_value_errors():
    name = first_run("diana")
    with pytest.raises(ValueError, match="shift_wire"):
        oracle_simulation(first_run("dcgd"), shift_wire=True)                 # another algorithm
    with pytest.raises(ValueError, match="shift_wire"):
        oracle_simulation(name, shift_wire="pipe")                            # another value
    for other in (name, first_run("dcgd")):
        with pytest.raises(ValueError, match="shift_wire"):
            oracle_simulation(other, shift_wire=True, wire=True)              # together with wire
