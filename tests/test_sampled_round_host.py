"""Host side of the sampled rounds (flc_encode / randk / topk _shift_reduce_sampled): the exported
symbols, the flc_row_map layout and every answer the entries give before they need a device.  The
refusals are decided from pointers, leading dimensions, bits and the HOST id array alone, so made-up
device addresses are enough here (nothing is launched, nothing but h_ids is dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest

from flpytorch_amd import _lib

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADER = os.path.join(ROOT, "include", "flcodec.h")
ENTRIES = ("flc_encode_shift_reduce_sampled", "flc_randk_shift_reduce_sampled", "flc_topk_shift_reduce_sampled")
A, B, BASE, OTHER, OUT, WS, DIDS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000
IDX_B, IDX_BASE, IDX_MSG, IDX_IN, IDX_OUT = 1, 2, 4, 8, 16
N_TOTAL, D = 7, 100


def params(codec, k=10):
    prm = _lib.FlcCodecParams()
    prm.codec = codec
    prm.k = k
    prm.randk_scale = 2.0
    return prm


def diana_rows(d=D):
    r = _lib.FlcShiftRows()
    r.d_a, r.lda, r.d_b, r.ldb = A, d, B, d
    r.d_shift_in, r.ldin, r.d_shift_out, r.ldout = B, d, B, d
    r.msg_scale, r.shift_alpha = 1.0, 0.5
    return r


def ef21_rows(d=D):
    r = _lib.FlcShiftRows()
    r.d_a, r.lda, r.d_b, r.ldb = A, d, B, d
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = B, d, B, d
    r.msg_scale = 1.0
    return r


def marina_rows(d=D):
    r = _lib.FlcShiftRows()
    r.d_a, r.lda, r.d_b, r.ldb = A, d, B, d
    r.d_base, r.ldbase = BASE, 0
    r.msg_scale = 1.0
    return r


class Map:
    """A flc_row_map over a real host id array (kept alive here) and a made-up device address."""

    def __init__(self, ids, indexed, n_total=N_TOTAL, h=True, dev=True):
        self.ids = np.asarray(ids, dtype=np.int32)
        self.m = _lib.FlcRowMap()
        self.m.h_ids = self.ids.ctypes.data if h else None
        self.m.d_ids = DIDS if dev else None
        self.m.n_total, self.m.indexed = n_total, indexed


ENTRY_CODEC = {"general": _lib.FLC_NATURAL, "randk": _lib.FLC_RANDK, "topk": _lib.FLC_TOPK}


def call(which, rows, mp, n, d=D, prm=None, pat=None, out=OUT, ws_bytes=0):
    """The entry `which` with no workspace: a call that passes every host check answers
    FLC_ERR_WORKSPACE (ident needs none, so the tests use codecs that do), a refused one its status."""
    lib = _lib.load()
    prm = prm or params(ENTRY_CODEC[which])
    rp = ctypes.byref(rows) if rows is not None else None
    mpp = ctypes.byref(mp.m) if mp is not None else None
    vp = ctypes.c_void_p
    if which == "general":
        return lib.flc_encode_shift_reduce_sampled(ctypes.byref(prm), ctypes.byref(pat) if pat else None, rp, mpp, n, d, None,
                                                   ctypes.c_float(1.0), None, vp(out), vp(WS), ws_bytes, None)
    if which == "randk":
        return lib.flc_randk_shift_reduce_sampled(ctypes.byref(prm), ctypes.byref(pat) if pat else None, rp, mpp, n, d, None,
                                                  ctypes.c_float(1.0), vp(out), vp(WS), ws_bytes, None)
    return lib.flc_topk_shift_reduce_sampled(ctypes.byref(prm), rp, mpp, n, d, None, ctypes.c_float(1.0), vp(out), vp(WS),
                                             ws_bytes, None)


WHICH = ("general", "randk", "topk")
DIANA_BITS = IDX_B | IDX_IN | IDX_OUT
EF21_BITS = IDX_B | IDX_BASE | IDX_MSG


def test_symbols_exported_and_declared():
    lib = _lib.load()
    declared = set(re.findall(r"\b(flc_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    for name in ENTRIES:
        for sym in (name, name + "_workspace_size"):
            assert sym in _lib.EXPORTS
            assert sym in declared
            assert hasattr(lib, sym), sym
        assert getattr(lib, name + "_workspace_size").restype is ctypes.c_size_t
    assert lib.flc_version() == 104                     # additive: the ABI version does not move


def test_row_map_layout_matches_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} flc_row_map;", text).group(1)
    fields = re.findall(r"^\s*(const int32_t\*|int64_t|uint32_t)\s+(\w+);", body, flags=re.M)
    assert [f[1] for f in fields] == [f[0] for f in _lib.FlcRowMap._fields_] == ["h_ids", "d_ids", "n_total", "indexed"]
    ctype_of = {"const int32_t*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32}
    assert [ctype_of[f[0]] for f in fields] == [f[1] for f in _lib.FlcRowMap._fields_]
    assert ctypes.sizeof(_lib.FlcRowMap) == 32 and _lib.FlcRowMap.indexed.offset == 24
    for name, val in (("B", 1), ("BASE", 2), ("MSG", 4), ("SHIFT_IN", 8), ("SHIFT_OUT", 16)):
        assert re.search(r"#define FLC_IDX_%s %d\b" % (name, val), text)
        assert getattr(_lib, "FLC_IDX_" + name) == val


@pytest.mark.parametrize("which", WHICH)
def test_empty_calls_need_no_device_and_no_map(which):
    assert call(which, _lib.FlcShiftRows(), None, 0, 1000) == _lib.FLC_OK
    assert call(which, _lib.FlcShiftRows(), None, 5, 0) == _lib.FLC_OK
    assert call(which, None, None, 0, 0) == _lib.FLC_OK
    assert call(which, _lib.FlcShiftRows(), Map([0], 0), -1, 4) == _lib.FLC_ERR_ARG
    assert call(which, diana_rows(), Map([0], DIANA_BITS), 65536) == _lib.FLC_ERR_ARG        # n > FLC_MAX_ROWS
    assert call(which, _lib.FlcShiftRows(), Map([0, 1], 0), 2) == _lib.FLC_ERR_ARG            # null a / b


@pytest.mark.parametrize("which", WHICH)
def test_a_good_call_gets_as_far_as_the_workspace(which):
    for ids in ([5, 0, 3], [6], [6, 5, 4, 3, 2, 1, 0], list(range(7))):
        assert call(which, diana_rows(), Map(ids, DIANA_BITS), len(ids)) == _lib.FLC_ERR_WORKSPACE
        assert call(which, ef21_rows(), Map(ids, EF21_BITS), len(ids)) == _lib.FLC_ERR_WORKSPACE
        assert call(which, marina_rows(), Map(ids, 0), len(ids)) == _lib.FLC_ERR_WORKSPACE
    # bits of absent operands are ignored; duplicates are fine while no output is indexed
    assert call(which, marina_rows(), Map([3, 3], IDX_MSG | IDX_IN | IDX_OUT), 2) == _lib.FLC_ERR_WORKSPACE
    assert call(which, marina_rows(), Map([3, 3], IDX_B), 2) == _lib.FLC_ERR_WORKSPACE


@pytest.mark.parametrize("which", WHICH)
def test_null_map_or_id_arrays(which):
    lib = _lib.load()
    assert call(which, diana_rows(), None, 3) == _lib.FLC_ERR_ARG
    assert b"map" in lib.flc_last_error_string()
    assert call(which, diana_rows(), Map([5, 0, 3], DIANA_BITS, h=False), 3) == _lib.FLC_ERR_ARG
    assert call(which, diana_rows(), Map([5, 0, 3], DIANA_BITS, dev=False), 3) == _lib.FLC_ERR_ARG


@pytest.mark.parametrize("which", WHICH)
def test_ids_outside_the_state(which):
    lib = _lib.load()
    assert call(which, diana_rows(), Map([5, N_TOTAL, 3], DIANA_BITS), 3) == _lib.FLC_ERR_ARG
    assert b"outside" in lib.flc_last_error_string()
    assert call(which, diana_rows(), Map([5, -1, 3], DIANA_BITS), 3) == _lib.FLC_ERR_ARG
    assert call(which, marina_rows(), Map([7], 0), 1) == _lib.FLC_ERR_ARG                    # also with nothing indexed
    assert call(which, diana_rows(), Map([0], DIANA_BITS, n_total=0), 1) == _lib.FLC_ERR_ARG
    assert call(which, diana_rows(), Map([0], DIANA_BITS | 32), 1) == _lib.FLC_ERR_ARG        # an unknown bit


@pytest.mark.parametrize("which", WHICH)
def test_duplicate_ids_with_an_indexed_output(which):
    lib = _lib.load()
    assert call(which, diana_rows(), Map([5, 0, 5], DIANA_BITS), 3) == _lib.FLC_ERR_ARG
    assert b"twice" in lib.flc_last_error_string()
    assert call(which, ef21_rows(), Map([1, 1], EF21_BITS), 2) == _lib.FLC_ERR_ARG


@pytest.mark.parametrize("which", WHICH)
def test_indexed_output_rows_that_overlap(which):
    r = diana_rows()
    r.ldb = r.ldin = r.ldout = D - 1
    assert call(which, r, Map([4], DIANA_BITS), 1) == _lib.FLC_ERR_ARG              # n == 1, but n_total rows
    assert call(which, r, Map([0], DIANA_BITS, n_total=1), 1) == _lib.FLC_ERR_WORKSPACE


@pytest.mark.parametrize("which", WHICH)
def test_in_place_pairs_need_the_same_bit(which):
    lib = _lib.load()
    for bits in (IDX_B | IDX_IN, IDX_B | IDX_OUT, IDX_OUT, IDX_IN | IDX_OUT, IDX_B):
        assert call(which, diana_rows(), Map([5, 0, 3], bits), 3) == _lib.FLC_ERR_ARG, bits
        assert b"in place" in lib.flc_last_error_string()
    for bits in (IDX_B | IDX_BASE, IDX_MSG, IDX_B | IDX_MSG, IDX_BASE | IDX_MSG):
        assert call(which, ef21_rows(), Map([5, 0, 3], bits), 3) == _lib.FLC_ERR_ARG, bits


@pytest.mark.parametrize("which", WHICH)
def test_a_shared_base_is_never_indexed(which):
    lib = _lib.load()
    assert call(which, marina_rows(), Map([5, 0, 3], IDX_BASE), 3) == _lib.FLC_ERR_ARG
    assert b"shared base" in lib.flc_last_error_string()


def test_sampled_randk_takes_no_counts():
    lib = _lib.load()
    pat = _lib.FlcPattern()
    pat.d_randk_counts = OTHER
    assert call("randk", diana_rows(), Map([5, 0, 3], DIANA_BITS), 3, pat=pat) == _lib.FLC_ERR_ARG
    assert b"d_randk_counts" in lib.flc_last_error_string()


def test_sibling_checks_apply_unchanged():
    lib = _lib.load()
    mp = Map([5, 0, 3], DIANA_BITS)
    for codec in (_lib.FLC_IDENT, _lib.FLC_NATURAL, _lib.FLC_TOPK, 99):
        assert call("randk", diana_rows(), mp, 3, prm=params(codec)) == _lib.FLC_ERR_UNSUPPORTED
        assert lib.flc_randk_shift_reduce_sampled_workspace_size(ctypes.byref(params(codec)), None, 3, D) == 0
    for codec in (_lib.FLC_IDENT, _lib.FLC_RANDK, 99):
        assert call("topk", diana_rows(), mp, 3, prm=params(codec)) == _lib.FLC_ERR_UNSUPPORTED
        assert lib.flc_topk_shift_reduce_sampled_workspace_size(ctypes.byref(params(codec)), 3, D) == 0
    assert call("general", diana_rows(), mp, 3, prm=params(99)) == _lib.FLC_ERR_UNSUPPORTED
    for which in ("randk", "topk"):
        assert call(which, diana_rows(), mp, 3, prm=params(ENTRY_CODEC[which], k=0)) == _lib.FLC_ERR_ARG       # K < 1
        assert call(which, diana_rows(), mp, 3, prm=params(ENTRY_CODEC[which], k=D + 1)) == _lib.FLC_ERR_ARG   # K > d
        r = diana_rows()
        r.d_shift_out = OTHER                                # a shift that is not in place: no sparse shape
        assert call(which, r, Map([5, 0, 3], IDX_B | IDX_IN), 3) == _lib.FLC_ERR_UNSUPPORTED
        r = diana_rows()
        r.msg_scale = -1.0
        assert call(which, r, mp, 3) == _lib.FLC_ERR_UNSUPPORTED
    r = diana_rows()
    r.d_shift_in = None                                      # shift_out without shift_in
    assert call("general", r, mp, 3) == _lib.FLC_ERR_ARG
    r = _lib.FlcShiftRows()                                  # a stored message over the shared base
    r.d_a, r.lda, r.d_b, r.ldb, r.msg_scale = A, D, B, D, 1.0
    r.d_base, r.ldbase, r.d_msg, r.ldmsg = BASE, 0, BASE, D
    assert call("general", r, Map([5, 0, 3], IDX_MSG), 3) == _lib.FLC_ERR_ARG
    assert call("general", diana_rows(), mp, 3, out=None) == _lib.FLC_ERR_ARG


def test_workspace_sizes():
    lib = _lib.load()
    n, d = 5, 100003
    g, gs = lib.flc_encode_shift_reduce_workspace_size, lib.flc_encode_shift_reduce_sampled_workspace_size
    for codec in (_lib.FLC_IDENT, _lib.FLC_NATURAL, _lib.FLC_STD_DITHERING, _lib.FLC_RANDK, _lib.FLC_TOPK):
        prm = params(codec, k=2001)
        assert gs(ctypes.byref(prm), n, d) == g(ctypes.byref(prm), n, d)       # the ids are the caller's
    prm = params(_lib.FLC_RANDK, k=3000)
    for compat in (False, True):
        pat = _lib.FlcPattern()
        pat.d_randk_idx = OTHER if compat else None
        base = lib.flc_randk_shift_reduce_workspace_size(ctypes.byref(prm), ctypes.byref(pat), n, d)
        need = lib.flc_randk_shift_reduce_sampled_workspace_size(ctypes.byref(prm), ctypes.byref(pat), n, d)
        assert base < need <= base + 512 + 8 * n                               # + the pointer table of shape B's fold
        assert call("randk", diana_rows(d), Map([5, 0, 3, 1, 6], DIANA_BITS), n, d, prm=prm, pat=pat,
                    ws_bytes=need - 1) == _lib.FLC_ERR_WORKSPACE
        assert b"workspace" in lib.flc_last_error_string()
    prm = params(_lib.FLC_TOPK, k=2001)
    base = lib.flc_topk_shift_reduce_workspace_size(ctypes.byref(prm), n, d)
    need = lib.flc_topk_shift_reduce_sampled_workspace_size(ctypes.byref(prm), n, d)
    assert base < need <= base + 512 + 8 * n
    assert call("topk", diana_rows(d), Map([5, 0, 3, 1, 6], DIANA_BITS), n, d, prm=prm, ws_bytes=need - 1) == _lib.FLC_ERR_WORKSPACE


def test_harness_refuses_resident_mode_outside_its_algorithms():
    """Simulation(resident=True) is diana / ef21 / cofig without the wire modes: anything else is a
    ValueError before anything touches a device."""
    from tests import harness_cases
    for name in harness_cases.RUN_NAMES:
        algo = harness_cases.META[name]["algorithm"]
        if algo in ("dcgd", "fedavg", "marina"):
            with pytest.raises(ValueError, match="resident"):
                harness_cases.simulation(name, "cpu", resident=True)
        elif algo in ("diana", "ef21"):
            with pytest.raises(ValueError, match="resident"):
                harness_cases.simulation(name, "cpu", resident=True, shift_wire=True)
