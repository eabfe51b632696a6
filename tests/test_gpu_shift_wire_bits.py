"""GPU parity of the bit-packed shifted steps (flc_pack_shift_bits / flc_unpack_shift_reduce_bits),
everything bit-exact against parent code: the byte-format shifted wire, flc_pack_bits of a - b, the
layout restated by tile_pack, and the fused shifted round.

Shapes: d = 1 (one lane), 2047 / 2048 / 2049 (the tile edge), 4 * 2048 + 1 (the four-tiles-per-workgroup
edge), 9 * 2048 + 5 (several workgroups, a ragged tail); n = 1, 3 (below the ring depth), 5 (one past
it), 9 (two rings plus one); B = 9, 2, 3, 4, 6, 7."""
import functools

import numpy as np
import pytest
import torch

from tests.harness_cases import DATA, META
from tests.test_wire_bits_host import tile_pack, width

pytestmark = pytest.mark.gpu

SPECS = ["natural", "terngrad", "qsgd:3", "qsgd:7", "qsgd:31", "qsgd:63"]
DS = [1, 2047, 2048, 2049, 4 * 2048 + 1, 9 * 2048 + 5]
FOLDS = [(1, 1, 0), (3, 2047, 0), (5, 2048, 0), (9, 2049, 0), (5, 4 * 2048 + 1, 0), (9, 9 * 2048 + 5, 0), (3, 2049, 1)]
SEED, CLIENT0, ALPHA, SCALE = 2024, 3, 0.75, 0.25


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def i32(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def rows(n, d, off=0):
    """a, b, base [n, d] and one shared [d] vector on the device, read-only and shared by the tests.
    a - b holds +0 (every 7th column from 7 on), -0 (column 1), the power of two 2.0 (column 2, a level
    of `natural`) and the row's largest magnitude (column 3: the top level under terngrad's inf norm);
    with d == 1 the lone element is the top level of every norm.  off = 1: every tensor starts one
    float past a 16-byte boundary (the element path)."""
    g = torch.Generator().manual_seed(1000 * n + d)
    a = torch.randn(n, d, generator=g) * 4
    b = a + torch.randn(n, d, generator=g)
    b[:, 7::7] = a[:, 7::7]
    if d > 3:
        a[:, 1], b[:, 1] = -0.0, 0.0
        a[:, 2], b[:, 2] = 3.0, 1.0
        a[:, 3], b[:, 3] = 1000.0, 0.0

    def dev(t):
        buf = torch.empty(t.numel() + off, device="cuda")
        buf[off:].copy_(t.reshape(-1))
        return buf[off:].view(t.shape)
    return dev(a), dev(b), dev(torch.randn(n, d, generator=g)), dev(torch.randn(d, generator=g))


def comp(ag, spec, d, i=0, compat=False):
    """Client CLIENT0 + i's compressor: device draws, or a generated pattern (the numpy stream)."""
    c = ag.initCompressor(spec, d)
    if compat:
        c.generateCompressPattern(np.random.RandomState(SEED + i), "cuda", 0, {})
    else:
        c.device_rng = (SEED, CLIENT0 + i)
    return c


# ---- client ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,off", [(d, 0) for d in DS] + [(4 * 2048 + 1, 1)])
@pytest.mark.parametrize("spec", SPECS)
def test_pack_shift_bits(ag, spec, d, off):
    ta, tb, _, _ = rows(1, d, off)
    a, b = ta[0], tb[0]
    for compat in (False, True):
        def new():
            return comp(ag, spec, d, compat=compat)
        want = new().compressPayload(a - b, bits=True)
        # MARINA: the payload only
        pl, msg, h = new().compressShiftPayload(a, b, bits=True)
        assert msg is None and h is None and torch.equal(pl, want), (spec, d, compat)
        byte_pl = new().compressShiftPayload(a, b)[0]
        if spec != "natural":                       # Q8's codes with the sign bit moved, in the tile layout
            c8 = byte_pl[16:16 + d].cpu().numpy().astype(np.uint32)
            wb = width(new())
            assert np.array_equal(pl[16:].cpu().numpy().view(np.uint32), tile_pack((c8 & 0x7F) | ((c8 >> 7) << (wb - 1)), wb))
        assert torch.equal(i32(new().decompressShiftPayload(pl, d, bits=True)), i32(new().decompressShiftPayload(byte_pl, d)))
        # DIANA in place: shift_out is shift is b
        hb, hq = b.clone(), b.clone()
        pl, _, h = new().compressShiftPayload(a, hb, alpha=ALPHA, shift=hb, shift_out=hb, bits=True)
        new().compressShiftPayload(a, hq, alpha=ALPHA, shift=hq, shift_out=hq)
        assert h.data_ptr() == hb.data_ptr() and torch.equal(pl, want) and torch.equal(i32(hb), i32(hq)), (spec, d, compat)
        # EF21: base is b, a message, scale != 1 — out of place and in place (out is b)
        pl, m, _ = new().compressShiftPayload(a, b, scale=SCALE, base=b, message=True, bits=True)
        mq = new().compressShiftPayload(a, b, scale=SCALE, base=b, message=True)[1]
        assert torch.equal(pl, want) and torch.equal(i32(m), i32(mq)), (spec, d, compat)
        gb = b.clone()
        pl, m, _ = new().compressShiftPayload(a, gb, scale=SCALE, base=gb, out=gb, bits=True)
        assert torch.equal(pl, want) and torch.equal(i32(gb), i32(mq)), (spec, d, compat)


def test_pack_shift_bits_aligned_and_element_paths_agree(ag):
    d = 4 * 2048 + 1
    for spec in ("natural", "qsgd:7"):
        pls = [comp(ag, spec, d).compressShiftPayload(*(t[0] for t in rows(1, d, off)[:2]), bits=True)[0] for off in (0, 1)]
        assert torch.equal(rows(1, d, 0)[0], rows(1, d, 1)[0]) and torch.equal(*pls)


# ---- server ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,off", FOLDS)
@pytest.mark.parametrize("spec", SPECS)
def test_unpack_shift_reduce_bits(ag, spec, n, d, off):
    ta, tb, tbase, tg = rows(n, d, off)
    cs = [comp(ag, spec, d, i) for i in range(n)]
    packed = {}
    for bits in (False, True):
        pls = [comp(ag, spec, d, i).compressShiftPayload(ta[i], tb[i], bits=bits)[0] for i in range(n)]
        mat = torch.zeros((n, pls[0].numel() + 32), dtype=torch.uint8, device="cuda")     # ld_bytes above the payload
        mat[:, :pls[0].numel()] = torch.stack(pls)
        packed[bits] = (pls, mat[:, :pls[0].numel()])
    ref, red = ag.ShiftPayloadReducer(cs[0]), ag.ShiftPayloadReducer(cs[0], bits=True)
    weights = list(np.random.default_rng(n).uniform(0.5, 2.0, n))
    # (base, msg_out): none; per-row base with msg_out absent / separate / the base itself; shared [D] base
    shapes = [(None, None), ("rows", None), ("rows", "new"), ("rows", "base"), ("shared", None), ("shared", "new")]
    for (base, msg), w, src in [(s, w, k) for s in shapes for w in (None, weights) for k in (0, 1)]:
        got = []
        for r, bits in ((ref, False), (red, True)):
            bs = None if base is None else (tg if base == "shared" else tbase.clone())
            ms = None if msg is None else (bs if msg == "base" else torch.zeros_like(ta))
            out = r(packed[bits][src], d, scale=SCALE, base=bs, msg_out=ms, weights=w)
            got.append((out, ms))
        tag = (spec, n, d, base, msg, w is not None, src)
        assert torch.equal(i32(got[0][0]), i32(got[1][0])), tag
        if msg is not None:
            assert torch.equal(i32(got[0][1]), i32(got[1][1])), tag


@pytest.mark.parametrize("shape", ["diana", "ef21", "marina"])
@pytest.mark.parametrize("spec", ["natural", "qsgd:7"])
def test_bit_packs_then_bit_fold_equal_the_fused_round(ag, spec, shape):
    n, d = 5, 4 * 2048 + 1
    ta, tb, _, tg = rows(n, d)
    kw = {"diana": {}, "ef21": {"scale": SCALE, "base": tb.clone()}, "marina": {"base": tg}}[shape]
    want_msg = torch.empty_like(ta)
    want, _, _ = ag.ShiftUplinkReducer(comp(ag, spec, d), seed=SEED)(ta, tb, client0=CLIENT0, msg_out=want_msg, **kw)
    pls = [comp(ag, spec, d, i).compressShiftPayload(ta[i], tb[i], bits=True)[0] for i in range(n)]
    if shape == "ef21":
        kw["base"] = tb.clone()
    msg = kw["base"] if shape == "ef21" else torch.empty_like(ta)                # the EF21 mirror in place
    got = ag.ShiftPayloadReducer(comp(ag, spec, d))(pls, d, msg_out=msg, bits=True, **kw)
    assert torch.equal(i32(got), i32(want)) and torch.equal(i32(msg), i32(want_msg))


# ---- refusals and the round harness --------------------------------------------------------------------
def test_refusals(ag):
    x = torch.ones(4096, device="cuda")
    for spec in ("qsgd:127", "topk:1%", "rank_k:2"):
        c = ag.initCompressor(spec, 4096)
        with pytest.raises(NotImplementedError):
            c.compressShiftPayload(x, x * 0.5, bits=True)
        with pytest.raises(NotImplementedError):
            c.decompressShiftPayload(torch.zeros(8192, dtype=torch.uint8, device="cuda"), 4096, bits=True)
        with pytest.raises(NotImplementedError):
            ag.ShiftPayloadReducer(c, bits=True)
    red = ag.ShiftPayloadReducer(ag.initCompressor("qsgd:7", 4096), bits=True)
    with pytest.raises(ValueError):
        red([], 4096, sparse=True)
    with pytest.raises(ValueError):
        red([], 4096, clients=[])
    out = torch.full((4096,), 7.0, device="cuda")
    assert red([], 4096, out=out) is out and not out.any()                       # n == 0 stores zeros


@pytest.mark.parametrize("algorithm", ["diana", "ef21", "marina"])
def test_harness_shift_wire_bits_same_round(ag, algorithm):
    from flpytorch_amd import harness
    name = next(k for k in sorted(META) if META[k]["algorithm"] == algorithm)
    m = META[name]
    runs = []
    for kw in ({}, {"wire_bits": True}):
        model = harness.DenseModel(DATA["data_A"], DATA["data_B"], m["samples_per_client"])
        sim = harness.Simulation(algorithm, "qsgd:7", model, DATA[f"{name}_x0"], m["num_clients"],
                                 m["clients_per_round"], 3, m["local_lr"], m["global_lr"], local_iters=m["local_iters"],
                                 runtime_seed=m["manual_runtime_seed"], device="cuda", record_iterates=True,
                                 shift_wire="socket", **kw)
        H = sim.run()
        sent = sum(st["client_state"]["stats"].get("payload_bytes", 0)
                   for r in H["history"].values() for st in r["client_states"].values())
        runs.append((sim.iterates, sent))
    assert len(runs[0][0]) == len(runs[1][0]) > 0
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x.numpy().view(np.uint32), y.numpy().view(np.uint32))
    assert 0 < runs[1][1] < runs[0][1]
