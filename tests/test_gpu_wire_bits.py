"""GPU contract of the bit-packed wire formats (flc_pack_bits / flc_unpack_bits / flc_unpack_reduce_bits),
each bit-exact: the payload is the tile layout (tests/test_wire_bits_host.py tile_pack) of the codes
flc_pack gives for the same row and pattern; the decode equals the byte format's decode; the server
fold equals the byte-format fold and the sequential fp32 numpy fold of the decoded rows."""
import numpy as np
import pytest
import torch

from tests.harness_cases import simulation
from tests.test_wire_bits_host import DS, SPECS, tile_pack, width

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def bits(a):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).view(np.uint32)


def rows_for(n, d, seed):
    """N(0,1) * 10^U(-3,3) with exact zeros and negative elements far below the first level (-0 * norm)."""
    g = np.random.default_rng(seed)
    r = (g.standard_normal((n, d)) * 10.0 ** g.uniform(-3, 3, (n, d))).astype(np.float32)
    r[:, ::7] = 0.0
    r[:, 3::11] = -1e-30
    return r


def compressor(ag, spec, d, mode="device", client=0):
    comp = ag.initCompressor(spec, d)
    if mode == "compat":
        comp.generateCompressPattern(np.random.RandomState(11 + client), "cuda", 0, {})
    else:
        comp.device_rng = (2024, client)
    return comp


def on_gpu(x, mode):
    if mode != "misaligned":
        return torch.from_numpy(x).cuda()
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda()
    return buf[1:]                                   # a view 4 bytes off the allocation's alignment


PACK_CASES = ([(s, d, "device") for s in SPECS for d in DS] + [("qsgd:7", d, "compat") for d in DS] +
              [("qsgd:15", DS[-1], "misaligned"), ("natural", 2049, "misaligned")])


@pytest.mark.parametrize("spec,d,mode", PACK_CASES)
def test_pack_bytes_and_unpack_bits(ag, spec, d, mode):
    comp, xt = compressor(ag, spec, d, mode), on_gpu(rows_for(1, d, d)[0], mode)
    assert mode != "misaligned" or xt.data_ptr() % 16 == 4
    b = width(comp)
    byte_pl = comp.compressPayload(xt)
    dense = comp.decompressPayload(byte_pl, d)
    got = comp.compressPayload(xt, bits=True).cpu().numpy()
    raw = byte_pl.cpu().numpy()
    if spec == "natural":
        codes, word = bits(dense) >> 23, 8
    else:
        c = raw[16:16 + d].astype(np.uint32)
        codes, word = (c & 0x7F) | ((c >> 7) << (b - 1)), 7 | (b << 8)
        assert ((c == 0x80).any() and (c == 0).any()) or d < 64        # the -0 * norm code and the +0 code occur
    head = raw[:16].view(np.uint32).copy()
    assert head[3] == 0
    head[0] = word
    want = np.concatenate([head, tile_pack(codes, b)]).view(np.uint8)
    assert got.size == want.size == comp.payloadBytes(d, bits=True)
    assert np.array_equal(got, want)
    back = comp.decompressPayload(torch.from_numpy(got).cuda(), d, bits=True)
    assert np.array_equal(bits(back), bits(dense))


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("n", [1, 3, 9])             # below the ring, not a multiple of it, past two rings
@pytest.mark.parametrize("d", [2049, 3 * 2048 + 77])
def test_fold_equals_byte_fold_and_numpy(ag, spec, n, d):
    rows = rows_for(n, d, 100 * n + d)
    comps = [compressor(ag, spec, d, client=i) for i in range(n)]
    xs = [torch.from_numpy(rows[i]).cuda() for i in range(n)]
    byte_pls = [comps[i].compressPayload(xs[i]) for i in range(n)]
    bit_pls = [comps[i].compressPayload(xs[i], bits=True) for i in range(n)]
    dense = [comps[i].decompressPayload(byte_pls[i], d).cpu().numpy() for i in range(n)]
    for w in (None, list(np.random.default_rng(n).uniform(0.5, 2.0, n))):
        acc = None
        for i in range(n):
            t = dense[i] if w is None else (np.float32(w[i]) * dense[i]).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
        want = (acc / np.float32(n if w is None else sum(w[1:], w[0]))).astype(np.float32)
        byte_fold = ag.PayloadReducer(comps[0])(torch.stack(byte_pls), d=d, weights=w)
        red = ag.PayloadReducer(comps[0], bits=True)
        for payloads in (torch.stack(bit_pls), bit_pls):                # strided rows, then a pointer array
            got = red(payloads, d=d, weights=w)
            assert np.array_equal(bits(got), bits(byte_fold))
            assert np.array_equal(bits(got), bits(want))


def test_natural_unrepresentable_elements_are_counted(ag):
    d = 2049
    x = rows_for(1, d, 5)[0]
    x[10], x[2047] = 1e-40, np.nan                   # a subnormal power of two and a NaN on the way out
    comp, xt = compressor(ag, "natural", d), torch.from_numpy(x).cuda()
    pl = comp.compressPayload(xt, bits=True)
    assert pl[:16].cpu().numpy().view(np.uint32)[3] == 2
    want, got = bits(comp.compressVector(xt)), bits(comp.decompressPayload(pl, d, bits=True))
    keep = np.ones(d, bool)
    keep[[10, 2047]] = False
    assert np.array_equal(got[keep], want[keep])
    with pytest.raises(ValueError, match="2 elements flagged"):
        comp.validatePayload(pl.cpu(), d, bits=True)


def test_level_index_above_s_reads_the_top_level(ag):
    d = 2049
    comp, xt = compressor(ag, "qsgd:10", d), torch.from_numpy(rows_for(1, d, 6)[0]).cuda()     # b = 5: indices to 15
    byte_pl, bit_pl = comp.compressPayload(xt), comp.compressPayload(xt, bits=True)
    byte_pl[16] = 15
    word = bit_pl[16:20].cpu().numpy().view(np.uint32)
    bit_pl[16:20] = torch.from_numpy(((word & ~np.uint32(31)) | np.uint32(15)).view(np.uint8)).cuda()
    got = bits(comp.decompressPayload(bit_pl, d, bits=True))
    assert np.array_equal(got, bits(comp.decompressPayload(byte_pl, d)))
    assert got[0] == bits(comp.levelsValues[-1:].cuda() * byte_pl[8:12].view(torch.float32))[0]
    with pytest.raises(ValueError, match="exceeds s=10"):
        comp.validatePayload(bit_pl.cpu(), d, bits=True)


@pytest.mark.parametrize("spec", ["qsgd:127", "qsgd:255", "randk:1%", "topk:1%", "ident"])
def test_codecs_without_a_bit_packed_form_are_refused(ag, spec):
    d = 4099
    comp = ag.initCompressor(spec, d)
    out = torch.full((8192,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError):
        comp.compressPayload(torch.ones(d, device="cuda"), out=out, bits=True)
    with pytest.raises(NotImplementedError):
        comp.decompressPayload(out, d, bits=True)
    with pytest.raises(NotImplementedError):
        ag.PayloadReducer(comp, bits=True)(out.reshape(2, 4096), d=d)
    assert bool((out == 0xA5).all())


def test_harness_wire_bits_same_run(ag):
    """DCGD with qsgd:10: the bit-packed messages (5 bits per element) give the byte-format run, bit for bit."""
    runs = []
    for kw in ({}, {"wire_bits": True}):
        sim = simulation("dcgd_qsgd10", "cuda", record_iterates=True, wire=True, **kw)
        runs.append((sim.run()["history"], sim.iterates))
    (hb, xb), (hw, xw) = runs
    assert len(xb) == len(xw) > 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(xb, xw))
    for rb, rw in ((hb[r], hw[r]) for r in hb):
        assert all(rb[k] == rw[k] for k in ("grad_sgd_server_l2", "x_before_round", "approximate_f_avg_value"))
        for c, st in rw["client_states"].items():
            sent, ref = st["client_state"]["stats"], rb["client_states"][c]["client_state"]["stats"]
            assert sent["send_scalars_to_master"] == ref["send_scalars_to_master"]
            # whole bit-packed messages were shipped: D = 2465 is two tiles of 256 * 5 bytes
            assert sent["payload_bytes"] > 0 and sent["payload_bytes"] % (16 + 2 * 256 * 5) == 0
            assert ref["payload_bytes"] % (16 + 2480) == 0
