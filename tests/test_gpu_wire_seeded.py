"""GPU contract of the seeded RandK message (flc_pack_seeded / flc_unpack_seeded / flc_unpack_reduce_seeded),
each bit-exact: the payload is the two 16-byte blocks and the kept values in the sampler's order
(oracle.devrng.randk_indices); the decode equals compressVector; the server fold equals the FMT_SPARSE
fold of the same rows and the sequential fp32 numpy fold of the decoded rows."""
import numpy as np
import pytest
import torch

from oracle import devrng

pytestmark = pytest.mark.gpu

SEED = 2024
DS = [4095, 4097, 3 * 4096 + 77]      # one short chunk; a last chunk of length 1; several chunks and a ragged end
KS = ["1", "1%", "50%", "100%"]       # one value; sparse; chunks with more than 64 members; every chunk full


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def bits(a):
    return (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).view(np.uint32)


def rows_for(n, d, seed):
    """N(0,1) * 10^U(-3,3) with exact zeros and -0 elements (+-0 values, -0 columns)."""
    g = np.random.default_rng(seed)
    r = (g.standard_normal((n, d)) * 10.0 ** g.uniform(-3, 3, (n, d))).astype(np.float32)
    r[:, ::7] = 0.0
    r[:, 3::11] = -0.0
    return r


def compressor(ag, k, d, client=0):
    comp = ag.initCompressor("randk:" + k, d)
    comp.device_rng = (SEED, client)
    return comp


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
def test_payload_bytes_validate_and_decode(ag, d, k):
    client = 5
    comp, x = compressor(ag, k, d, client), rows_for(1, d, d)[0]
    xt = torch.from_numpy(x).cuda()
    K, key = comp.K, int(devrng.client_key(SEED, client))
    got = comp.compressPayload(xt, seeded=True).cpu().numpy()
    vals = (np.float32(d / K) * x[devrng.randk_indices(SEED, client, d, K)]).astype(np.float32)
    head = np.array([9, K, 0, 0, key & 0xFFFFFFFF, key >> 32, d, 0], dtype=np.uint32)
    want = np.concatenate([head.view(np.uint8), vals.view(np.uint8), np.zeros(-4 * K % 16, np.uint8)])
    assert got.size == want.size == comp.payloadBytes(d, seeded=True) == 32 + (4 * K + 15) // 16 * 16
    assert np.array_equal(got, want)
    comp.validatePayload(got, d, seeded=True, client=client)
    comp.validatePayload(got, d, seeded=True)
    flipped = got.copy()
    flipped[4] ^= 1                                        # count
    for bad, kw in ((got, {"client": client + 1}), (got, {"d": d + 1}), (flipped, {}), (got[:-16], {})):
        with pytest.raises(ValueError):
            comp.validatePayload(bad, kw.get("d", d), seeded=True, client=kw.get("client"))
    back = comp.decompressPayload(torch.from_numpy(got).cuda(), d, seeded=True)
    dense = comp.compressVector(xt)
    assert np.array_equal(bits(back), bits(dense))
    assert K < 64 or (bits(back) == 0x80000000).any()      # -0 values travel


def numpy_fold(dense, w):
    acc = None
    for i, row in enumerate(dense):
        t = row if w is None else (np.float32(w[i]) * row).astype(np.float32)
        acc = t if acc is None else (acc + t).astype(np.float32)
    return (acc / np.float32(len(dense) if w is None else sum(w[1:], w[0]))).astype(np.float32)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [1, 3, 65])                  # 65: past one 64-row batch
@pytest.mark.parametrize("d", DS)
def test_fold_equals_sparse_fold_and_numpy(ag, d, n, k):
    """n = 1, K = 1 % is also the case in which a lane of the -0 resolution lists no entry of the row
    (fewer than 64 entries in a chunk) and must still see the kept-column words the other lanes set."""
    rows = rows_for(n, d, 100 * n + d)
    comps = [compressor(ag, k, d, client=i) for i in range(n)]
    xs = [torch.from_numpy(rows[i]).cuda() for i in range(n)]
    sparse_pls = [comps[i].compressPayload(xs[i]) for i in range(n)]
    seeded_pls = [comps[i].compressPayload(xs[i], seeded=True) for i in range(n)]
    dense = [comps[i].decompressPayload(sparse_pls[i], d).cpu().numpy() for i in range(n)]
    wr = list(np.random.default_rng(n).uniform(0.5, 2.0, n))
    wr[-1] = -wr[-1]                                       # the -0 rule's sign branch
    red = ag.PayloadReducer(comps[0], seeded=True)
    for w in (None, wr):
        want = numpy_fold(dense, w)
        sparse_fold = ag.PayloadReducer(comps[0])(torch.stack(sparse_pls), d=d, weights=w)
        for payloads in (torch.stack(seeded_pls), seeded_pls):           # strided rows, then a pointer array
            got = red(payloads, d=d, weights=w)
            assert np.array_equal(bits(got), bits(sparse_fold))
            assert np.array_equal(bits(got), bits(want))


def test_message_drawn_for_another_d_contributes_nothing(ag):
    """Bounds on what the kernels take from a message: a draw block naming 2 d makes the row the +0 row."""
    n, d = 3, DS[-1]
    rows = rows_for(n, d, 7)
    comps = [compressor(ag, "1%", d, client=i) for i in range(n)]
    pls = torch.stack([comps[i].compressPayload(torch.from_numpy(rows[i]).cuda(), seeded=True) for i in range(n)])
    dense = [comps[i].decompressPayload(pls[i], d, seeded=True).cpu().numpy() for i in range(n)]
    pls[1, 24:28] = torch.from_numpy(np.array([2 * d], np.uint32).view(np.uint8)).cuda()
    dense[1] = np.zeros(d, np.float32)
    with pytest.raises(ValueError, match="drawn for d="):
        comps[1].validatePayload(pls[1].cpu(), d, seeded=True)
    assert np.array_equal(bits(comps[1].decompressPayload(pls[1], d, seeded=True)), bits(dense[1]))
    got = ag.PayloadReducer(comps[0], seeded=True)(pls, d=d)
    assert np.array_equal(bits(got), bits(numpy_fold(dense, None)))


@pytest.mark.parametrize("spec", ["randk:1%", "topk:1%", "qsgd:7", "ident"])
def test_codecs_without_a_seeded_form_are_refused(ag, spec):
    d = 4099
    comp = ag.initCompressor(spec, d)                      # randk without device_rng: the compat stream
    if spec.startswith("randk"):
        comp.generateCompressPattern(np.random.RandomState(11), "cuda", 0, {})
    elif spec != "ident":
        comp.device_rng = (SEED, 0)
    out = torch.full((8192,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(NotImplementedError):
        comp.payloadBytes(d, seeded=True)
    with pytest.raises(NotImplementedError):
        comp.compressPayload(torch.ones(d, device="cuda"), out=out, seeded=True)
    with pytest.raises(NotImplementedError):
        comp.decompressPayload(out, d, seeded=True)
    with pytest.raises(NotImplementedError):
        ag.PayloadReducer(comp, seeded=True)(out.reshape(2, 4096), d=d)
    assert bool((out == 0xA5).all())
    with pytest.raises(ValueError):
        compressor(ag, "1%", d).compressPayload(torch.ones(d, device="cuda"), out=out, seeded=True, bits=True)
    assert bool((out == 0xA5).all())
