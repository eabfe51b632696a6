"""GPU contract of the sparse level message (flc_pack_slev / flc_unpack_slev / flc_unpack_reduce_slev).
The payload is, byte for byte, the layout of tests/test_wire_slev_host.py slev_pack applied to the
Q8 codes flc_pack gives for the same row and pattern.  The sign of zero does not travel, so decode
and fold are compared through canon(a) = bits(a + 0.0f), NaN by position: the decode against
compressVector, the fold against the Q8 fold and the sequential fp32 numpy fold of the Q8 decodes."""
import numpy as np
import pytest
import torch

from tests.test_wire_slev_host import DS, slev_pack, used_bytes, used_of

pytestmark = pytest.mark.gpu

SPECS = ["terngrad", "qsgd:127"]


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def agree(a, b):
    a, b = host(a) + np.float32(0), host(b) + np.float32(0)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def rows_for(n, d, seed):
    """N(0,1) * 10^U(-3,3) with exact zeros and -0 elements (tests/test_gpu_wire_seeded.py)."""
    g = np.random.default_rng(seed)
    r = (g.standard_normal((n, d)) * 10.0 ** g.uniform(-3, 3, (n, d))).astype(np.float32)
    r[:, ::7] = 0.0
    r[:, 3::11] = -0.0
    return r


def compressor(ag, spec, d, mode="device", client=0):
    comp = ag.initCompressor(spec, d)
    if mode == "compat":
        comp.generateCompressPattern(np.random.RandomState(11 + client), "cuda", 0, {})
    else:
        comp.device_rng = (2024, client)
    return comp


def on_gpu(x, mode="device"):
    if mode != "misaligned":
        return torch.from_numpy(x).cuda()
    buf = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x).cuda()
    return buf[1:]                                   # a view 4 bytes off the allocation's alignment


def pack_and_check(comp, xt, d):
    """The message of xt, checked against the Q8 message's codes, the validator and compressVector."""
    raw = comp.compressPayload(xt).cpu().numpy()
    dense = comp.compressVector(xt)
    keep = (host(dense).view(np.uint32) << 1) != 0
    want = slev_pack(raw[:16].view(np.uint32), raw[16:16 + d], keep)
    got = comp.compressPayload(xt, sparse_levels=True).cpu().numpy()
    assert got.size == want.size == used_of(got, d) == used_bytes(d, int(keep.sum())) <= comp.payloadBytes(d, sparse_levels=True)
    assert np.array_equal(got, want)
    comp.validatePayload(got, d, sparse_levels=True)
    assert agree(comp.decompressPayload(torch.from_numpy(got).cuda(), d, sparse_levels=True), dense)
    return got, int(keep.sum())


@pytest.mark.parametrize("spec,d,mode", [(s, d, "device") for s in SPECS for d in DS] +
                         [("qsgd:127", DS[-1], "compat"), ("qsgd:127", DS[-1], "misaligned")])
def test_payload_validate_and_decode(ag, spec, d, mode):
    comp, xt = compressor(ag, spec, d, mode), on_gpu(rows_for(1, d, d)[0], mode)
    assert mode != "misaligned" or xt.data_ptr() % 16 == 4
    got, nnz = pack_and_check(comp, xt, d)
    io = used_bytes(d, 0)
    bad = [(got, d + 1), (got[:-16], d)]
    if nnz >= 2 and got[16 + 4:16 + 8].view(np.uint32)[0] >= 2:           # two entries in chunk 0: swap them
        sw = got.copy()
        sw[io:io + 4] = got[io:io + 4].view(np.uint16)[::-1].copy().view(np.uint8)
        bad.append((sw, d))
    if nnz:                                                               # a level-0 entry under a finite norm
        z = got.copy()
        z[io + (2 * nnz + 15) // 16 * 16] &= 0x80
        bad.append((z, d))
    assert len(bad) == 4 or d == 1 or spec == "terngrad"
    for msg, dd in bad:
        with pytest.raises(ValueError):
            comp.validatePayload(msg, dd, sparse_levels=True)


def extreme_rows():
    full = np.where(np.arange(4097) % 2, -3.0, 3.0).astype(np.float32)    # |x| / norm * s = 127 / sqrt(4097) ~ 1.98
    hole = rows_for(1, 3 * 4096, 5)[0]
    hole[4096:8192] = 0.0
    nonfinite = rows_for(1, 4097, 6)[0]
    nonfinite[[5, 4096]] = [np.nan, np.inf]
    return {"full": full, "hole": hole, "zero": np.zeros(4097, np.float32), "nonfinite": nonfinite}


@pytest.mark.parametrize("case", ["full", "hole", "zero", "nonfinite"])
def test_chunk_extremes(ag, case):
    x = extreme_rows()[case]
    d = x.size
    comp = compressor(ag, "qsgd:127", d)
    got, nnz = pack_and_check(comp, on_gpu(x), d)
    tab = got[16:16 + 4 * (-(-d // 4096) + 1)].view(np.uint32)
    if case == "full":                                # a chunk with all 4096 entries; used size = capacity
        assert nnz == d and tab[1] == 4096 and got.size == comp.payloadBytes(d, sparse_levels=True)
    elif case == "hole":                              # an empty chunk between non-empty ones
        assert 0 < tab[1] == tab[2] < tab[3]
    elif case == "zero":
        assert nnz == 0
    else:                                             # NaN outputs by position: level-0 entries, accepted
        assert nnz == d and not (got[used_bytes(d, 0) + (2 * d + 15) // 16 * 16:][:d] & 0x7F).any()


def numpy_fold(dense, w):
    acc = None
    for i, row in enumerate(dense):
        t = row if w is None else (np.float32(w[i]) * row).astype(np.float32)
        acc = t if acc is None else (acc + t).astype(np.float32)
    return (acc / np.float32(len(dense) if w is None else sum(w[1:], w[0]))).astype(np.float32)


def packed_rows(ag, spec, n, d, seed):
    """n rows' Q8 payloads and sparse level messages: as a list of used views and as capacity rows."""
    rows = rows_for(n, d, seed)
    comps = [compressor(ag, spec, d, client=i) for i in range(n)]
    xs = [torch.from_numpy(rows[i]).cuda() for i in range(n)]
    q8 = torch.stack([comps[i].compressPayload(xs[i]) for i in range(n)])
    mat = torch.zeros(n, comps[0].payloadBytes(d, sparse_levels=True), dtype=torch.uint8, device="cuda")
    views = [comps[i].compressPayload(xs[i], out=mat[i], sparse_levels=True) for i in range(n)]
    return comps, q8, mat, [v.clone() for v in views]


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("n", [1, 3, 65])                  # 65: past one 64-row batch and any ring depth
@pytest.mark.parametrize("d", DS)
def test_fold_agrees_with_q8_fold_and_numpy(ag, d, n, spec):
    comps, q8, mat, msgs = packed_rows(ag, spec, n, d, 100 * n + d)
    dense = [comps[i].decompressPayload(q8[i], d).cpu().numpy() for i in range(n)]
    wr = list(np.random.default_rng(n).uniform(0.5, 2.0, n))
    wr[-1] = -wr[-1]
    red = ag.PayloadReducer(comps[0], sparse_levels=True)
    for w in (None, wr):
        q8_fold = ag.PayloadReducer(comps[0])(q8, d=d, weights=w)
        for payloads in (msgs, mat):                        # a pointer array, then strided capacity rows
            got = red(payloads, d=d, weights=w)
            assert agree(got, q8_fold)
            assert agree(got, numpy_fold(dense, w))
    with pytest.raises(ValueError):
        red(msgs, d=d, weights=[float("inf")] * n)


@pytest.mark.parametrize("spec", ["natural", "randk:1%", "topk:1%", "qsgd:255", "ident"])
def test_refusals(ag, spec):
    d = 4097
    comp = ag.initCompressor(spec, d)
    if spec == "randk:1%":
        comp.device_rng = (2024, 0)
    x = torch.ones(d, device="cuda")
    sentinel = torch.full((d,), 7.0, device="cuda")
    buf = torch.full((used_bytes(d, d),), 0xA5, dtype=torch.uint8, device="cuda")
    for call in (lambda: comp.payloadBytes(d, sparse_levels=True),
                 lambda: comp.validatePayload(bytes(64), d, sparse_levels=True),
                 lambda: comp.compressPayload(x, out=buf, sparse_levels=True),
                 lambda: comp.decompressPayload(buf, d, sparse_levels=True),
                 lambda: ag.PayloadReducer(comp, sparse_levels=True)([buf], d=d, out=sentinel)):
        with pytest.raises(NotImplementedError):
            call()
    assert (buf == 0xA5).all() and (sentinel == 7.0).all()
    for kw in ({"bits": True}, {"seeded": True}):
        with pytest.raises(ValueError):
            ag.initCompressor("qsgd:7", d).payloadBytes(d, sparse_levels=True, **kw)
        with pytest.raises(ValueError):
            ag.PayloadReducer(ag.initCompressor("qsgd:7", d), sparse_levels=True, **kw)([buf], d=d)


def test_malformed_bytes_stay_inside_the_tile(ag):
    """The decode kernels' bounds contract (as tests/test_gpu_transport.py states for the other formats):
    an index of 0xFFFF, a level index above s and a tab word past nnz are decoded and folded without
    validation; only the chunks those bytes belong to (1 and 2) differ from the clean result."""
    spec, n, d = "qsgd:5", 3, DS[-1]
    comps, _, mat, _ = packed_rows(ag, spec, n, d, 9)
    red = ag.PayloadReducer(comps[0], sparse_levels=True)
    clean_fold, clean_row = red(mat, d=d).cpu().numpy(), comps[1].decompressPayload(mat[1], d, sparse_levels=True).cpu().numpy()
    m = mat[1].cpu().numpy()
    tab = m[16:16 + 20].view(np.uint32)
    nnz, io = int(tab[4]), used_bytes(d, 0)
    assert tab[1] < tab[2] < nnz
    first = int(tab[1])                                  # chunk 1's first entry
    m[io + 2 * first:io + 2 * first + 2] = 0xFF
    m[io + (2 * nnz + 15) // 16 * 16 + first] = 0xFF
    m[16 + 8:16 + 12] = np.array([nnz + 1000], np.uint32).view(np.uint8)
    with pytest.raises(ValueError):
        comps[1].validatePayload(m, d, sparse_levels=True)
    mat[1] = torch.from_numpy(m).cuda()
    fold, row = red(mat, d=d).cpu().numpy(), comps[1].decompressPayload(mat[1], d, sparse_levels=True).cpu().numpy()
    for got, clean in ((fold, clean_fold), (row, clean_row)):
        assert np.isfinite(got).all()
        assert agree(got[:4096], clean[:4096]) and agree(got[3 * 4096:], clean[3 * 4096:])
