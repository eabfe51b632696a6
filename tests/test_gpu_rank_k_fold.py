"""GPU contract of the Rank-K fold from the factor payloads (PayloadReducer(factored=True),
flc_unpack_reduce_factored, k_rk_fold).

The reference is float64 over the factor blocks read back from the very messages and the fp32-rounded
weights, ref = sum_i w_i U'_i (SV)_i / w_total: no SVD ambiguity, the check is on the fold alone.  With
m = n K' and u = 2^-24 a term passes through at most m + 2 roundings (weight, product, m - 1 sums, the
division), so elementwise
    |got - ref| <= 1.01 (m + 4) u (sum_i |w_i| |U'_i| |(SV)_i|) / |w_total| + m 2^-126
(the last term: a flushed subnormal product)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(5, 200, 150, 2),      # edge tiles in both dimensions, B % 4 != 0
         (3, 85, 29, 3),        # odd B: unaligned U' columns, odd K', a tile wider than the matrix
         (4, 64, 64, 5),        # K' no multiple of the instruction's k
         (9, 64, 64, 1),        # K' = 1, an odd contraction, more rows than pipeline stages
         (2, 64, 64, 100),      # K clamped to K' = 64: several slabs per row
         (3, 97, 1, 4),         # B = 1, K' = 1
         (3, 320, 300, 7),      # several tiles, a partial last tile in both dimensions
         (1, 129, 130, 3)]      # n = 1, one past a tile multiple


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def low_rank(g, A, B, r, noise):
    u = g.standard_normal((A, r)) * np.linspace(3.0, 1.0, r)
    return ((u @ g.standard_normal((r, B))) + noise * g.standard_normal((A, B))).astype(np.float32).reshape(-1)


@functools.lru_cache(maxsize=None)
def packed(n, A, B, K):
    """The n messages of a case and their factors as float64: U'_i [K', B], (SV)_i [A, K']."""
    from flpytorch_amd import aggregation as ag
    g = np.random.default_rng([n, A, B, K])
    comp = ag.initCompressor(f"rank_k:{K}", A * B)
    assert (comp.A, comp.B) == (A, B)
    kp = min(K, A, B)
    uoff = (B * kp + 3) & ~3
    pays, us, svs = [], [], []
    for _ in range(n):
        p = comp.compressPayload(torch.from_numpy(low_rank(g, A, B, kp, 1e-3)).cuda())
        body = p.cpu().numpy()[16:].view(np.float32)
        us.append(body[:B * kp].reshape(kp, B).astype(np.float64))
        svs.append(body[uoff:uoff + kp * A].reshape(A, kp).astype(np.float64))
        pays.append(p)
    return comp, pays, us, svs, [float(x) for x in g.uniform(0.5, 2.0, n)]


def check_fold(ag, comp, pays, us, svs, w, A, B):
    """The factored fold of ``pays`` against float64 over the factors, under the docstring's bound."""
    n, kp = len(us), us[0].shape[0]
    w32 = np.float32(w).astype(np.float64) if w is not None else np.ones(n)
    wt = float(np.float32(sum(w))) if w is not None else float(n)      # the fp32 divisor the call passes
    ref = sum(wi * (sv @ u) for wi, u, sv in zip(w32, us, svs)) / wt
    mag = sum(abs(wi) * (np.abs(sv) @ np.abs(u)) for wi, u, sv in zip(w32, us, svs)) / abs(wt)
    m = n * kp
    bound = 1.01 * (m + 4) * 2.0 ** -24 * mag + m * 2.0 ** -126
    got = ag.PayloadReducer(comp, factored=True)(pays, A * B, weights=w).cpu().numpy().astype(np.float64).reshape(A, B)
    err = np.abs(got - ref)
    print(f"max err / bound = {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), float(np.max(err / bound))


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "plain"])
@pytest.mark.parametrize("n,A,B,K", CASES)
def test_fold_against_float64_of_the_factors(ag, n, A, B, K, weighted):
    comp, pays, us, svs, w = packed(n, A, B, K)
    check_fold(ag, comp, pays, us, svs, w if weighted else None, A, B)


@pytest.mark.parametrize("A,B", [(2100, 2000), (2051, 2001)], ids=["vector-loads", "scalar-loads"])
def test_large_tile_kernel(ag, A, B):
    """A grid of at least 256 tiles of 128 x 128 takes the large-tile kernel, which no shape up to 320 x 300
    reaches: partial tiles in both dimensions, K' = 20 in two slabs.  The messages are written here from
    drawn factors (a well-formed message: validatePayload), so no SVD of that size runs."""
    n, K = 2, 20
    g = np.random.default_rng([A, B])
    comp = ag.initCompressor(f"rank_k:{K}", A * B)
    assert (comp.A, comp.B) == (A, B)
    uoff = (B * K + 3) & ~3
    msgs = np.zeros((n, comp.payloadBytes()), np.uint8)
    us = [g.standard_normal((K, B)).astype(np.float32) for _ in range(n)]
    svs = [g.standard_normal((A, K)).astype(np.float32) for _ in range(n)]
    for i in range(n):
        msgs[i, :16].view(np.int32)[:] = (6, K, 0, 0)
        body = msgs[i, 16:].view(np.float32)
        body[:B * K], body[uoff:uoff + K * A] = us[i].ravel(), svs[i].ravel()
    comp.validatePayload(msgs[0])
    check_fold(ag, comp, torch.from_numpy(msgs).cuda(), [u.astype(np.float64) for u in us],
               [sv.astype(np.float64) for sv in svs], [0.75, 1.5], A, B)


def test_forms_and_calls_give_the_same_bits_without_a_row_workspace(ag):
    n, A, B, K = 3, 320, 300, 7
    comp, pays, _, _, w = packed(n, A, B, K)
    d = A * B
    red = ag.PayloadReducer(comp, factored=True)
    one = red(pays, d, weights=w)
    two = red(pays, d, weights=w)
    mat = red(torch.stack(pays), d, weights=w)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    assert torch.equal(one.view(torch.int32), mat.view(torch.int32))
    from flpytorch_amd import _lib
    prm, _ = comp.codec_params(one.device)
    assert _lib.load().flc_unpack_reduce_factored_workspace_size(ctypes.byref(prm), n, d) < 4 * d


def test_refusals_and_no_rows(ag):
    d = 64 * 64
    with pytest.raises(NotImplementedError):
        ag.PayloadReducer(ag.initCompressor("topk:1%", d), factored=True)
    comp = ag.initCompressor("rank_k:3", d)
    with pytest.raises(ValueError):
        ag.PayloadReducer(comp, factored=True, bits=True)
    out = torch.full((d,), float("nan"), device="cuda")
    got = ag.PayloadReducer(comp, factored=True)([], d, out=out)
    assert torch.count_nonzero(got).item() == 0
