"""GPU parity of the sparse shifted-wire fold (ShiftPayloadReducer(..., sparse=True),
flc_unpack_shift_reduce_sparse) against a plain numpy fp32 restatement: the entries decoded from the
payload bytes, m[idx] = base[idx] + val * scale, the sequential fold with the first term assigned and
one division.  Every comparison is of int32 views: bit equality, no tolerance."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_shift_wire import ef21_mult, inputs, reference_round, row_comp

pytestmark = pytest.mark.gpu

BURST = (3, 12288 + 4)       # topk:600 with every large difference inside tile 1: > 256 entries in one tile
CASES = [(s, n, d) for s in ("topk:1%", "topk:5", "randk:1%") for n, d in ((1, 7), (5, 4099), (9, 300001))]
CASES.append(("topk:600", *BURST))


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


@functools.lru_cache(maxsize=None)
def case(spec, n, d):
    """Rows a, b (b is the EF21 mirror), the shared base, the payloads, their compressors.  inputs()'s +0 and
    -0 difference columns; row 1 has a == b (count == 0); mirror row 0 holds a -0 at the unlisted column 0."""
    from flpytorch_amd import aggregation as ag
    a, b, _, gp = inputs(n, d)
    a, b = a.copy(), b.copy()
    if (n, d) == BURST:
        a[:, :4096], a[:, 8192:] = b[:, :4096], b[:, 8192:]
        a[:, 4096:8192] *= 100.0
    elif d > 4096:
        a[:, 4095:4097] = b[:, 4095:4097] + 1e6            # entries on both sides of the tile boundary
    if n > 1:
        a[1] = b[1]
    a[0, 0] = b[0, 0] = -0.0                                # -0 - -0 = +0: not listed
    ta, tb, tg = (torch.from_numpy(v).cuda() for v in (a, b, gp.copy()))
    comps = [row_comp(ag, spec, d, "compat", i) for i in range(n)]
    pls = [comps[i].compressShiftPayload(ta[i], tb[i])[0] for i in range(n)]
    return ta, tb, tg, comps, pls


def decoded(pl, K, d):
    raw = pl.cpu().numpy()
    cnt, off = int(raw[:16].view(np.uint32)[1]), 16 + (4 * max(1, min(K, d)) + 15) // 16 * 16
    return raw[16:16 + 4 * cnt].view(np.uint32).astype(np.int64), raw[off:off + 4 * cnt].view(np.float32)


def restated(pls, K, d, scale, mirror, shared, weights):
    scale, acc, rows = np.float32(scale), None, []
    for i, pl in enumerate(pls):
        idx, val = decoded(pl, K, d)
        if mirror is not None:
            m = mirror[i].copy()
            m[idx] = mirror[i][idx] + val * scale
        else:
            t = np.zeros(d, dtype=np.float32) * scale
            t[idx] = val * scale
            m = t if shared is None else shared + t
        rows.append(m)
        wm = m if weights is None else np.float32(weights[i]) * m
        acc = wm if i == 0 else acc + wm
    total = float(len(pls)) if weights is None else sum(weights[1:], weights[0])
    return acc / np.float32(total), rows


def bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).reshape(-1).view(np.int32)


@pytest.mark.parametrize("spec,n,d", CASES)
def test_sparse_fold_equals_the_restatement(ag, spec, n, d):
    ta, tb, tg, comps, pls = case(spec, n, d)
    K, mult = comps[0].K, ef21_mult(comps[0])
    assert n == 1 or decoded(pls[1], K, d)[0].size == 0 < decoded(pls[0], K, d)[0].size
    if (n, d) == BURST:
        assert all(((i >= 4096) & (i < 8192)).sum() > 256 for i in (decoded(p, K, d)[0] for p in (pls[0], pls[2])))
    red = ag.ShiftPayloadReducer(comps[0])
    mat = torch.stack(pls)
    for weights in (None, list(np.random.default_rng(n).uniform(0.5, 2.0, n))):
        src = pls if weights is None else mat              # a pointer list, then strided rows
        # B: the EF21 mirror in place (aligned rows, then a leading dimension of 1 mod 4: the scalar path)
        for ld in (d, d + (1 - d) % 4 + 4):
            mirror = torch.zeros((n, ld), device="cuda")[:, :d]
            mirror.copy_(tb)
            got = red(src, d, scale=mult, base=mirror, msg_out=mirror, weights=weights, sparse=True)
            want, rows = restated(pls, K, d, mult, tb.cpu().numpy(), None, weights)
            assert np.array_equal(bits(got), bits(want)), (ld, weights is not None)
            assert np.array_equal(bits(mirror.contiguous()), bits(np.stack(rows)))
            general = tb.clone()
            gout = red(src, d, scale=mult, base=general, msg_out=general, weights=weights)
            dm = np.flatnonzero(bits(mirror.contiguous()) != bits(general))
            assert dm.tolist() == [0] and bits(mirror)[0] == -2 ** 31 and bits(general)[0] == 0   # the stored -0 alone
            assert set(np.flatnonzero(bits(got) != bits(gout)).tolist()) <= {0}
        # C: MARINA's shared base; D: the plain fold — the general entry's bits without condition
        for kw, shared in (({"base": tg}, tg.cpu().numpy()), ({}, None)):
            got = red(src, d, scale=0.25, weights=weights, sparse=True, **kw)
            want, _ = restated(pls, K, d, 0.25, None, shared, weights)
            assert np.array_equal(bits(got), bits(want)), (sorted(kw), weights is not None)
            assert np.array_equal(bits(got), bits(red(src, d, scale=0.25, weights=weights, **kw)))


@pytest.mark.parametrize("spec", ["topk:1%", "randk:1%"])
def test_sparse_fold_over_sampled_mirror_rows(ag, spec):
    n, d, ids = 3, 4099, [5, 0, 3]
    _, tb, _, comps, pls = case(spec, 5, d)
    red = ag.ShiftPayloadReducer(comps[0])
    state = torch.randn((7, d), device="cuda")
    state[ids] = tb[:n]
    before = state.clone()
    got = red(pls[:n], d, scale=0.5, base=state, msg_out=state, sparse=True, clients=ids)
    gathered = tb[:n].clone()
    want = red(pls[:n], d, scale=0.5, base=gathered, msg_out=gathered, sparse=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(state[ids]), bits(gathered))
    assert np.array_equal(bits(state[[1, 2, 4, 6]]), bits(before[[1, 2, 4, 6]]))


@pytest.mark.parametrize("spec,n,d", [c for c in CASES if c[1] > 1 and c[2] < 100000])
def test_sparse_fold_equals_the_device_resident_round(ag, spec, n, d):
    """Shape B against ShiftUplinkReducer's sparse siblings over the rows the payloads were packed from."""
    ta, tb, _, comps, pls = case(spec, n, d)
    mult, weights = ef21_mult(comps[0]), list(np.random.default_rng(n).uniform(0.5, 2.0, n))
    sibling = {"sparse": True} if spec.startswith("randk") else {"batched": True}
    tb2, mirror = tb.clone(), tb.clone()
    want, _ = reference_round(ag, spec, n, d, "compat", ta, tb2, weights, scale=mult, base=tb2, msg_out=tb2, **sibling)
    got = ag.ShiftPayloadReducer(comps[0])(pls, d, scale=mult, base=mirror, msg_out=mirror, weights=weights, sparse=True)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(mirror), bits(tb2))
