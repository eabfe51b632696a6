"""The many-row TopK filter's workgroup items (k_topk_filter_fast_wg, launched as k_topk_filter_g4):
an item is 4 consecutive 4-chunk groups (16 chunks) of one row, staged by four loader waves and
reserved, tabbed and copied out by a writer wave.  Every case is K = 1 % through UplinkReducer,
plain and weighted, bit-exact against the oracle; the launch profiler shows the 4-chunk filter ran
and the path flags (1 = list overflow, 8 = exact path) show which rows left the fast path."""
import math

import numpy as np
import pytest
import torch

from oracle import codecs as oc
from tests.test_gpu_parity import _FilterVariants, _topk_enc, _topk_rows, assert_bitexact

pytestmark = pytest.mark.gpu

GROUP = 4 * 4096            # elements of a 4-chunk group (one loader wave's share of an item)
GCAP = 512                  # staged entries a group holds


@pytest.fixture(scope="module")
def ag():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from flpytorch_amd import aggregation
    return aggregation


def _run(ag, rows, spec, g, row_groups=None):
    """One plain and one weighted uplink of rows; returns the path flags of the plain call."""
    n, d = rows.shape
    k = math.ceil(0.01 * d)
    enc = _topk_enc(rows, k)
    comp = ag.initCompressor(spec, d)
    assert comp.K == k
    if row_groups:
        comp.row_groups = row_groups
    red = ag.UplinkReducer(comp)
    rt = torch.from_numpy(rows).cuda()
    with _FilterVariants() as fv:
        got = red(rt)
    assert fv.g4 >= 1 and fv.g2 == 0, f"filter variants g4={fv.g4} g2={fv.g2}: not the workgroup-item path"
    assert_bitexact(got, oc.reduce_plain(enc))
    fl = np.asarray(ag.select_row_flags(red.comp, n, d))
    w = [float(v) for v in g.uniform(0.5, 2.0, n)]
    with _FilterVariants() as fv:
        got = red(rt, weights=w)
    assert fv.g4 >= 1 and fv.g2 == 0
    assert_bitexact(got, oc.reduce_plain(enc, w))
    return fl


@pytest.mark.parametrize("kind", ["normal", "heavy", "ties"])
@pytest.mark.parametrize("d", [262_145, 300_007, 319_493])
def test_wg_ragged_items(ag, kind, d):
    """n = 256 (the smallest many-row shape with n * D >= 64 Mi).  D = 262 145: 65 chunks, the last
    item is one chunk holding one element; 300 007: 74 chunks, the last item holds 2.5 groups;
    319 493: 79 chunks, the last item holds 3 full groups and a ragged fourth."""
    n = 256
    assert n * d >= 64 << 20
    g = np.random.default_rng([n, d, len(kind), 7])
    fl = _run(ag, _topk_rows(kind, n, d, g), "topk:1%", g)
    if kind == "normal":
        assert not np.any(fl & 8), f"{int(np.sum((fl & 8) != 0))} rows took the exact path"


# big entries per group 0..3 of the row's first item; groups 1 (and 3) sit at the staging capacity,
# their siblings hold counts that are no multiple of 4 (the copied-out pieces meet off the quads)
SEAMS = {"g1": [(255, 511, 257, 0), (257, 512, 255, 0), (255, 513, 257, 0)],
         "g1+g3": [(255, 511, 257, 513), (257, 513, 255, 512), (255, 512, 257, 511), (257, 512, 255, 513)]}


@pytest.mark.parametrize("where", sorted(SEAMS))
def test_wg_seams_and_overflow_inside_one_item(ag, where):
    """n = 17, D = 4 000 000, rows as test_topk_4chunk_group_staging_capacity builds them: K big
    entries (|x| >= 1) among small ones (|x| < 1e-3), the first item (elements 0..65 535) zero but
    for a chosen number of big entries in each of its four groups.  A group stages exactly its big
    entries: 511 and 512 fit, 513 overflows the group (flag 1) and its row is redone exactly
    (flag 8) while its siblings' pieces are still copied out."""
    n, d = 17, 4_000_000
    k = d // 100
    g = np.random.default_rng([len(where), 17, 3])
    rows = (g.uniform(1e-4, 1e-3, (n, d)) * np.where(g.random((n, d)) < 0.5, -1.0, 1.0)).astype(np.float32)
    rows[:, :4 * GROUP] = 0.0
    counts = [SEAMS[where][i % len(SEAMS[where])] for i in range(n)]
    for i in range(n):
        idx = [q * GROUP + g.choice(GROUP, size=m, replace=False) for q, m in enumerate(counts[i])]
        idx.append(4 * GROUP + g.choice(d - 4 * GROUP, size=k - sum(counts[i]), replace=False))
        idx = np.concatenate(idx)
        rows[i, idx] = ((np.abs(g.standard_normal(idx.size)) + 1.0) *
                        np.where(g.random(idx.size) < 0.5, -1.0, 1.0)).astype(np.float32)
    fl = _run(ag, rows, "topk:1%", g)
    for i in range(n):
        over = max(counts[i]) > GCAP
        assert bool(fl[i] & 1) == over and (not over or fl[i] & 8), f"row {i} {counts[i]}: flags {fl[i]}"


def test_wg_row_list_overflow_clustered(ag):
    """Clustered rows at n = 256, D = 300 007 in 2 row groups (as
    test_topk_exact_fallback_in_side_select): every row overflows its list inside the items that
    hold the cluster, carries flag 8 and comes out exact.  (At this D the list holds 2 K + 8192 =
    14 196 entries and 19 groups of at most 512 cannot pass it, so the overflow here is a group past
    its staging; test_wg_reservation_crosses_list_capacity crosses the list's end.)"""
    n, d = 256, 300_007
    g = np.random.default_rng([n, d, 9, 5])
    fl = _run(ag, _topk_rows("clustered", n, d, g), "topk:1%", g, row_groups=2)
    assert np.any(fl & 1), "no row overflowed"
    over = (fl & 1) != 0
    assert np.all(fl[over] & 8), f"{int(np.sum((fl[over] & 8) == 0))} overflowing rows without the exact path"


def _odd_rows(g):
    n, d = 65, 1_048_583
    assert n * d >= 64 << 20
    return g.standard_normal((n, d)).astype(np.float32)


def test_wg_odd_item_count(ag):
    """n = 65, D = 1 048 583 (257 chunks: 17 items a row, the last one chunk of 7 elements): a row
    count that is no multiple of the 64 rows of a block of the item order.  Normal rows."""
    g = np.random.default_rng([65, 11])
    fl = _run(ag, _odd_rows(g), "topk:1%", g)
    assert not np.any(fl & 8), f"{int(np.sum((fl & 8) != 0))} rows took the exact path"


def test_wg_reservation_crosses_list_capacity(ag):
    """A whole-item reservation that crosses the end of the row's list mid-row, no group past its
    staging.  n = 65, D = 1 048 583, K = 10 486: the list holds 2 K + 8192 = 29 164 entries.  Every
    fourth row has exactly 480 entries of magnitude >= 2 in each of its 64 full groups (K of them
    distinct and >= 3, the others exactly 2) among entries < 1e-3: the sample sees ~2.9 % of such
    entries, its rank (~1 % + 4 sigma) falls on a 2, so the filter admits 480 a group (<= 512, no
    group overflows), 1920 an item, 30 720 a row, and the 16th item reserved passes the list's end.
    Those rows carry flags 1 and 8, the normal rows between them neither; the result is exact."""
    n, d = 65, 1_048_583
    k = math.ceil(0.01 * d)
    per, full = 480, 64
    assert per <= GCAP and per * full > 2 * k + 8192 >= per * 4 * 15
    g = np.random.default_rng([65, 13])
    rows = _odd_rows(g)
    crafted = list(range(0, n, 4))
    for i in crafted:
        r = (g.uniform(1e-4, 1e-3, d) * np.where(g.random(d) < 0.5, -1.0, 1.0)).astype(np.float32)
        idx = np.concatenate([q * GROUP + g.choice(GROUP, size=per, replace=False) for q in range(full)])
        g.shuffle(idx)
        sign = np.where(g.random(idx.size) < 0.5, -1.0, 1.0)
        val = np.full(idx.size, 2.0)
        val[:k] = np.abs(g.standard_normal(k)) + 3.0
        r[idx] = (val * sign).astype(np.float32)
        rows[i] = r
    fl = _run(ag, rows, "topk:1%", g)
    for i in range(n):
        if i in crafted:
            assert fl[i] & 1 and fl[i] & 8, f"crafted row {i}: flags {fl[i]}"
        else:
            assert not fl[i] & 9, f"normal row {i}: flags {fl[i]}"
