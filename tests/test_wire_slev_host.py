"""Host side of the sparse level wire format (FMT_SLEV, include/flcodec.h "Sparse level messages"):
capacity and used sizes against the layout's formula, and flc_payload_validate_slev on hand-built
messages, each rule violated once.  No GPU compute is called here."""
import ctypes

import numpy as np
import pytest

from flpytorch_amd import _lib, aggregation as ag

DS = [1, 4095, 4096, 4097, 3 * 4096 + 77]


def a16(b):
    return (b + 15) // 16 * 16


def used_bytes(d, nnz):
    return 16 + a16(4 * (-(-d // 4096) + 1)) + a16(2 * nnz) + a16(nnz)


def slev_pack(head, codes, keep):
    """The message of a row's Q8 codes with the elements `keep` listed: header words (format word
    replaced), chunk offsets, chunk-local u16 indices, the codes; each block zero-padded to 16 B."""
    j = np.nonzero(keep)[0]
    C = -(-codes.size // 4096)
    tab = np.searchsorted(j, 4096 * np.arange(C + 1)).astype(np.uint32)
    head = np.asarray(head, np.uint32).copy()
    head[0] = 10
    pad = lambda a: np.concatenate([a.view(np.uint8), np.zeros(-a.nbytes % 16, np.uint8)])
    return np.concatenate([head.view(np.uint8), pad(tab), pad((j % 4096).astype(np.uint16)), pad(codes[j].astype(np.uint8))])


def used_of(msg, d):
    return _lib.load().flc_payload_slev_used(ctypes.c_void_p(msg.ctypes.data), msg.size, d)


@pytest.mark.parametrize("d", DS)
def test_capacity_and_used_bytes(d):
    comp = ag.initCompressor("qsgd:127", d)
    assert comp.payloadBytes(d, sparse_levels=True) == used_bytes(d, d)
    codes = np.full(d, 0x83, np.uint8)
    for keep in (np.zeros(d, bool), np.arange(d) % 3 == 0, np.ones(d, bool)):
        msg = slev_pack([10, d, 0, 0], codes, keep)
        assert used_of(msg, d) == msg.size == used_bytes(d, int(keep.sum()))
        assert used_of(msg[:16 + 4 * -(-d // 4096)], d) == 0            # tab[C] not reached


def message(d, s, norm=1.5, seed=0):
    g = np.random.default_rng(seed)
    codes = (g.integers(1, s + 1, d) | (g.integers(0, 2, d) << 7)).astype(np.uint8)
    keep = g.random(d) < 0.3
    keep[-1] = True                                                     # the last chunk is not empty
    keep[np.nonzero(~keep)[0][:(5 - keep.sum()) % 16]] = True           # nnz % 16 == 5: both planes are padded
    return slev_pack([10, d, np.float32(norm).view(np.uint32), 0], codes, keep)


def put(m, at, value, dtype=np.uint32):
    m[at:at + np.dtype(dtype).itemsize] = np.array([value], dtype).view(np.uint8)
    return m


D, S = 4097 + 4096, 5                                   # C = 3, the last chunk of length 1
IO = 16 + a16(4 * 4)                                    # the idx plane


def planes(m):
    nnz = int(m[16 + 12:16 + 16].view(np.uint32)[0])
    return nnz, IO + a16(2 * nnz)


def swap_first_pair(m):
    m[IO:IO + 4] = m[IO:IO + 4].view(np.uint16)[::-1].copy().view(np.uint8)
    return m


def grow_last_chunk(m):
    """tab[C] = tab[C - 1] + 2 with room for it: two entries in the chunk of length 1."""
    t2 = int(m[16 + 8:16 + 12].view(np.uint32)[0])
    return put(np.concatenate([m, np.zeros(64, np.uint8)]), 16 + 12, t2 + 2)


@pytest.mark.parametrize("reason,change", [
    ("header format 2", lambda m: put(m, 0, 2)),
    ("count 4097", lambda m: put(m, 4, 4097)),
    ("bytes, the message of", lambda m: m[:-16]),
    ("entries, d=", lambda m: put(m, 16 + 12, D + 1)),
    (r"tab\[0\] = 1", lambda m: put(m, 16, 1)),
    ("chunk 1 holds entries", lambda m: put(m, 16 + 4, int(m[16 + 8:16 + 12].view(np.uint32)[0]) + 1)),   # tab[1] > tab[2]
    ("chunk 2 holds entries", grow_last_chunk),
    ("not ascending", swap_first_pair),
    ("not ascending", lambda m: put(m, IO + 2 * (planes(m)[0] - 1), 1, np.uint16)),    # index 1 in the chunk of length 1
    ("level index 6 outside", lambda m: put(m, planes(m)[1], 0x86, np.uint8)),
    ("level index 0 outside", lambda m: put(m, planes(m)[1], 0x80, np.uint8)),
    ("padding", lambda m: put(m, m.size - 1, 1, np.uint8)),
    ("padding", lambda m: put(m, IO + 2 * planes(m)[0], 1, np.uint16)),                 # behind the last index
    ("3 elements flagged", lambda m: put(m, 12, 3)),
])
def test_validate_slev_refuses(reason, change):
    comp = ag.initCompressor(f"qsgd:{S}", D)
    good = message(D, S)
    comp.validatePayload(good.tobytes(), D, sparse_levels=True)
    with pytest.raises(ValueError, match=reason):
        comp.validatePayload(change(good.copy()).tobytes(), D, sparse_levels=True)


def test_level_zero_is_legal_under_a_non_finite_norm():
    comp, d = ag.initCompressor("terngrad", 100), 100
    codes = np.where(np.arange(d) % 2, 0x80, 0x00).astype(np.uint8)
    msg = slev_pack([10, d, np.float32(np.inf).view(np.uint32), 0], codes, np.ones(d, bool))
    comp.validatePayload(msg.tobytes(), d, sparse_levels=True)
