"""Host side of the bit-packed wire formats (FMT_LBITS / FMT_NAT9, include/flcodec.h "Bit-packed
messages"): payload sizes against the layout's formula and the reference's counted bits, and
flc_payload_validate_bits on hand-built messages.  No GPU compute is called here."""
import numpy as np
import pytest

from flpytorch_amd import aggregation as ag

SPECS = ["terngrad", "qsgd:3", "qsgd:7", "qsgd:15", "qsgd:31", "qsgd:63", "natural"]
DS = [1, 2047, 2048, 2049, 3 * 2048 + 77]


def width(comp):
    """Bits per code: 9 for natural, else the sign and bit_length(s) bits of level index."""
    return 1 + int(comp.s).bit_length() if hasattr(comp, "s") else 9


def tile_pack(codes, b):
    """The body of a bit-packed message: tiles of 2048 codes, element 256 t + 4 l + q is lane l's code
    4 t + q, a lane's 32 codes LSB-first in b words, word k of lane l at word k * 64 + l of the tile."""
    T = -(-codes.size // 2048)
    c = np.zeros(T * 2048, np.uint32)
    c[:codes.size] = codes
    c = c.reshape(T, 8, 64, 4).transpose(0, 2, 1, 3).reshape(T, 64, 32)
    bit = ((c[..., None] >> np.arange(b, dtype=np.uint32)) & 1).astype(np.uint8)
    words = np.packbits(bit.reshape(T, 64, 32 * b), axis=-1, bitorder="little").view(np.uint32)
    return np.ascontiguousarray(words.transpose(0, 2, 1)).reshape(-1)


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("d", DS)
def test_payload_bytes(spec, d):
    comp = ag.initCompressor(spec, d)
    b = width(comp)
    assert comp.payloadBytes(d, bits=True) == 16 + 256 * b * -(-d // 2048)
    if spec.startswith("qsgd"):     # s not a power of two: the reference's counted bits, plus the tile padding
        assert 8 * (comp.payloadBytes(d, bits=True) - 16) <= 32 * (comp._need_to_send(d) - 1) + b * (-d % 2048)


def message(d, b, s, seed=0):
    g = np.random.default_rng(seed)
    codes = (g.integers(0, s + 1, d) | (g.integers(0, 2, d) << (b - 1))).astype(np.uint32)
    head = np.array([7 | (b << 8), d, np.float32(1.5).view(np.uint32), 0], np.uint32)
    return np.concatenate([head, tile_pack(codes, b)])


def edit(words, at, value):
    words[at] = value
    return words


@pytest.mark.parametrize("reason,change", [
    ("bytes, the bit-packed message", lambda m: m[:-1]),
    ("header format 2", lambda m: edit(m, 0, 2 | (4 << 8))),
    ("b=5 bits per code", lambda m: edit(m, 0, 7 | (5 << 8))),
    ("count 2048", lambda m: edit(m, 1, 2048)),
    ("3 elements flagged", lambda m: edit(m, 3, 3)),
    ("level code 7 at 1 exceeds s=5", lambda m: edit(m, 4, m[4] | (7 << 4))),     # lane 0's code 1: element 1
])
def test_validate_bits_refuses(reason, change):
    d, comp = 2049, ag.initCompressor("qsgd:5", 2049)                               # b = 4, indices up to 7
    good = message(d, 4, 5)
    comp.validatePayload(good.tobytes(), d, bits=True)
    with pytest.raises(ValueError, match=reason):
        comp.validatePayload(change(good.copy()).tobytes(), d, bits=True)
