"""CPU tests for the references in kernel_refs.py and for the host paths of
crc32c, gather, gather_ptr, fill and LZ4 decode.

The GPU tests in test_gpu_kernel_edges.py compare the kernels with
native.crc32c, numpy slicing and the LZ4 assembler's raw bytes.  This file
shows, without a device, that those yardsticks agree with each other: the
bytewise CRC with native.crc32c on the published vectors, the pure-Python
LZ4 decoder with the host decoder on both corpora, and every matrix of
kernel_edge_cases.py with the host arena.
"""
import numpy as np
import pytest

import kernel_edge_cases as edges
from curvine_amd import native
from kernel_refs import (Lz4RefError, crc32c_ref, cvlz, cvlz_decode_ref,
                         lz4_block, lz4_block_decode_ref)


@pytest.fixture(scope="module")
def host_arena():
    a = native.Arena(-1, 40 << 20)
    yield a
    a.close()


# ---------------------------------------------------------------------------
# CRC32C
# ---------------------------------------------------------------------------

KNOWN = [
    (b"123456789", 0xE3069283),
    # RFC 3720 B.4
    (bytes(32), 0x8A9136AA),
    (b"\xff" * 32, 0x62A8AB43),
    (bytes(range(32)), 0x46DD794E),
    (bytes(range(31, -1, -1)), 0x113FDB5C),
]


@pytest.mark.parametrize("data,crc", KNOWN)
def test_crc_known_answers(data, crc):
    assert crc32c_ref(data) == crc
    assert native.crc32c(data) == crc


def test_crc_ref_vs_native():
    rng = np.random.default_rng(11)
    for n in list(range(65)) + [4095, 4096, 4097, 65536]:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert crc32c_ref(data) == native.crc32c(data), n


def test_crc_chaining():
    data = np.random.default_rng(12).integers(
        0, 256, 10000, dtype=np.uint8).tobytes()
    whole = native.crc32c(data)
    assert whole == crc32c_ref(data)
    for cut in (0, 1, 7, 8, 9, 4096, 9999, 10000):
        a, b = data[:cut], data[cut:]
        assert native.crc32c(b, native.crc32c(a)) == whole, cut
        assert crc32c_ref(b, crc32c_ref(a)) == whole, cut
        assert native.crc32c_combine(native.crc32c(a), native.crc32c(b),
                                     len(b)) == whole, cut


# ---------------------------------------------------------------------------
# LZ4 assembler and decoder
# ---------------------------------------------------------------------------

def test_assembler_bytes():
    """The assembler's output for a hand-worked block."""
    block, raw = lz4_block([(b"ab", 2, 6)], b"xyz")
    #  token 0x22: 2 literals, match 4+2 | "ab" | offset 2 | token 0x30 "xyz"
    assert block == b"\x22ab\x02\x00\x30xyz"
    assert raw == b"abababab" + b"xyz"
    # 15 and 270 are the first lengths with one and two extension bytes
    assert lz4_block([], bytes(15))[0][:2] == b"\xf0\x00"
    assert lz4_block([], bytes(270))[0][:3] == b"\xf0\xff\x00"
    assert lz4_block([(b"a", 1, 19)], None)[0] == b"\x1fa\x01\x00\x00"
    assert lz4_block([(b"a", 1, 274)], None)[0] == b"\x1fa\x01\x00\xff\x00"
    assert cvlz([b"\x10a"], 8, 1) == \
        b"4LZC" + (1).to_bytes(8, "little") + (8).to_bytes(4, "little") + \
        (1).to_bytes(4, "little") + (2).to_bytes(4, "little") + b"\x10a"


@pytest.mark.parametrize("name", edges.WELL_FORMED)
def test_lz4_well_formed(host_arena, name):
    container, raw = edges.well_formed(name)
    assert cvlz_decode_ref(container) == raw
    assert native.lz4_decompress(container) == raw
    edges.lz4_decode(host_arena, name)


@pytest.mark.parametrize("name", edges.MALFORMED)
def test_lz4_malformed(host_arena, name):
    container = edges.malformed(name)
    with pytest.raises(Lz4RefError):
        cvlz_decode_ref(container)
    with pytest.raises(RuntimeError, match="lz4"):
        native.lz4_decompress(container)
    edges.lz4_reject(host_arena, name)


def test_lz4_malformed_is_only_the_middle_chunk():
    """Each malformed container is damaged in its middle chunk alone: with
    that chunk replaced by a good one it decodes."""
    good, raw = lz4_block([(b"0123456789", 3, 20)], bytes(34))
    assert lz4_block_decode_ref(good, 64) == raw
    for name in edges.MALFORMED:
        c = edges.malformed(name)
        sizes = np.frombuffer(c, dtype="<u4", count=3, offset=20)
        first = c[32:32 + sizes[0]]
        last = c[32 + sizes[0] + sizes[1]:]
        assert len(last) == sizes[2], name
        assert len(lz4_block_decode_ref(first, 64)) == 64, name
        assert len(lz4_block_decode_ref(last, 64)) == 64, name
        with pytest.raises(Lz4RefError):
            lz4_block_decode_ref(c[32 + sizes[0]:32 + sizes[0] + sizes[1]], 64)


# ---------------------------------------------------------------------------
# the arena matrices on a host arena
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "zeros", "ones"])
def test_crc_matrix(host_arena, kind):
    edges.crc_matrix(host_arena, kind)


def test_crc_small(host_arena):
    edges.crc_small(host_arena)


def test_crc_coverage(host_arena):
    edges.crc_coverage(host_arena)


@pytest.mark.parametrize("path", edges.TILE_PATHS)
def test_gather_tile_paths(host_arena, path):
    edges.gather_tile_paths(host_arena, edges.HostDst, path)


def test_gather_alignment(host_arena):
    edges.gather_alignment(host_arena, edges.HostDst)


def test_gather_grid_stride(host_arena):
    edges.gather_grid_stride(host_arena, edges.HostDst)


def test_gather_empty(host_arena):
    edges.gather_empty(host_arena, edges.HostDst)


@pytest.mark.parametrize("residue", range(16))
def test_fill_matrix(host_arena, residue):
    edges.fill_matrix(host_arena, residue)


def test_fill_grid_stride(host_arena):
    edges.fill_grid_stride(host_arena)
