"""The edge matrices for crc32c, gather, gather_ptr, fill and LZ4 decode,
written once against the Arena interface.  tests/test_kernel_refs.py runs
them on a host arena, where the C++ host paths answer, and
tests/test_gpu_kernel_edges.py on a device arena, where crc32c_kernel,
copy_extents_kernel, fill_kernel and lz4_decompress_kernel do.  The
expectations come from numpy slicing, native.crc32c on the same bytes and
the LZ4 assembler's own byte-by-byte copy; every comparison is bitwise.

An arena needs 40 MiB.  `dst_factory(n, value)` returns a destination
buffer for gather_ptr in the arena's own memory kind, with `.ptr` and
`.numpy()`.
"""
import functools
import random

import numpy as np
import pytest

from curvine_amd import native
from kernel_refs import cvlz, lz4_block, lz4_sequence

SUB = 4096                  # bytes per thread in crc32c_kernel
TILE = 65536                # bytes per workgroup tile in copy_extents_kernel
GUARD = 0x5A


class HostDst:
    """gather_ptr destination for a host arena."""

    def __init__(self, n, value):
        self.a = np.full(n, value, dtype=np.uint8)
        self.ptr = self.a.ctypes.data

    def numpy(self):
        return self.a


class TorchDst:
    """gather_ptr destination for a device arena: a torch uint8 tensor."""

    def __init__(self, n, value):
        import torch
        self.t = torch.full((n,), value, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.ptr = self.t.data_ptr()

    def numpy(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _read(arena, off, n):
    out = np.zeros(n, dtype=np.uint8)
    if n:
        arena.read(off, out, 0, n)
    return out


# ---------------------------------------------------------------------------
# CRC32C
# ---------------------------------------------------------------------------

# Inside one 256-thread workgroup the tree combine meets a ragged right node
# at level k whenever the count has bit k clear below its top bit: 3, 5, 7,
# 9, 31, 33, 127, 129, 255 and 300 (0b100101100) walk the per-bit matrix
# loop at every level.  257, 300, 511, 513 and 767 end in a partial last
# workgroup, which the host side combines with a shorter shift.
CRC_COUNTS = (1, 2, 3, 5, 7, 8, 9, 31, 33, 127, 128, 129, 255, 256, 257, 300,
              511, 512, 513, 767)
CRC_TAILS = (0, 1, 7, 8, 4095)
CRC_OFFSETS = (0, 8, 4104, 1, 3, 4099, 4103)
CRC_BASE = 1 << 20
_CRC_SPAN = 4104 + 767 * SUB + 4095


def _crc_kind(kind):
    if kind == "random":
        return _rand(_CRC_SPAN, 21)
    return np.full(_CRC_SPAN, 0 if kind == "zeros" else 0xFF, dtype=np.uint8)


def crc_matrix(arena, kind):
    """arena.crc32c over every count x tail x offset of one data kind.  The
    bytes are written once; each case checksums a window of them."""
    data = _crc_kind(kind)
    arena.write(CRC_BASE, data, 0, len(data))
    bad = []
    for off in CRC_OFFSETS:
        for count in CRC_COUNTS:
            for tail in CRC_TAILS:
                n = count * SUB + tail
                got = arena.crc32c(CRC_BASE + off, n)
                want = native.crc32c(data[off:off + n])
                if got != want:
                    bad.append((off, count, tail, hex(got), hex(want)))
    assert not bad, f"{kind}: {len(bad)} wrong, first {bad[:5]}"


def crc_small(arena):
    """Lengths below one sub-chunk, where only the head and tail code runs,
    at every offset residue mod 8."""
    data = _rand(8192, 22)
    arena.write(CRC_BASE, data, 0, len(data))
    for off in range(0, 17):
        for n in (0, 1, 2, 6, 7, 8, 9, 15, 16, 17, 4095):
            assert arena.crc32c(CRC_BASE + off, n) == \
                native.crc32c(data[off:off + n]), (off, n)


def crc_coverage(arena):
    """300 sub-chunks + 7 bytes: one flipped byte in the first, a middle and
    the last sub-chunk and in the tail each changes the CRC, which still
    equals the host's: no sub-chunk drops out of the ragged combine."""
    n = 300 * SUB + 7
    data = _rand(n, 23)
    arena.write(CRC_BASE, data, 0, n)
    clean = arena.crc32c(CRC_BASE, n)
    assert clean == native.crc32c(data)
    for pos in (17, 150 * SUB + 1234, 299 * SUB + 4095, 300 * SUB + 3):
        data[pos] ^= 0x40
        arena.write(CRC_BASE + pos, data[pos:pos + 1], 0, 1)
        got = arena.crc32c(CRC_BASE, n)
        assert got != clean, f"flip at {pos} not seen"
        assert got == native.crc32c(data), f"flip at {pos}"
        data[pos] ^= 0x40
        arena.write(CRC_BASE + pos, data[pos:pos + 1], 0, 1)
    assert arena.crc32c(CRC_BASE, n) == clean


# ---------------------------------------------------------------------------
# extent copy: gather (packed into a host buffer) and gather_ptr (explicit
# destination offsets in the arena's own memory kind)
# ---------------------------------------------------------------------------

SRC_N = 1 << 20


@functools.lru_cache(maxsize=None)
def _src():
    a = _rand(SRC_N, 31)
    a.setflags(write=False)
    return a


def _load_src(arena):
    arena.write(0, _src(), 0, SRC_N)
    return _src()


def _check_gather(arena, extents, label):
    src = _src()
    total = sum(n for _, n in extents)
    out = np.full(total + 32, GUARD, dtype=np.uint8)
    arena.gather(extents, out, 16)
    parts = [src[o:o + n] for o, n in extents]
    want = np.concatenate([np.full(16, GUARD, dtype=np.uint8)] + parts +
                          [np.full(16, GUARD, dtype=np.uint8)])
    assert np.array_equal(out, want), label


def _check_gather_ptr(arena, dst_factory, triples, dst_n, label):
    src = _src()
    model = np.full(dst_n, GUARD, dtype=np.uint8)
    used = np.zeros(dst_n, dtype=bool)
    for s, d, n in triples:
        assert d + n <= dst_n and not used[d:d + n].any(), \
            "test extents overlap or leave the destination"
        used[d:d + n] = True
        model[d:d + n] = src[s:s + n]
    dst = dst_factory(dst_n, GUARD)
    arena.gather_ptr(triples, dst.ptr)
    assert np.array_equal(dst.numpy(), model), label


# (src_off, len) of the three tile shapes: exactly one tile, one tile plus
# one 16-byte vector, three tiles
_SHAPES = ((16, TILE), (2 * TILE + 32, TILE + 16), (6 * TILE, 3 * TILE))


def _tile_path_cases():
    """name -> (gather extents, gather_ptr triples).  `shift` moves source
    and destination alike, so 0 keeps the 16-byte path, 12 leaves the
    4-byte path and 1 the byte path."""
    cases = {}
    for name, shift, extra in (("vec16", 0, None), ("vec4", 12, None),
                               ("byte", 1, (9 * TILE + 3, 2 * TILE + 1))):
        shapes = [(s + shift, n) for s, n in _SHAPES]
        if extra:
            shapes.append(extra)
        # gather packs from 0: a leading extent of `shift` bytes gives the
        # destinations the same residue as the sources
        ext = ([(5, shift)] if shift else []) + shapes
        triples, d = [], 64 + shift
        for s, n in shapes:
            triples.append((s, d, n))
            d += (n + 15) // 16 * 16 + 64       # keeps d = shift mod 16
        cases[name] = (ext, triples, d + 64)
    return cases


TILE_PATHS = ("vec16", "vec4", "byte")


def gather_tile_paths(arena, dst_factory, path):
    _load_src(arena)
    ext, triples, dst_n = _tile_path_cases()[path]
    if path == "vec16":
        assert all(s % 16 == 0 and n % 16 == 0 for s, n in ext)
        assert all(s % 16 == 0 and d % 16 == 0 and n % 16 == 0
                   for s, d, n in triples)
    elif path == "vec4":
        assert all(s % 16 == 12 and d % 16 == 12 and n % 4 == 0
                   for s, d, n in triples)
    else:
        assert all(s % 2 == 1 and d % 2 == 1 for s, d, n in triples)
        assert triples[-1][2] == 2 * TILE + 1
    _check_gather(arena, ext, path)
    _check_gather_ptr(arena, dst_factory, triples, dst_n, path)


_ALIGN_LENS = (0, 1, 3, 4, 15, 16, 17, 64)


def gather_alignment(arena, dst_factory):
    """Every source residue x destination residue (mod 16) x length, 2048
    extents in one call each."""
    _load_src(arena)
    combos = [(sr, dr, n) for sr in range(16) for dr in range(16)
              for n in _ALIGN_LENS]
    random.Random(32).shuffle(combos)
    # gather_ptr: destination offsets are given directly
    triples = [(16 * ((i * 37) % 60000) + sr, i * 128 + dr, n)
               for i, (sr, dr, n) in enumerate(combos)]
    _check_gather_ptr(arena, dst_factory, triples, len(combos) * 128 + 64,
                      "alignment")
    # gather: the destination residue is the running total, so a pad extent
    # of 0..15 bytes in front of each case steers it
    ext, total = [], 0
    for i, (sr, dr, n) in enumerate(combos):
        pad = (dr - total) % 16
        ext.append((16 * ((i * 53) % 60000) + 7, pad))
        ext.append((16 * ((i * 37) % 60000) + sr, n))
        total += pad + n
        assert (total - n) % 16 == dr
    _check_gather(arena, ext, "alignment")


def gather_grid_stride(arena, dst_factory):
    """8300 extents of 1..40 bytes are 8300 tiles for a grid capped at
    8192: the last 108 are reached only by `tile += gridDim.x`."""
    _load_src(arena)
    rng = random.Random(33)
    lens = [rng.randint(1, 40) for _ in range(8300)]
    srcs = [rng.randrange(SRC_N - 40) for _ in lens]
    _check_gather(arena, list(zip(srcs, lens)), "grid-stride")
    triples = [(s, 16 + i * 48 + (i % 7), n)
               for i, (s, n) in enumerate(zip(srcs, lens))]
    _check_gather_ptr(arena, dst_factory, triples, 16 + 8300 * 48 + 64,
                      "grid-stride")


def gather_empty(arena, dst_factory):
    """No extents, and only zero-length extents, do nothing and raise
    nothing; a zero-length extent inside a normal list is skipped."""
    _load_src(arena)
    for ext in ([], [(5, 0)], [(5, 0), (9, 0), (SRC_N, 0)]):
        out = np.full(64, GUARD, dtype=np.uint8)
        arena.gather(ext, out, 8)
        assert (out == GUARD).all(), ext
        dst = dst_factory(256, GUARD)
        arena.gather_ptr([(s, 32, n) for s, n in ext], dst.ptr)
        assert (dst.numpy() == GUARD).all(), ext
    _check_gather(arena, [(0, 100), (50, 0), (200, 64), (7, 0)], "mixed")
    _check_gather_ptr(arena, dst_factory,
                      [(0, 16, 100), (50, 120, 0), (200, 128, 64),
                       (7, 0, 0)], 256, "mixed")


# ---------------------------------------------------------------------------
# fill
# ---------------------------------------------------------------------------

FILL_LENS = (0, 1, 15, 16, 17, 31, 33, 255, 4101, 65537)
_FILL_G = 64                # guard bytes either side of each filled range


def fill_matrix(arena, residue):
    """Offsets 4096 + residue (mod 16) x every length x values 0x00 and
    0xAB.  The lengths lie side by side, each in a slot with 64 guard bytes
    before and after, at slot strides that keep the residue; the slots are
    prefilled with 0x5A in one write, filled one by one and read back in
    one read."""
    base = 4096 + residue - _FILL_G
    slots, pos = [], 0
    for n in FILL_LENS:
        slots.append((pos + _FILL_G, n))
        pos += (n + 2 * _FILL_G + 15) // 16 * 16
    assert slots[0][0] + base == 4096 + residue
    for value in (0x00, 0xAB):
        model = np.full(pos, GUARD, dtype=np.uint8)
        arena.write(base, model, 0, pos)
        for rel, n in slots:
            assert (base + rel) % 16 == residue
            arena.fill(base + rel, n, value)
            model[rel:rel + n] = value
        got = _read(arena, base, pos)
        if not np.array_equal(got, model):
            first = int(np.flatnonzero(got != model)[0])
            raise AssertionError(
                f"residue {residue} value {value:#x}: first difference at "
                f"region byte {first}; slots {slots}")


def fill_grid_stride(arena):
    """32 MiB + 4099 bytes at offset 4099: 2097408 vectors for a grid of
    8192 x 256 threads, so the 16-byte loop goes round a second time, on a
    destination of residue 3; the 3-byte tail follows."""
    off, n = 4099, (32 << 20) + 4099
    guard = np.full(_FILL_G, GUARD, dtype=np.uint8)
    arena.write(off - _FILL_G, guard, 0, _FILL_G)
    arena.write(off + n, guard, 0, _FILL_G)
    arena.fill(off, n, 0xAB)
    got = _read(arena, off - _FILL_G, n + 2 * _FILL_G)
    assert (got[:_FILL_G] == GUARD).all() and (got[-_FILL_G:] == GUARD).all()
    assert np.array_equal(got[_FILL_G:-_FILL_G],
                          np.full(n, 0xAB, dtype=np.uint8))


# ---------------------------------------------------------------------------
# LZ4 corpora.  Every entry is (container, raw_bytes); builders are cached
# so the host and device legs decode the very same bytes.
# ---------------------------------------------------------------------------

LZ4_DST = 4099
LZ4_GUARD = 0xEE
_LZ4_G = 64

MATCH_OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255,
                 256, 65535)
MATCH_LENS = (4, 18, 19, 64, 65, 273, 274, 1000)
LITERAL_RUNS = (0, 1, 14, 15, 16, 269, 270, 271, 525)


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def _single(seqs, last):
    block, raw = lz4_block(seqs, last)
    return cvlz([block], max(len(raw), 1), len(raw)), raw


def _match_offset(off):
    """`off` literals, then every match length at that offset with a few
    fresh literals in between so the period's content changes.  18/19 and
    273/274 sit either side of the one- and two-byte length extension."""
    rng = random.Random(1000 + off)
    seqs = [(_rb(rng, off if i == 0 else 5), off, m)
            for i, m in enumerate(MATCH_LENS)]
    return _single(seqs, _rb(rng, 6))


def _literal_runs(last):
    rng = random.Random(41)
    seqs = [(_rb(rng, 20), 3, 5)]
    seqs += [(_rb(rng, n), 7, 8) for n in LITERAL_RUNS]
    return _single(seqs, last)


def _random_block(rng, cap):
    """A random well-formed block that decodes to exactly `cap` bytes."""
    seqs, pos = [], 0
    while cap - pos > 48:
        lit = rng.choice((0, 1, 3, 14, 15, 16, 30)) or (0 if pos else 1)
        off = rng.randint(1, min(pos + lit, 65535))
        mlen = rng.randint(4, min(cap - pos - lit - 1, 300))
        seqs.append((_rb(rng, lit), off, mlen))
        pos += lit + mlen
    block, raw = lz4_block(seqs, _rb(rng, cap - pos))
    assert len(raw) == cap
    return block, raw


def _many_chunks(chunk_size, n_chunks, last):
    rng = random.Random(chunk_size)
    caps = [chunk_size] * (n_chunks - 1) + [last]
    blocks, raws = zip(*[_random_block(rng, cap) for cap in caps])
    raw = b"".join(raws)
    return cvlz(list(blocks), chunk_size, len(raw)), raw


def _tiny_chunks():
    """16400 literal-only chunks of 16 bytes (the last of 7) for a grid
    capped at 16384: chunks 16384.. are reached only by `c += gridDim.x`."""
    raw = _rand(16399 * 16 + 7, 42).tobytes()
    blocks = [lz4_sequence(raw[i:i + 16]) for i in range(0, len(raw), 16)]
    assert len(blocks) == 16400
    return cvlz(blocks, 16, len(raw)), raw


def _host_compressed(kind):
    rng = random.Random(7)
    raw = {
        "text8": lambda: bytes(rng.choices(b"abcdefgh", k=200_000)),
        "random": lambda: _rand(100_000, 43).tobytes(),
        "zeros_then_random":
            lambda: bytes(5 * 65536) + _rand(1000, 44).tobytes(),
        "pattern123": lambda: (b"pattern123" * 14000)[:2 * 65536 + 13],
    }[kind]()
    return native.lz4_compress(raw), raw


_WELL_FORMED = {
    **{f"offset{o}": functools.partial(_match_offset, o)
       for o in MATCH_OFFSETS},
    "literal_runs": lambda: _literal_runs(b""),
    "literal_runs_end_on_match": lambda: _literal_runs(None),
    # the match reaches back to the first byte of the chunk
    "offset_is_position": lambda: _single(
        [(_rb(random.Random(45), 13), 13, 40)], b"tail!"),
    # the match source is the literals of the same sequence
    "source_in_own_literals": lambda: _single(
        [(b"0123456789abcdef", 16, 8), (b"wxyz", 4, 30)], b"closing"),
    "chunks_4096": lambda: _many_chunks(4096, 20, 1234),
    "chunks_1000": lambda: _many_chunks(1000, 37, 333),
    "chunks_16_x16400": _tiny_chunks,
    "empty": lambda: (cvlz([], 65536, 0), b""),
    **{f"host_{k}": functools.partial(_host_compressed, k)
       for k in ("text8", "random", "zeros_then_random", "pattern123")},
}
WELL_FORMED = tuple(_WELL_FORMED)


@functools.lru_cache(maxsize=None)
def well_formed(name):
    return _WELL_FORMED[name]()


_MAL_CAP = 64


def _malformed_blocks():
    """name -> damaged block for a chunk of 64 raw bytes."""
    rng = random.Random(46)
    r = functools.partial(_rb, rng)
    closing = lz4_sequence(r(8))
    return {
        "offset_zero": lz4_sequence(r(8), 0, 10) + closing,
        "offset_before_start": lz4_sequence(r(8), 9, 10) + closing,
        # the token announces 20 literals, 5 follow
        "literals_past_block": bytes([0xF0, 5]) + r(5),
        "literals_past_cap": lz4_block([], r(_MAL_CAP + 6))[0],
        "match_past_cap": lz4_block([(r(10), 5, _MAL_CAP - 4)], b"")[0],
        "literal_ext_to_end": bytes([0xF0, 255, 255, 255]),
        "match_ext_to_end": bytes([0x1F]) + r(1) + b"\x01\x00\xff\xff",
        "ends_inside_offset": bytes([0x10]) + r(1) + b"\x01",
        "short_decode": lz4_block([(r(10), 3, 20)], r(10))[0],
        "empty_chunk": b"",
    }


MALFORMED = tuple(_malformed_blocks())


@functools.lru_cache(maxsize=None)
def malformed(name):
    """A three-chunk container whose middle chunk is damaged.  The damaged
    chunk is followed by a whole valid one, so a decoder that lacks an end
    check still reads only bytes of this container's payload."""
    good, raw = lz4_block([(_rb(random.Random(47), 10), 3, 20)],
                          _rb(random.Random(48), _MAL_CAP - 30))
    assert len(raw) == _MAL_CAP
    return cvlz([good, _malformed_blocks()[name], good], _MAL_CAP,
                3 * _MAL_CAP)


def _lz4_window(arena, raw_size):
    arena.fill(LZ4_DST - _LZ4_G, raw_size + 2 * _LZ4_G, LZ4_GUARD)


def lz4_decode(arena, name):
    container, raw = well_formed(name)
    _lz4_window(arena, len(raw))
    assert arena.lz4_decompress_into(LZ4_DST, container) == len(raw)
    got = arena.read_bytes(LZ4_DST - _LZ4_G, len(raw) + 2 * _LZ4_G)
    guard = bytes([LZ4_GUARD]) * _LZ4_G
    assert got[:_LZ4_G] == guard and got[len(got) - _LZ4_G:] == guard, name
    assert got[_LZ4_G:_LZ4_G + len(raw)] == raw, name


def lz4_reject(arena, name):
    container = malformed(name)
    raw_size = 3 * _MAL_CAP
    _lz4_window(arena, raw_size)
    with pytest.raises(RuntimeError, match="lz4"):
        arena.lz4_decompress_into(LZ4_DST, container)
    guard = bytes([LZ4_GUARD]) * _LZ4_G
    assert arena.read_bytes(LZ4_DST - _LZ4_G, _LZ4_G) == guard, name
    assert arena.read_bytes(LZ4_DST + raw_size, _LZ4_G) == guard, name
