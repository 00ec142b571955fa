"""Shared helpers for the LZ4 tests: a strict CVLZ / LZ4-block checker and
the seeded data kinds.  The checker is deliberately independent of the
codec in csrc/lz4.hip: it walks every chunk and enforces the LZ4
end-of-block rules third-party decoders rely on."""
import os
import random
import struct

CHUNK = 65536
MAGIC = 0x435A4C34


def worst_case(n: int) -> int:
    """Upper bound of a container for n raw bytes: header, sizes table and
    the LZ4 worst case (n + n//255 + 16) per chunk."""
    n_chunks = (n + CHUNK - 1) // CHUNK
    total = 20 + 4 * n_chunks
    for c in range(n_chunks):
        cn = min(CHUNK, n - c * CHUNK)
        total += cn + cn // 255 + 16
    return total


def _length(buf, si, nib):
    if nib == 15:
        while True:
            b = buf[si]
            si += 1
            nib += b
            if b != 255:
                break
    return nib, si


def strict_check(container: bytes, raw_len: int) -> None:
    magic, raw, chunk, n_chunks = struct.unpack_from("<IQII", container, 0)
    assert magic == MAGIC
    assert raw == raw_len
    assert chunk == CHUNK
    assert n_chunks == (raw_len + CHUNK - 1) // CHUNK
    sizes = struct.unpack_from(f"<{n_chunks}I", container, 20)
    payload = container[20 + 4 * n_chunks:]
    assert sum(sizes) == len(payload), "sizes table != payload length"
    base = 0
    for c, cs in enumerate(sizes):
        buf = payload[base:base + cs]
        base += cs
        cn = min(CHUNK, raw_len - c * CHUNK)
        si = di = 0
        last_lit = None
        while True:
            assert si < cs, f"chunk {c}: ran off the block"
            tok = buf[si]
            lit, si = _length(buf, si + 1, tok >> 4)
            assert si + lit <= cs and di + lit <= cn, f"chunk {c}: literals overrun"
            si += lit
            di += lit
            if si == cs:            # last sequence: literals only
                assert tok & 0xF == 0, f"chunk {c}: last sequence has a match"
                last_lit = lit
                break
            assert si + 2 <= cs
            off = buf[si] | (buf[si + 1] << 8)
            mlen, si = _length(buf, si + 2, tok & 0xF)
            mlen += 4
            assert off != 0 and off <= di, f"chunk {c}: offset {off} at {di}"
            if cn >= 13:
                assert di + 12 < cn, f"chunk {c}: match starts at {di} of {cn}"
            else:
                raise AssertionError(f"chunk {c}: match in a {cn}-byte chunk")
            di += mlen
            assert di <= cn - 5, f"chunk {c}: match ends at {di} of {cn}"
        assert di == cn, f"chunk {c}: produced {di} of {cn}"
        assert last_lit >= min(cn, 5), f"chunk {c}: last literals {last_lit}"


def zero_first_match_offset(container: bytes) -> bytes:
    """The container with the first match offset of chunk 0 set to 0, which
    no decoder may accept."""
    _, _, _, n_chunks = struct.unpack_from("<IQII", container, 0)
    start = 20 + 4 * n_chunks
    tok = container[start]
    lit, si = _length(container, start + 1, tok >> 4)
    si += lit
    assert si + 2 <= start + struct.unpack_from("<I", container, 20)[0], \
        "chunk 0 has no match"
    out = bytearray(container)
    out[si] = out[si + 1] = 0
    return bytes(out)


def text8(n: int, seed: int = 7) -> bytes:
    return bytes(random.Random(seed).choices(b"abcdefgh", k=n))


def pattern(n: int) -> bytes:
    return (b"pattern123" * (n // 10 + 1))[:n]


CPU_KINDS = {
    "zeros": lambda n: bytes(n),
    "urandom": lambda n: os.urandom(n),
    "pattern123": pattern,
    "text8": text8,
}
