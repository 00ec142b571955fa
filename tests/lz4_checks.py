"""Shared helpers for the LZ4 tests: a strict CVLZ / LZ4-block checker and
the seeded data kinds.  The checker is deliberately independent of the
codec in csrc/lz4.hip: it walks every chunk and enforces the LZ4
end-of-block rules third-party decoders rely on.  `sequences` lists what
a compressor emitted with the same walk, and `norepeat` / `compose` /
`planted` build inputs whose ideal parse is known."""
import random
import struct

import numpy as np

from kernel_refs import lz4_block

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


def sequences(container: bytes):
    """Per chunk, the list of (lit_len, offset, match_len,
    block_pos_of_literals) of every sequence; offset and match_len are None
    for the closing literals-only sequence.  The position is that of the
    first literal byte inside the chunk's block.  Meant for containers that
    passed strict_check."""
    _, _, _, n_chunks = struct.unpack_from("<IQII", container, 0)
    sizes = struct.unpack_from(f"<{n_chunks}I", container, 20)
    base = 20 + 4 * n_chunks
    out = []
    for cs in sizes:
        buf = container[base:base + cs]
        base += cs
        seqs, si = [], 0
        while True:
            tok = buf[si]
            lit, si = _length(buf, si + 1, tok >> 4)
            at = si
            si += lit
            if si == cs:
                seqs.append((lit, None, None, at))
                break
            off = buf[si] | (buf[si + 1] << 8)
            mlen, si = _length(buf, si + 2, tok & 0xF)
            seqs.append((lit, off, mlen + 4, at))
        out.append(seqs)
    return out


def payloads(container: bytes):
    """The chunk payloads of a container."""
    _, _, _, n_chunks = struct.unpack_from("<IQII", container, 0)
    sizes = struct.unpack_from(f"<{n_chunks}I", container, 20)
    base, out = 20 + 4 * n_chunks, []
    for cs in sizes:
        out.append(container[base:base + cs])
        base += cs
    return out


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


def rand_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(
        0, 256, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------------
# inputs with a known ideal parse
# ---------------------------------------------------------------------------

def repeats(data: bytes):
    """Ascending start positions of the 4-byte windows that occurred
    earlier in `data`."""
    a = np.frombuffer(data, np.uint8).astype(np.uint32)
    if len(a) < 4:
        return np.zeros(0, np.int64)
    w = a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24
    first = np.unique(w, return_index=True)[1]
    seen = np.ones(len(w), bool)
    seen[first] = False
    return np.flatnonzero(seen)


def norepeat(n: int, seed: int) -> bytes:
    """n seeded random bytes in which no 4-byte window occurs twice."""
    while True:
        data = rand_bytes(n, seed)
        if len(repeats(data)) == 0:
            return data
        seed += 1_000_003


def compose(parts, seed: int):
    """parts = [L0, (O1, M1), L1, (O2, M2), L2, ...]: L fresh literal bytes,
    then M bytes copied from O back (overlap allowed), alternating, ending
    on literals.  All literals come from one norepeat draw; the byte after
    a copy breaks it.  Asserted: a 4-byte window repeats an earlier one
    only where it lies wholly inside a copy, and the first window of every
    copy does, so the only matches a compressor can find are the planted
    ones, no earlier and no longer.  Returns (data, ideal_block)."""
    lits = parts[0::2]
    copies = parts[1::2]
    assert len(lits) == len(copies) + 1 and lits[0] >= 1
    assert all(n >= 1 for n in lits) and all(m >= 4 for _, m in copies)
    while True:
        pool = norepeat(sum(lits), seed)
        seed += 7919
        data, seqs, spans, at = bytearray(), [], [], 0
        broke = True
        for i, n in enumerate(lits):
            lit = pool[at:at + n]
            at += n
            if i and lit[0] == data[-copies[i - 1][0]]:
                broke = False           # the literal would extend the copy
                break
            data += lit
            if i < len(copies):
                off, m = copies[i]
                assert 1 <= off <= len(data)
                spans.append((len(data), len(data) + m))
                seqs.append((lit, off, m))
                for _ in range(m):
                    data.append(data[-off])
        if not broke:
            continue
        rep = repeats(bytes(data))
        inside = np.zeros(len(data), bool)
        for s, e in spans:
            inside[s:e - 3] = True
        if inside[rep].all() and all(s in rep for s, _ in spans):
            break
    block, raw = lz4_block(seqs, bytes(lit))
    assert raw == bytes(data)
    return raw, block


def planted(L: int, O: int, M: int, seed: int):
    """norepeat(L), M bytes copied from O back, a breaking byte and
    norepeat(20): the first repeated 4-byte window begins exactly at L.
    Returns (data, ideal_block)."""
    assert 1 <= O <= L
    return compose([L, (O, M), 21], seed)


CPU_KINDS = {
    "zeros": lambda n: bytes(n),
    "urandom": lambda n: rand_bytes(n, 5),
    "pattern123": pattern,
    "text8": text8,
}
