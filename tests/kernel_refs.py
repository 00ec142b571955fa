"""Plain references for the kernel edge tests: a bytewise CRC32C, an LZ4
block assembler, the CVLZ container packer and a pure-Python LZ4 block
decoder.  Nothing here imports the project: the references are written from
the CRC32C polynomial and the LZ4 block format alone, so agreement with the
host and device codecs is evidence and not a tautology."""
import struct

MAGIC = 0x435A4C34          # "4LZC", little-endian on the wire

# ---------------------------------------------------------------------------
# CRC32C (Castagnoli), reflected polynomial 0x82F63B78
# ---------------------------------------------------------------------------

_POLY = 0x82F63B78


def _make_table():
    table = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ _POLY if c & 1 else c >> 1
        table.append(c)
    return table


_TABLE = _make_table()


def crc32c_ref(data, init: int = 0) -> int:
    """CRC32C of `data`, one byte at a time.  `init` is the finished CRC of
    the bytes that came before, so crc32c_ref(b, crc32c_ref(a)) is the CRC
    of a + b: the convention of native.crc32c.  Meant for inputs of at most
    64 KiB."""
    crc = init ^ 0xFFFFFFFF
    for b in bytes(data):
        crc = (crc >> 8) ^ _TABLE[(crc ^ b) & 0xFF]
    return crc ^ 0xFFFFFFFF


# ---------------------------------------------------------------------------
# LZ4 block assembler
# ---------------------------------------------------------------------------

def _ext(n: int) -> bytes:
    """Extension bytes of a length field whose nibble is 15."""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


def lz4_sequence(literals: bytes, offset=None, match_len: int = 4) -> bytes:
    """One sequence: token, literal-length extension, literals and, unless
    `offset` is None (a closing literals-only sequence), the 2-byte offset
    and the match-length extension.  Nothing is validated, so this also
    assembles the malformed blocks."""
    lit = len(literals)
    tok = min(lit, 15) << 4
    out = bytearray()
    if offset is not None:
        assert match_len >= 4
        tok |= min(match_len - 4, 15)
    out.append(tok)
    if lit >= 15:
        out += _ext(lit)
    out += literals
    if offset is not None:
        out += struct.pack("<H", offset)
        if match_len - 4 >= 15:
            out += _ext(match_len - 4)
    return bytes(out)


def lz4_block(seqs, last_literals=b""):
    """Assemble [(literals, offset, match_len), ...] and the closing
    literals into one LZ4 block.  Returns (block_bytes, raw_bytes), the raw
    bytes being produced by carrying out every copy one byte at a time.
    `last_literals=None` leaves the closing sequence out, so the block ends
    on a match.  The LZ4 end-of-block rules (last five bytes literal, no
    match in the last twelve) are not enforced: a decoder has to accept any
    well-formed sequence stream."""
    block = bytearray()
    raw = bytearray()
    for literals, offset, match_len in seqs:
        block += lz4_sequence(literals, offset, match_len)
        raw += literals
        assert 0 < offset <= len(raw), "lz4_block only simulates valid matches"
        for _ in range(match_len):
            raw.append(raw[-offset])
    if last_literals is not None:
        block += lz4_sequence(last_literals)
        raw += last_literals
    return bytes(block), bytes(raw)


# ---------------------------------------------------------------------------
# CVLZ container: magic u32 | raw_size u64 | chunk_size u32 | n_chunks u32 |
# comp_size[n] u32 | chunk payloads
# ---------------------------------------------------------------------------

def cvlz(chunks, chunk_size: int, raw_size: int) -> bytes:
    out = bytearray(struct.pack("<IQII", MAGIC, raw_size, chunk_size,
                                len(chunks)))
    out += struct.pack(f"<{len(chunks)}I", *[len(c) for c in chunks])
    for c in chunks:
        out += c
    return bytes(out)


# ---------------------------------------------------------------------------
# pure-Python decoder
# ---------------------------------------------------------------------------

class Lz4RefError(ValueError):
    pass


def _read_len(block, si, n):
    """Length extension after a nibble of 15; the block may not end inside
    it."""
    while True:
        if si >= len(block):
            raise Lz4RefError("block ends inside a length extension")
        b = block[si]
        si += 1
        n += b
        if b != 255:
            return n, si


def lz4_block_decode_ref(block: bytes, cap: int) -> bytes:
    """Decode one block that must produce exactly `cap` bytes.  Raises on
    everything the host decoder rejects and on a short decode."""
    comp_n = len(block)
    out = bytearray()
    si = 0
    while si < comp_n:
        tok = block[si]
        si += 1
        lit = tok >> 4
        if lit == 15:
            lit, si = _read_len(block, si, lit)
        if len(out) + lit > cap:
            raise Lz4RefError("literals run past the chunk's raw size")
        if si + lit > comp_n:
            raise Lz4RefError("literals run past the block")
        out += block[si:si + lit]
        si += lit
        if si >= comp_n:
            break                       # the last sequence has no match
        if si + 2 > comp_n:
            raise Lz4RefError("block ends inside a match offset")
        off = block[si] | (block[si + 1] << 8)
        si += 2
        mlen = tok & 0xF
        if mlen == 15:
            mlen, si = _read_len(block, si, mlen)
        mlen += 4
        if off == 0:
            raise Lz4RefError("match offset 0")
        if off > len(out):
            raise Lz4RefError("match offset before the chunk's start")
        if len(out) + mlen > cap:
            raise Lz4RefError("match runs past the chunk's raw size")
        for _ in range(mlen):
            out.append(out[-off])
    if len(out) != cap:
        raise Lz4RefError(f"decoded {len(out)} bytes of {cap}")
    return bytes(out)


def cvlz_decode_ref(container: bytes) -> bytes:
    """Decode a whole container with lz4_block_decode_ref."""
    if len(container) < 20:
        raise Lz4RefError("short container")
    magic, raw_size, chunk_size, n = struct.unpack_from("<IQII", container, 0)
    if magic != MAGIC:
        raise Lz4RefError("bad magic")
    if len(container) < 20 + 4 * n:
        raise Lz4RefError("truncated sizes table")
    sizes = struct.unpack_from(f"<{n}I", container, 20)
    if sum(sizes) > len(container) - 20 - 4 * n:
        raise Lz4RefError("truncated payload")
    if n * chunk_size < raw_size or (n and (n - 1) * chunk_size >= raw_size):
        raise Lz4RefError("chunk table does not match raw size")
    out = bytearray()
    base = 20 + 4 * n
    for c, cs in enumerate(sizes):
        cap = min(chunk_size, raw_size - c * chunk_size)
        out += lz4_block_decode_ref(container[base:base + cs], cap)
        base += cs
    return bytes(out)
