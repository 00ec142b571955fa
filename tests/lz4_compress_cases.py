"""Crafted edge cases for the LZ4 compressors, written once against the
Arena interface.  tests/test_lz4_compress_cases.py runs them on a host
arena, where lz4_compress_block answers, and
tests/test_gpu_lz4_compress_edges.py on a device arena, where
lz4_compress_kernel does.

Nothing here imports project code: a `Ctx` carries the arena, the codec
module (its `lz4_decompress` is one of the two project decoders that must
agree with the oracle) and a 64 KiB-aligned offset base; the cases use
36 MiB of the arena from there.  The oracle for bytes is the pure-Python
decoder kernel_refs.cvlz_decode_ref; the inputs come from lz4_checks'
seeded builders, whose ideal parse is known by construction.

What the compressor may and may not do: it is free to start a planted
match late (a hash collision hides the candidate), so no case asserts the
exact parse.  Every container must decode to the input under all three
decoders, obey the end-of-block rules and the size bound; a planted match
of 24 bytes or more must make the chunk smaller than its input; and over
the dense sweeps every listed literal and match length must actually be
emitted.  A planted case whose first sequence is not the ideal one is run
again on the same shape with up to two further seeds, every run fully
checked, so that a length hidden by one collision is still produced."""
import functools
import struct

import numpy as np

from kernel_refs import cvlz_decode_ref
from lz4_checks import (CHUNK, compose, norepeat, payloads, planted,
                        rand_bytes, sequences, strict_check, text8,
                        worst_case)

G = 32                          # guard bytes either side of source and target
SRC_GUARD = bytes([0x5A]) * G
DST_GUARD = bytes([0xEE]) * G
ARENA_BYTES = 40 << 20          # what the test modules allocate
MAX_N = 16 << 20                # the per-call limit of Arena.lz4_compress
SEEDS = 3                       # runs of one planted shape, at the most


class Ctx:
    def __init__(self, arena, codec, base):
        assert base % CHUNK == 0
        self.arena, self.codec, self.base = arena, codec, base
        self.src = base + CHUNK                     # 64 KiB-aligned
        self.dst = self.src + (17 << 20) + 3        # odd residue
        assert self.dst + MAX_N + G <= ARENA_BYTES
        self.results = {}


def compress(ctx, data, at=None):
    """Write `data` between guards, compress it, and see that neither the
    source nor the guards changed."""
    at = ctx.src if at is None else at
    framed = SRC_GUARD + data + SRC_GUARD
    ctx.arena.write(at - G, framed, 0, len(framed))
    c = ctx.arena.lz4_compress(at, len(data))
    assert ctx.arena.read_bytes(at - G, len(framed)) == framed, \
        f"compress changed its source or the bytes around it (n={len(data)})"
    return c


def check(ctx, container, data, tag=""):
    n = len(data)
    try:
        strict_check(container, n)
    except (AssertionError, IndexError, struct.error) as e:
        raise AssertionError(f"{tag}: strict_check: {e!r}") from e
    try:
        ref = cvlz_decode_ref(container)
    except ValueError as e:
        raise AssertionError(f"{tag}: reference decoder: {e}") from e
    assert ref == data, f"{tag}: reference decoder gives other bytes"
    assert len(container) <= worst_case(n), f"{tag}: {len(container)} bytes"
    assert ctx.codec.lz4_decompress(container) == data, \
        f"{tag}: host decoder disagrees with the reference"
    ctx.arena.fill(ctx.dst - G, n + 2 * G, 0xEE)
    assert ctx.arena.lz4_decompress_into(ctx.dst, container) == n, tag
    got = ctx.arena.read_bytes(ctx.dst - G, n + 2 * G)
    assert got[:G] == DST_GUARD and got[G + n:] == DST_GUARD, \
        f"{tag}: lz4_decompress_into wrote outside its target"
    assert got[G:G + n] == data, \
        f"{tag}: lz4_decompress_into disagrees with the reference"


def run(ctx, data, tag, at=None):
    c = compress(ctx, data, at)
    check(ctx, c, data, tag)
    return c


# ---------------------------------------------------------------------------
# families 1-3: one planted match each
# ---------------------------------------------------------------------------

LIT_LENS = tuple(range(1, 601)) + tuple(range(770, 791))
MATCH_LENS = tuple(range(4, 601)) + tuple(range(770, 801))
PERIODS = tuple(range(1, 71))
PERIOD_PREFIXES = (20, 0)       # 0: the run starts the chunk


def _run_lens(p):
    return tuple(sorted({p + 4, 64, 259, 260, 261, 516, 1000} -
                        set(range(p + 4))))


def _shapes(family):
    """[(L, O, M)]: L literals, then M bytes at offset O, then 21
    literals."""
    if family == "literal":
        return [(L, min(L, 100), 40) for L in LIT_LENS]
    if family == "match100":
        return [(100, 100, M) for M in MATCH_LENS]
    if family == "match37":
        return [(37, 37, M) for M in MATCH_LENS]
    assert family == "period"
    # a run of R bytes of period p after `pre` literals is p literals more
    # and a match of R - p at offset p
    return [(pre + p, p, R - p) for pre in PERIOD_PREFIXES for p in PERIODS
            for R in _run_lens(p)]


PLANTED_FAMILIES = ("literal", "match100", "match37", "period")


def planted_family(ctx, family):
    """Run every shape of one family (once per Ctx) and return what the
    coverage and the recorded figures need."""
    if family in ctx.results:
        return ctx.results[family]
    res = {"lit": set(), "match": set(), "cases": 0, "exact": 0,
           "excess": 0, "reseeded": []}
    for i, (L, O, M) in enumerate(_shapes(family)):
        for attempt in range(SEEDS):
            seed = 100_000 * (PLANTED_FAMILIES.index(family) + 1) + \
                10 * i + attempt
            data, ideal = planted(L, O, M, seed)
            tag = f"planted(L={L}, O={O}, M={M}, seed={seed})"
            c = run(ctx, data, tag)
            seqs = sequences(c)[0]
            payload = payloads(c)[0]
            if M >= 24:
                # ideally the match saves M bytes for at most 7; a start
                # 16 bytes late still leaves a saving
                assert len(payload) < len(data), \
                    f"{tag}: {len(payload)} bytes for {len(data)}: " \
                    f"the match was not used, sequences {seqs}"
            res["lit"].update(s[0] for s in seqs)
            res["match"].update(s[2] for s in seqs if s[2] is not None)
            res["excess"] = max(res["excess"], len(payload) - len(ideal))
            exact = seqs[0][:3] == (L, O, M)
            if attempt == 0:
                res["cases"] += 1
                res["exact"] += exact
            if exact:
                assert payload == ideal, f"{tag}: ideal parse, other bytes"
                break
            if attempt == 0:
                res["reseeded"].append((L, O, M))
    ctx.results[family] = res
    return res


def coverage(ctx):
    """Every listed literal length and match length was emitted by this
    arena's compressor somewhere in families 1-3."""
    lit, match = set(), set()
    for family in PLANTED_FAMILIES:
        res = planted_family(ctx, family)
        lit |= res["lit"]
        match |= res["match"]
    missing_lit = sorted(set(LIT_LENS) - lit)
    missing_match = sorted(set(MATCH_LENS) - match)
    assert not missing_lit and not missing_match, \
        f"never emitted: literal lengths {missing_lit}, " \
        f"match lengths {missing_match}"


def recorded(ctx):
    """The figures that are recorded and not asserted."""
    out = {}
    for family in PLANTED_FAMILIES:
        res = planted_family(ctx, family)
        out[family] = {"cases": res["cases"], "exact": res["exact"],
                       "max_payload_minus_ideal": res["excess"],
                       "reseeded": res["reseeded"]}
    out["cases"] = sum(v["cases"] for v in out.values())
    out["exact"] = sum(out[f]["exact"] for f in PLANTED_FAMILIES)
    out["exact_share"] = round(out["exact"] / out["cases"], 4)
    out["max_payload_minus_ideal"] = max(
        out[f]["max_payload_minus_ideal"] for f in PLANTED_FAMILIES)
    return out


# ---------------------------------------------------------------------------
# family 4: literal store alignment
# ---------------------------------------------------------------------------

def store_alignment(ctx):
    """A literal run of 256 bytes or more is stored 16 bytes per lane once
    its destination is aligned.  A first sequence of 16..31 literals moves
    the long run through every residue of its position in the block, which
    is the residue of the device store address: slots are 64-byte
    aligned."""
    residues = set()
    for L1 in range(16, 32):
        for L2 in (256, 300, 1000):
            seed = 500_000 + 10 * L1 + L2
            data, _ = compose([L1, (L1, 8), L2, (100, 40), 21], seed)
            tag = f"store_alignment(L1={L1}, L2={L2})"
            c = run(ctx, data, tag)
            assert len(payloads(c)[0]) < len(data), tag
            residues.update(at % 16 for lit, _, _, at in sequences(c)[0]
                            if lit >= 256)
    assert residues == set(range(16)), \
        f"long literal runs never stored at residues " \
        f"{sorted(set(range(16)) - residues)}"


# ---------------------------------------------------------------------------
# families 5 and 6: source residue, chunk independence, determinism
# ---------------------------------------------------------------------------

MIXED_N = 2 * CHUNK + 13


@functools.lru_cache(maxsize=None)
def mixed():
    """2 x 65536 + 13 bytes: planted matches, period runs and text8 by
    turns, one planted piece laid over each chunk boundary."""
    rng = np.random.default_rng(600)
    out = bytearray()
    i = 0
    while len(out) < MIXED_N:
        kind = i % 4
        if kind == 0:
            L = int(rng.choice((1, 14, 15, 16, 255, 256, 257, 270, 525)))
            M = int(rng.choice((4, 18, 19, 20, 260, 274, 516, 529)))
            out += planted(L, min(L, 100), M, 600 + i)[0]
        elif kind == 1:
            p = int(rng.integers(1, 71))
            R = int(rng.choice((64, 259, 260, 261, 516, 1000)))
            if R >= p + 4:
                out += compose([20 + p, (p, R - p), 21], 600 + i)[0]
        else:
            out += text8(int(rng.integers(500, 4000)), seed=600 + i)
        i += 1
    for b in (CHUNK, 2 * CHUNK):
        piece = planted(300, 100, 274, 700 + b)[0]
        at = b - 330                    # the match straddles the boundary
        out[at:at + min(len(piece), MIXED_N - at)] = \
            piece[:min(len(piece), MIXED_N - at)]
    return bytes(out[:MIXED_N])


def source_residue(ctx):
    """The same bytes at every residue mod 16 and either side of a 64 KiB
    boundary: byte-identical containers."""
    data = mixed()
    first = run(ctx, data, "mixed at residue 0")
    offsets = [ctx.src + r for r in range(1, 16)] + \
        [ctx.src + CHUNK - 5, ctx.src + CHUNK + 5]
    for at in offsets:
        assert compress(ctx, data, at) == first, \
            f"container depends on the source offset: {at - ctx.src}"


def chunk_independence(ctx):
    """Three calls give the same bytes, and each chunk's payload is what
    the same bytes give when compressed alone."""
    data = mixed()
    whole = run(ctx, data, "mixed")
    for _ in range(2):
        assert compress(ctx, data) == whole, "two calls, two containers"
    parts = payloads(whole)
    assert len(parts) == 3
    for c, part in enumerate(parts):
        piece = data[c * CHUNK:(c + 1) * CHUNK]
        alone = run(ctx, piece, f"mixed chunk {c} alone", ctx.src + 7)
        assert payloads(alone) == [part], \
            f"chunk {c} compresses differently inside the 3-chunk call"


# ---------------------------------------------------------------------------
# family 7: chunk ends
# ---------------------------------------------------------------------------

def _end_match(cn, start, end, seed, head=None):
    """cn bytes whose only repeat starts at `start` and would run to `end`;
    None where the shape does not exist."""
    if start < 1 or end - start < 4 or end > cn:
        return None
    O = min(start, 9)
    if end == cn:
        # the copy runs into the last byte: no breaking literal follows
        data = bytearray(norepeat(start, seed))
        for _ in range(cn - start):
            data.append(data[-O])
        return bytes(data)
    return compose([start, (O, end - start), cn - end], seed)[0]


def small_chunk_ends(ctx):
    """Every chunk length 0..40 on zeros, period 3 and a planted match that
    presses on both end-of-block rules: no match starts in the last 12
    bytes, none ends in the last 5."""
    for cn in range(0, 41):
        datas = {"zeros": bytes(cn), "period3": (b"xyz" * 14)[:cn]}
        for start in range(cn - 14, cn - 10):
            for end in list(range(cn - 6, cn - 2)) + [cn]:
                d = _end_match(cn, start, end, 7000 + cn)
                if d is not None:
                    datas[f"match {start}..{end}"] = d
        for name, data in datas.items():
            assert len(data) == cn
            run(ctx, data, f"cn={cn} {name}")


_END_SHAPES = [(s, e) for s in (14, 13, 12, 11) for e in (6, 5, 4, 3)]


def full_chunk_ends(ctx, kind):
    """n = 65536 + k for k in 0..20: a full chunk followed by one of k
    bytes."""
    for k in range(21):
        n = CHUNK + k
        if kind == "zeros":
            data = bytes(n)
        elif kind == "period3":
            data = (b"xyz" * (n // 3 + 1))[:n]
        else:
            # random bytes; the first chunk ends on a planted match that
            # starts 14..11 and stops 6..3 bytes before the chunk's end
            # (k = 16..20: runs into its last byte), the second chunk is
            # the same piece cut to k bytes
            s, e = _END_SHAPES[k % 16]
            end = CHUNK if k >= 16 else CHUNK - e
            tail = _end_match(200, 200 - s, 200 - (CHUNK - end), 7100 + k)
            first = rand_bytes(CHUNK - 200, 7200 + k) + tail
            data = first + tail[:k]
        assert len(data) == n
        run(ctx, data, f"{kind} n=65536+{k}")


END_KINDS = ("zeros", "period3", "planted")


# ---------------------------------------------------------------------------
# family 8: the largest call
# ---------------------------------------------------------------------------

def largest_call(ctx, n):
    """256 chunks.  Each holds seeded random bytes stamped with its index
    and a 4 KiB region repeating a 64-byte motif, so a chunk that lands in
    another's slot, or is dropped, changes the bytes; the matches add up to
    about 1 MiB, which keeps the pure-Python decode short."""
    assert (n + CHUNK - 1) // CHUNK == 256
    a = np.random.default_rng(800).integers(0, 256, n, dtype=np.uint8)
    for c in range(256):
        lo = c * CHUNK
        cn = min(CHUNK, n - lo)
        stamp = np.frombuffer(struct.pack("<I", 0xC0DE0000 + c), np.uint8)
        a[lo:lo + min(4, cn)] = stamp[:cn]
        at = 64 + (c * 241) % (CHUNK - 4096 - 64)
        if at + 4096 <= cn:
            a[lo + at:lo + at + 4096] = np.tile(a[lo + at:lo + at + 64], 64)
    data = a.tobytes()
    c = run(ctx, data, f"largest call n={n}")
    # a chunk with a motif region saves 4096 - 64 bytes less the match's
    # own cost (under 30) and pays at most cn / 255 + 16 = 273 for its
    # literals: 3700 net at the least, in 255 chunks; the header is 1044
    assert len(c) < n - 255 * 3500, f"n={n}: {len(c)} bytes, motifs not found"
