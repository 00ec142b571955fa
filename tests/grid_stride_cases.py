"""Shared cases for the grid-stride tests (host arena and MI355X): every
tiled typed, token and array kernel run with more tiles than workgroups.

The tiled kernels walk their tile table with

    for (tile = blockIdx.x; tile < n_tiles; tile += gridDim.x)

under a grid of min(n_tiles, TILE_GRID_CAP).  Each case here is one call of
at least 2 * CAP + 300 tiles built from tiny items, so tiles i, i + CAP and
i + 2 * CAP run in one workgroup: the first 300 workgroups take three trips,
the rest two.  What a case holds to, and asserts in Python before it runs:

  own slot          every tile writes into a slot of its own in a
                    sentinel-filled destination, at least 16 guard bytes on
                    either side; the whole destination is compared, so a trip
                    not taken leaves sentinel and a trip done with the wrong
                    tile writes outside its slot
  partners differ   the items of tiles i and i + CAP differ in dtype pair
                    (where one call mixes pairs), source residue mod 16,
                    destination residue and length; the choices follow
                    i % CAP and i // CAP, never i % k alone (CAP is a power
                    of two)
  straddling items  multi-tile items lie across tile indices CAP-1 | CAP and
                    2*CAP-1 | 2*CAP, so a non-zero tile_off is consumed on a
                    later trip
  content per item  disjoint slices of one seeded random pool

The tile counts come from the items and the exported tile constants, never
from the module.  Expected values come from torch on the CPU, numpy and the
reference helpers of the other *_cases files; every comparison is bitwise
and every input finite.  A host arena runs the same items through the host
twins, which proves the builders and references; only a device arena has
workgroups and trips."""
import numpy as np
import torch

from safetensors_cases import ISZ, TORCH, expected, from_raw
from safetensors_save_cases import finite_raw
import safetensors_fp8_cases as f8c
import token_window_cases as tc

SENTINEL = 0xAB
GUARD = 16
EXTRA = 300                     # workgroups that take a third trip
ARENA_BYTES = 64 << 20


class Tier:
    """The arena under test and the memory on its side: cpu tensors for a
    host arena (device -1), cuda tensors for a device arena."""

    def __init__(self, native, arena, device):
        self.native, self.arena, self.device = native, arena, device
        self.mod = native.load()
        self.D = native.DTYPES
        self.CAP = self.mod.TILE_GRID_CAP
        self.tdev = "cpu" if device < 0 else f"cuda:{device}"
        assert arena.base_ptr() % 16 == 0

    def put(self, img):
        """a uint8 image as a tensor on this side, on the 16-byte grid"""
        t = torch.from_numpy(np.ascontiguousarray(img)).to(self.tdev)
        assert t.data_ptr() % 16 == 0
        return t

    def get(self, t):
        return t.cpu().numpy()

    def arena_put(self, off, img):
        assert off % 16 == 0 and off + len(img) <= ARENA_BYTES
        self.arena.write(off, np.ascontiguousarray(img).tobytes())

    def arena_get(self, off, n):
        return np.frombuffer(self.arena.read_bytes(off, n), dtype=np.uint8)


# ------------------------------------------------------------------ planning

def pick(options, start, taken=()):
    """options[start], or the next one that no partner has taken"""
    for k in range(len(options)):
        v = options[(start + k) % len(options)]
        if v not in taken:
            return v
    raise AssertionError("no option left that differs from the partners")


def lay_tiles(CAP, make, bigs=None, n_min=None):
    """Items in tile order until the call has n_min tiles.  make(tile, r,
    trip, big, partners) returns the item (a dict) whose first tile is
    `tile` = trip * CAP + r; `big` is None for a one-tile item or the number
    of tiles of the multi-tile item that starts here; `partners` are the
    items that own the tiles CAP before this item's.  Returns (items,
    owner) with owner[tile] the index of the item the tile belongs to."""
    n_min = 2 * CAP + EXTRA + 4 if n_min is None else n_min
    bigs = {CAP - 1: 3, 2 * CAP - 2: 3} if bigs is None else bigs
    items, owner = [], []
    tile = 0
    while tile < n_min:
        k = bigs.get(tile, 1)
        seen, partners = set(), []
        for t in range(tile, tile + k):
            if t >= CAP and owner[t - CAP] not in seen:
                seen.add(owner[t - CAP])
                partners.append(items[owner[t - CAP]])
        it = make(tile, tile % CAP, tile // CAP, bigs.get(tile), partners)
        it["tile"], it["tiles"] = tile, k
        items.append(it)
        owner += [len(items) - 1] * k
        tile += k
    return items, owner


def check_plan(CAP, items, owner, counted, keys, straddle=True):
    """What every case asserts of its own item list: the tile count (counted
    by the case from its items and the tile constants), partners that
    differ in every key, and the straddling items."""
    assert counted == [it["tiles"] for it in items]
    n_tiles = sum(counted)
    assert n_tiles == len(owner) and n_tiles >= 2 * CAP + EXTRA
    for t in range(n_tiles - CAP):
        a, b = items[owner[t]], items[owner[t + CAP]]
        assert a is not b
        for k in keys:
            assert a[k] != b[k], (k, t, a[k])
    if straddle:
        for edge in (CAP, 2 * CAP):
            it = items[owner[edge]]
            assert owner[edge - 1] == owner[edge] and it["tile"] < edge, edge
    return n_tiles


def slots(sizes, residues):
    """Byte offsets of own slots on the 16-byte grid: item k lies `residues
    [k]` bytes past a 16-byte boundary with at least GUARD bytes that belong
    to nothing else before and after it.  Returns (offsets, total)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    residues = np.asarray(residues, dtype=np.int64)
    span = (GUARD + residues + sizes + GUARD + 15) // 16 * 16
    base = np.concatenate([[0], np.cumsum(span)])
    return base[:-1] + GUARD + residues, int(base[-1])


def image(total, offs, chunks, fill=SENTINEL):
    img = np.full(total, fill, dtype=np.uint8)
    for o, c in zip(offs, chunks):
        img[o:o + len(c)] = c
    return img


def check_image(what, CAP, got, exp, items, offs, sizes):
    """The whole destination, byte for byte: written slots, guards and every
    byte between.  On a mismatch says whose slot it is and whether the slot
    still holds the sentinel (a trip that was not taken)."""
    if np.array_equal(got, exp):
        return
    b = int(np.nonzero(got != exp)[0][0])
    untouched = [it["tile"] for it, o, n in zip(items, offs, sizes)
                 if n and (got[o:o + n] == SENTINEL).all()
                 and not (exp[o:o + n] == SENTINEL).all()]
    k = max(int(np.searchsorted(np.asarray(offs), b, side="right")) - 1, 0)
    where = "in its slot" if offs[k] <= b < offs[k] + sizes[k] else \
        "outside every slot"
    raise AssertionError(
        f"{what}: byte {b} is {got[b]:#x}, expected {exp[b]:#x}, {where}: "
        f"item {k}, first tile {items[k]['tile']} = "
        f"{items[k]['tile'] // CAP} * CAP + {items[k]['tile'] % CAP}; "
        f"{len(untouched)} slots still hold only the sentinel, tile indices "
        f"{untouched[:3]} .. {untouched[-3:]}")


def pool_slices(items, key, counts, make):
    """Content per item: for every value of it[key] one pool make(value,
    total) of bytes, cut into disjoint slices of counts[k] bytes."""
    out = [None] * len(items)
    for v in sorted({it[key] for it in items}):
        idx = [k for k, it in enumerate(items) if it[key] == v]
        pool = np.frombuffer(make(v, sum(counts[k] for k in idx)), np.uint8)
        at = 0
        for k in idx:
            out[k] = pool[at:at + counts[k]]
            at += counts[k]
    return out


# ------------------------------------------------- a, b, c: cast segments

PLAIN_PAIRS = (("F32", "BF16"), ("F32", "F16"), ("BF16", "F32"),
               ("F16", "BF16"), ("F8_E4M3", "F32"), ("F8_E5M2", "BF16"),
               ("I8", "I8"), ("I64", "I64"))
BIG_PAIRS = (("F32", "BF16"), ("BF16", "F32"), ("F16", "BF16"))
QUANT_PAIRS = (("F32", "F8_E4M3"), ("F16", "F8_E4M3"), ("BF16", "F8_E4M3"))
DEQUANT_PAIRS = (("F8_E4M3", "F32"), ("F8_E4M3", "F16"), ("F8_E4M3", "BF16"))
# short runs (element-wise path) and runs of CAST_SHORT_RUN = 64 and more
PLAIN_LENS = tuple(range(1, 41)) + (64, 65, 79, 100)
EVERY = (0, 8, 67)
SCALED_LENS = {0: (64, 65, 70, 96, 130, 133, 5, 33),
               8: tuple(range(1, 41)),
               67: (64, 65, 67, 70, 96, 130, 133, 5, 33)}


def residue_options(align):
    return tuple(range(0, 16, align))


def cast_tiles_of(n, pair, cast_tile):
    """tiles of one segment: a converting pair tiles by CAST_TILE elements, a
    same-dtype copy is flattened to bytes and tiles by 4 * CAST_TILE"""
    s, d = pair
    if s == d:
        return -(-n * ISZ[s] // (4 * cast_tile))
    return -(-n // cast_tile)


def item_scale(tile):
    """binades apart from the partner's (CAP is no multiple of 23)"""
    return 2.0 ** ((tile % 23) - 11) * 1.37


def plan_cast(tier, store, scaled):
    CAP, cast_tile = tier.CAP, tier.mod.CAST_TILE
    pairs = PLAIN_PAIRS if not scaled else \
        (QUANT_PAIRS if store else DEQUANT_PAIRS)

    def make(tile, r, trip, big, partners):
        def taken(key):
            return {p[key] for p in partners}
        it = {}
        it["pair"] = pick(pairs if not (big and not scaled) else BIG_PAIRS,
                          r + 3 * trip + (1 if big else 0), taken("pair"))
        s, d = it["pair"]
        if scaled:
            it["every"] = pick(EVERY, r + trip, taken("every") if not big
                               else {0, 8})
            it["e0"] = 1 + (3 * r + 5 * trip) % 61
            it["scale"] = item_scale(tile)
        if big:
            assert s != d
            it["n"] = pick((2 * cast_tile + 3, 2 * cast_tile + 5), trip,
                           taken("n"))
        else:
            lens = SCALED_LENS[it["every"]] if scaled else PLAIN_LENS
            it["n"] = pick(lens, 7 * r + 11 * trip, taken("n"))
        # a load reads the arena at any byte, a store reads a tensor at its
        # itemsize; destinations are aligned to their itemsize
        it["sres"] = pick(residue_options(ISZ[s] if store else 1),
                          5 * r + 7 * trip, taken("sres"))
        it["dres"] = pick(residue_options(ISZ[d]), 3 * r + 5 * trip,
                          taken("dres"))
        return it

    items, owner = lay_tiles(CAP, make)
    counted = [cast_tiles_of(it["n"], it["pair"], cast_tile) for it in items]
    keys = ["pair", "sres", "dres", "n"] + (["scale"] if scaled else [])
    check_plan(CAP, items, owner, counted, keys)
    assert {it["pair"] for it in items} >= set(pairs)
    if not store:
        assert {it["sres"] for it in items} == set(range(16))
    if scaled:
        for t in range(len(owner) - CAP):
            a, b = items[owner[t]]["scale"], items[owner[t + CAP]]["scale"]
            assert max(a, b) / min(a, b) >= 2.0
        assert {it["every"] for it in items} == set(EVERY)
        assert all(it["e0"] for it in items)
    return items


def scaled_groups(items):
    """The f32 scales of the scaled items: item k reads groups 0 .. g1 of
    its own array (the groups before scale_e0's exist and are never read),
    each group a different multiple of the item's scale.  Returns (all
    scales, first index of each item, group index of every element)."""
    start, scales, idx = [], [], []
    at = 0
    for it in items:
        e = it["e0"] + np.arange(it["n"], dtype=np.int64)
        g = e // it["every"] if it["every"] else np.zeros_like(e)
        n_g = int(g[-1]) + 1
        scales.append(np.float32(it["scale"]) *
                      (1 + 0.25 * (np.arange(n_g) % 4)).astype(np.float32))
        start.append(at)
        idx.append(at + g)
        at += n_g
    return np.concatenate(scales).astype(np.float32), start, idx


def cast_contents(items, scaled, store, scales, idx):
    """(source bytes, expected destination bytes) of every item"""
    rng = np.random.default_rng(101 + 2 * scaled + store)
    sb = [it["n"] * ISZ[it["pair"][0]] for it in items]
    S = torch.from_numpy(scales) if scaled else None

    if scaled and store:
        # values that land all over e4m3's range once divided by their scale
        def make(pair, total):
            ks = [k for k, it in enumerate(items) if it["pair"] == pair]
            sc = scales[np.concatenate([idx[k] for k in ks])]
            v = rng.standard_normal(len(sc)).astype(np.float32) * sc * \
                np.exp2(rng.integers(-8, 10, len(sc))).astype(np.float32)
            v = np.clip(v, -60000.0, 60000.0)
            t = torch.from_numpy(v).to(TORCH[pair[0]])
            assert bool(torch.isfinite(t.float()).all())
            return t.view(torch.uint8).numpy().tobytes()
    else:
        def make(pair, total):
            return finite_raw(rng, pair[0], total // ISZ[pair[0]])

    src = pool_slices(items, "pair", sb, make)
    exp = [None] * len(items)
    for pair in sorted({it["pair"] for it in items}):
        s, d = pair
        ks = [k for k, it in enumerate(items) if it["pair"] == pair]
        raw = np.concatenate([src[k] for k in ks]).tobytes()
        if s == d:
            out = np.frombuffer(raw, np.uint8)
        else:
            if not scaled:
                t = expected(raw, s, d)
            else:
                gi = torch.from_numpy(np.concatenate([idx[k] for k in ks]))
                x = from_raw(raw, s)
                t = f8c.flat_quant(x, S, gi) if store else \
                    f8c.flat_dequant(x, S, gi, TORCH[d])
            assert not bool(torch.isnan(t.float()).any())
            out = t.contiguous().view(torch.uint8).numpy()
        at = 0
        for k in ks:
            nb = items[k]["n"] * ISZ[d]
            exp[k] = out[at:at + nb]
            at += nb
        assert at == len(out)
    return src, exp


def case_cast(tier, store, scaled=False, block=False):
    """Arena.convert_ptr (store False) or Arena.store_ptr (store True) with
    7-tuples, with 10-tuples under given group scales, or (block) with
    14-tuples under given tile scales, see plan_block_cast.

    Own slot: sources and destinations each lie in a slot of their own, 16
    sentinel bytes or more around every destination, the whole destination
    image compared.  Partners differ in dtype pair, source residue,
    destination residue and length (and, scaled, in their scale by two
    binades or more).  A 2 * CAST_TILE + 3 and a 2 * CAST_TILE + 5 element
    segment straddle tiles CAP-1 | CAP and 2*CAP-1 | 2*CAP.  Plain: the
    pairs cycle over F32->BF16, F32->F16, BF16->F32, F16->BF16, F8_E4M3->F32,
    F8_E5M2->BF16, I8->I8, I64->I64; a load's sources cover every residue
    mod 16, a store's every multiple of the itemsize.  Scaled: F32 / F16 /
    BF16 -> F8_E4M3 (store) or back (load), every item under scales of its
    own, 2**((tile % 23) - 11) * 1.37 times a factor per group, scale_every
    cycling over 0, 8 (element-wise branch) and 67 (runs of 64 and more, cut
    where a group ends), scale_e0 never 0: a scale kept from the tile before
    changes bits."""
    CAP, D = tier.CAP, tier.D
    if block:
        scaled = True
        items = plan_block_cast(tier, store)
        scales, start, idx = block_groups(items)
    else:
        items = plan_cast(tier, store, scaled)
        scales, start, idx = scaled_groups(items) if scaled else \
            (None, None, None)
    src, exp = cast_contents(items, scaled, store, scales, idx)
    s_offs, s_total = slots([len(c) for c in src], [it["sres"] for it in items])
    d_offs, d_total = slots([len(c) for c in exp], [it["dres"] for it in items])
    s_img = image(s_total, s_offs, src, fill=0x5A)
    exp_img = image(d_total, d_offs, exp)
    blank = np.full(d_total, SENTINEL, dtype=np.uint8)
    if store:
        sbuf = tier.put(s_img)
        tier.arena_put(0, blank)
        a0, b0 = sbuf.data_ptr(), 0
    else:
        tier.arena_put(0, s_img)
        dbuf = tier.put(blank)
        a0, b0 = 0, dbuf.data_ptr()
    if scaled:
        scale_buf = tier.put(scales.view(np.uint8))
    segs = []
    for k, it in enumerate(items):
        s, d = it["pair"]
        seg = (a0 + int(s_offs[k]), b0 + int(d_offs[k]), 1, it["n"],
               it["n"] * ISZ[s], D[s], D[d])
        if block:
            seg = seg[:2] + (it["M"], it["K"], it["K"] * ISZ[s], D[s], D[d],
                             scale_buf.data_ptr() + 4 * start[k], 0, it["K"],
                             it["M"], it["K"], it["bm"], it["bn"])
        elif scaled:
            seg += (scale_buf.data_ptr() + 4 * start[k], it["every"],
                    it["e0"])
        segs.append(seg)
    (tier.arena.store_ptr if store else tier.arena.convert_ptr)(segs)
    got = tier.arena_get(0, d_total) if store else tier.get(dbuf)
    what = ("store_ptr" if store else "convert_ptr") + \
        (" block" if block else " scaled" if scaled else "")
    check_image(what, CAP, got, exp_img, items, d_offs,
                [len(c) for c in exp])
    if store:
        assert np.array_equal(tier.get(sbuf), s_img), "a source changed"
    else:
        assert np.array_equal(tier.arena_get(0, s_total), s_img), \
            "a source changed"


# -------------------------------------------------------- g: token windows

TOKEN_T = 9
TOKEN_PAIRS = (("U16", "I32"), ("I32", "I64"))
VOCAB = 1000


class WindowCall(tc.Call):
    """token_window_cases.Call with the sources gathered into one image and
    written to the arena once."""

    def start(self, total):
        self.src_img = np.full(total, 0x5A, dtype=np.uint8)

    def place(self, off, tokens):
        raw = np.frombuffer(tokens.tobytes(), np.uint8)
        self.src_img[off:off + len(raw)] = raw


def case_token_windows(tier, src, dst):
    """Arena.token_windows, one piece per tile, 2 * CAP + 304 pieces of 1 to
    10 tokens in windows of T = 9.

    Own slot: piece k lies in row 2k + 1 of x and y, so a whole untouched
    row (36 or 72 bytes) separates two pieces, the pieces cover only part of
    their row, and x and y are compared whole, guards included.  Partners
    differ in source residue mod 16, destination residue (row, j0), j0 and
    length; the dtype pair is the call's.  No piece can straddle a trip: a
    piece holds at most T + 1 tokens, one tile (multi-tile pieces are
    token_window_cases.case_long's).  Vocabulary: with r = tile % CAP, ids
    outside [0, 1000) lie in no tile of the workgroups r % 4 == 0, in the
    first-trip tile only of r % 4 == 1, in the second-trip tile only of
    r % 4 == 2, in both of r % 4 == 3, and in the third-trip tile of every
    third workgroup; the returned count equals the reference's exactly, a
    second call with vocab_size 0 returns 0."""
    CAP, T = tier.CAP, TOKEN_T
    ss, ds = np.dtype(tc.NP_SRC[src]).itemsize, np.dtype(tc.NP_DST[dst]).itemsize
    lead = GUARD + ds
    shapes = tuple((j0, n) for j0 in range(T + 1)
                   for n in range(1, T + 2 - j0))

    def make(tile, r, trip, big, partners):
        it = {"row": 2 * len_items[0] + 1}
        len_items[0] += 1
        tj = {p["j0"] for p in partners} | {None}
        tn = {p["n"] for p in partners}
        for k in range(len(shapes)):
            j0, n = shapes[(7 * r + 11 * trip + k) % len(shapes)]
            dres = (lead + (it["row"] * T + j0) * ds) % 16
            if j0 not in tj and n not in tn and \
                    dres not in {p["dres"] for p in partners}:
                break
        else:
            raise AssertionError("no shape left that differs")
        it.update(j0=j0, n=n, dres=dres)
        it["sres"] = pick(range(16), 5 * r + 7 * trip,
                          {p["sres"] for p in partners})
        it["bad"] = (r % 4 in (1, 3)) if trip == 0 else \
            (r % 4 in (2, 3)) if trip == 1 else r % 3 == 0
        return it

    len_items = [0]
    items, owner = lay_tiles(CAP, make, bigs={})
    tile_tokens = tier.mod.TOKEN_TILE
    counted = [-(-it["n"] // tile_tokens) for it in items]
    check_plan(CAP, items, owner, counted, ["sres", "dres", "j0", "n"],
               straddle=False)
    seen = {(items[owner[r]]["bad"], items[owner[r + CAP]]["bad"])
            for r in range(CAP)}
    assert seen == {(False, False), (True, False), (False, True), (True, True)}
    assert {items[owner[2 * CAP + r]]["bad"] for r in range(EXTRA)} == \
        {False, True}

    rng = np.random.default_rng(211)
    offenders = [VOCAB] + [v for v in tc.SPECIALS[src] if v < 0 or v >= VOCAB]
    s_offs, s_total = slots([it["n"] * ss for it in items],
                            [it["sres"] for it in items])
    results = []
    for vocab in (VOCAB, 0):
        c = WindowCall(tier.arena, tier.D, tier.tdev, src, dst, T,
                       rows=2 * len(items) + 1)
        c.start(s_total)
        for k, it in enumerate(items):
            t = tc.make_tokens(rng, src, it["n"], below=VOCAB)
            if it["bad"]:
                for q in range(1 + k % it["n"]):
                    t[(k + 3 * q) % it["n"]] = offenders[(k + q) % len(offenders)]
            c.place(int(s_offs[k]), t)
            c.piece(int(s_offs[k]), it["row"], it["j0"], t)
        tier.arena_put(0, c.src_img)
        results.append(c.run(vocab=vocab))
    assert results[0] >= CAP and results[1] == 0


# --------------------------------------------------------- d: absmax scales

ABSMAX_SRC = ("F32", "F16", "BF16")
# (rows, run, elements between two runs, scale_every): runs and groups of
# CAST_SHORT_RUN = 64 and more reduce by run with one commit per group and
# tile, everything else goes element-wise; rows * run differs in each
ABSMAX_SHAPES = ((1, 64, 0, 0), (1, 100, 0, 64), (2, 67, 5, 67),
                 (1, 130, 0, 67), (2, 64, 0, 0), (1, 96, 0, 64),
                 (1, 5, 0, 0), (3, 7, 2, 8), (2, 33, 3, 8), (1, 40, 0, 0),
                 (4, 9, 0, 8), (1, 1, 0, 0))
ABSMAX_SHARED = range(40, 104)  # workgroups whose tiles meet in one slot
PREFILL = 7.0


def case_absmax(tier):
    """native.absmax_scales, one segment per tile, each with slots of its
    own in an f32 array pre-filled with 7.0.

    Own slot: at least one float that belongs to no segment lies between
    two slot ranges, so merge_scale_slots merges nothing, scale_slots_kernel
    gets more than 2 * CAP ranges for its zeroing and its finishing pass, and
    the whole array is compared: the gaps still read 7.0, a group nobody
    reduced into reads 2**-40 / 448.  Partners differ in source dtype,
    source residue, slot residue and length.  Leaks: with r = tile % CAP the
    segments of the first-trip tiles with r // 2 even hold one value of
    3e4 and nothing else above 1e-3, the others nothing above 1e-3, and
    every later tile is the opposite of its partner, so
    a maximum carried into the next tile in `m` or through `lds` changes the
    partner's scale; the elements between the runs of a strided segment
    hold 6e4.  The tiles of workgroups 40 .. 103 share one slot across
    their trips (scale_every 0, same out_ptr) and meet in one atomicMax; they
    alone keep their partner's slot residue.  Both branches: runs and groups
    of 64 and more (several commits per tile), and short runs or groups.
    Segments of 2 * CAST_TILE + 3 and + 5 elements under groups of 67
    straddle tiles CAP-1 | CAP and 2*CAP-1 | 2*CAP."""
    CAP, D, cast_tile = tier.CAP, tier.D, tier.mod.CAST_TILE

    def make(tile, r, trip, big, partners):
        def taken(key):
            return {p[key] for p in partners}
        it = {"dt": pick(ABSMAX_SRC, r + trip, taken("dt"))}
        shared = not big and r in ABSMAX_SHARED
        if big:
            shape = (1, pick((2 * cast_tile + 3, 2 * cast_tile + 5), trip,
                             taken("n")), 0, 67)
        else:
            shapes = [s for s in ABSMAX_SHAPES if s[3] == 0 or not shared]
            shape = pick([s for s in shapes if s[0] * s[1] not in taken("n")],
                         7 * r + 11 * trip)
        it["rows"], it["run"], it["gap"], it["every"] = shape
        it["n"] = it["rows"] * it["run"]
        it["e0"] = 0 if shared else (3 * r + 5 * trip) % 50
        it["groups"] = (it["e0"] + it["n"] - 1) // it["every"] + 1 \
            if it["every"] else 1
        it["sres"] = pick(residue_options(ISZ[it["dt"]]), 5 * r + 7 * trip,
                          taken("sres"))
        it["share"] = partners[0] if shared and partners else None
        it["ores"] = it["share"]["ores"] if it["share"] else \
            pick(range(4), r + 3 * trip, taken("ores"))
        assert len(taken("hi")) <= 1
        it["hi"] = not partners[0]["hi"] if partners else (r // 2) % 2 == 0
        it["hi_at"] = (7 * r + trip) % it["n"]
        return it

    items, owner = lay_tiles(CAP, make)
    counted = [-(-it["n"] // cast_tile) for it in items]
    n_tiles = check_plan(CAP, items, owner, counted, ["dt", "sres", "n", "hi"])
    shared = 0
    for t in range(n_tiles - CAP):
        a, b = items[owner[t]], items[owner[t + CAP]]
        assert (b["share"] is a) == (t % CAP in ABSMAX_SHARED)
        assert (a["ores"] != b["ores"]) == (b["share"] is None)
        shared += b["share"] is a
    assert shared == len(ABSMAX_SHARED) * 2
    by_run = [it["run"] >= 64 and (it["every"] == 0 or it["every"] >= 64)
              for it in items]
    assert {(w, o // CAP) for w, o in zip(by_run, [it["tile"] for it in items])
            } == {(w, t) for w in (False, True) for t in (0, 1, 2)}

    # slots: a gap of one float or more before every range
    at = 0
    for it in items:
        if it["share"]:
            it["out"] = it["share"]["out"]
            continue
        at += 1
        at += (it["ores"] - at) % 4
        it["out"] = at
        at += it["groups"]
    n_out = at + 1
    ranges = sorted({(it["out"], it["groups"]) for it in items})
    assert len(ranges) > 2 * CAP
    assert all(a + n < b for (a, n), (b, _m) in zip(ranges, ranges[1:]))

    # sources
    rng = np.random.default_rng(307)
    ext = [(it["rows"] - 1) * (it["run"] + it["gap"]) + it["run"]
           for it in items]

    def make_pool(dt, total):
        n = total // ISZ[dt]
        v = (1e-6 + rng.random(n) * 9e-4) * rng.choice([-1.0, 1.0], n)
        return v.astype(np.float32)
    sel, gidx = [], []
    for k, it in enumerate(items):
        s = (np.arange(it["rows"])[:, None] * (it["run"] + it["gap"]) +
             np.arange(it["run"])[None, :]).ravel()
        e = it["e0"] + np.arange(it["n"])
        sel.append(s)
        gidx.append(it["out"] + (e // it["every"] if it["every"] else 0 * e))
    src = [None] * len(items)
    amax = torch.zeros(n_out)
    for dt in ABSMAX_SRC:
        ks = [k for k, it in enumerate(items) if it["dt"] == dt]
        v = make_pool(dt, sum(ext[k] for k in ks) * ISZ[dt])
        at, where, groups = 0, [], []
        for k in ks:
            it = items[k]
            run_at = at + sel[k]
            gaps = np.setdiff1d(at + np.arange(ext[k]), run_at)
            v[gaps] = 6e4
            if it["hi"]:
                v[run_at[it["hi_at"]]] = 3e4 * (-1.0 if k % 2 else 1.0)
            where.append(run_at)
            groups.append(gidx[k])
            at += ext[k]
        t = torch.from_numpy(v).to(TORCH[dt])
        assert bool(torch.isfinite(t.float()).all())
        raw = t.view(torch.uint8).numpy()
        at = 0
        for k in ks:
            src[k] = raw[at * ISZ[dt]:(at + ext[k]) * ISZ[dt]]
            at += ext[k]
        # the reference of safetensors_fp8_cases.flat_scales, all slots at once
        a = t.float().abs()[torch.from_numpy(np.concatenate(where))]
        amax.scatter_reduce_(0, torch.from_numpy(np.concatenate(groups)), a,
                             "amax")
    scale = (amax.clamp(min=2 ** -40) / 448).numpy()
    exp = np.full(n_out, PREFILL, dtype=np.float32)
    for o, n in ranges:
        exp[o:o + n] = scale[o:o + n]
    # the leak cases say what they should
    big_scale, small_scale = np.float32(3e4 / 448 / 2), np.float32(1e-3 / 448)
    for it in items:
        if it["share"] is None and it["tile"] % CAP not in ABSMAX_SHARED:
            top = exp[it["out"]:it["out"] + it["groups"]].max()
            assert (top > big_scale) == it["hi"] and \
                (it["hi"] or top <= small_scale)

    s_offs, s_total = slots([len(c) for c in src], [it["sres"] for it in items])
    s_img = image(s_total, s_offs, src, fill=0x5A)
    sbuf = tier.put(s_img)
    obuf = tier.put(np.full(n_out, PREFILL, dtype=np.float32).view(np.uint8))
    segs = [(sbuf.data_ptr() + int(s_offs[k]), it["rows"], it["run"],
             (it["run"] + it["gap"]) * ISZ[it["dt"]], D[it["dt"]],
             obuf.data_ptr() + 4 * it["out"], it["every"], it["e0"],
             it["groups"]) for k, it in enumerate(items)]
    tier.native.absmax_scales(tier.device, segs)
    got = tier.get(obuf).view(np.uint32)
    want = exp.view(np.uint32)
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        k = max(j for j, it in enumerate(items) if it["out"] <= i)
        raise AssertionError(
            f"absmax_scales: slot {i} is {got[i]:#x} "
            f"({got[i:i + 1].view(np.float32)[0]!r}), expected {want[i]:#x} "
            f"({exp[i]!r}); {int((got != want).sum())} slots differ; item "
            f"{k}, first tile {items[k]['tile']} = {items[k]['tile'] // CAP} "
            f"* CAP + {items[k]['tile'] % CAP}, hi={items[k]['hi']}")
    assert np.array_equal(tier.get(sbuf), s_img), "a source changed"


# --------------------------------------------------------- j: array samples

import array_sample_cases as asc  # noqa: E402

ARRAY_SHAPE, ARRAY_CROP = (6, 7, 3), (4, 5)
ARRAY_COMBOS = (("F32", "NCHW"), ("F32", "NHWC"), ("BF16", "NCHW"),
                ("BF16", "NHWC"))
ARRAY_KINDS = ("both", "first_out", "second_out")


class SampleCall(asc.Call):
    """array_sample_cases.Call with the sources gathered into one image,
    written to the arena once, and one reference per sample."""

    def start(self, total):
        self.src_img = np.full(total, 0x5A, dtype=np.uint8)
        self.ref_row, self.ref = None, None

    def place(self, off, img):
        self.src_img[off:off + img.size] = img.ravel()

    def piece(self, off, row, e0, n, img):
        self.pieces.append((off, row, e0, n))
        if self.ref_row != row:
            dy, dx, flip = self.rows[row]
            self.ref_row, self.ref = row, asc.ref_sample(
                img, dy, dx, flip, self.crop, self.scale, self.bias,
                self.layout, self.dst)
        raw, emap = self.ref
        hit = np.repeat((emap >= e0) & (emap < e0 + n), self.ds)
        a = self.lead + row * self.out_el * self.ds
        self.exp[a:a + self.out_el * self.ds][hit] = raw[hit]


def plan_array(CAP, array_tile):
    """Samples of 6x7x3 bytes, each cut into two pieces = two tiles, until
    the call has 2 * CAP + 304 tiles."""
    H, W, C = ARRAY_SHAPE
    h, w = ARRAY_CROP
    wc, size = W * C, H * W * C
    half = CAP // 2
    samples, items, owner = [], [], []
    while len(owner) < 2 * CAP + EXTRA + 4:
        b = len(samples)
        tile, trip, wg = 2 * b, 2 * b // CAP, b % half
        p = samples[b - half] if b >= half else None
        kind = ARRAY_KINDS[(wg + trip) % 3]
        dys = {"both": (0, 1, 2), "first_out": (1, 2), "second_out": (0, 1)}
        for k in range(3 * 3 * 2):
            j = 5 * wg + 7 * trip + k
            aug = (dys[kind][j % len(dys[kind])], (j // 3) % (W - w + 1),
                   (j // 2) % 2)
            if p is None or aug != p["aug"]:
                break
        dy = aug[0]
        cuts = {"both": range(dy * wc + 1, (dy + h) * wc),
                "first_out": range(1, dy * wc + 1),
                "second_out": range((dy + h) * wc, size)}[kind]
        short = 9 if b % 5 == 0 and kind != "second_out" else 0
        cuts = [c for c in cuts if c < size - short]
        for k in range(len(cuts) * 16):
            j = 11 * wg + 13 * trip + k
            cut, sres = cuts[j % len(cuts)], (j // len(cuts) + 3 * wg) % 16
            if p is None or (cut != p["cut"] and sres != p["sres"] and
                             (sres + cut) % 16 != (p["sres"] + p["cut"]) % 16
                             and size - short - cut != size - p["short"]
                             - p["cut"]):
                break
        else:
            raise AssertionError("no cut left that differs")
        s = {"aug": aug, "cut": cut, "sres": sres, "kind": kind,
             "short": short}
        samples.append(s)
        for e0, n in ((0, cut), (cut, size - short - cut)):
            y0, y1 = e0 // wc, (e0 + n - 1) // wc
            items.append({"tile": len(owner), "tiles": 1, "row": b, "e0": e0,
                          "n": n, "sres": (sres + e0) % 16, "aug": aug,
                          "skipped": y0 > dy + h - 1 or y1 < dy})
            owner.append(len(items) - 1)
    counted = [-(-it["n"] // array_tile) for it in items]
    check_plan(CAP, items, owner, counted, ["sres", "n", "aug"],
               straddle=False)
    # a tile that returns before its barriers, then a tile that stages, in
    # one workgroup; and the reverse
    orders = {(items[t]["skipped"], items[t + CAP]["skipped"])
              for t in range(CAP)}
    assert orders == {(False, False), (True, False), (False, True)}
    assert any(it["skipped"] for it in items[2 * CAP:])
    assert any(s["short"] and s["aug"][0] == 2 for s in samples)
    return samples, items


def case_array_samples(tier, dst, layout):
    """Arena.array_samples over samples of 6x7x3 bytes, crop 4x5, each cut
    into two pieces at a byte of its own: two tiles per sample, 2 * CAP + 304
    tiles.

    Own slot: the destination is dense, [batch, 3, 4, 5] or [batch, 4, 5, 3],
    so the slots are the samples' own elements; the whole buffer with 16
    guard bytes either side is compared, every crop element against the
    reference, and every byte no piece covers (the last 9 bytes of every
    fifth sample are in no piece) still holds the sentinel.  Partners (both
    first pieces or both second pieces, of samples CAP / 2 apart) differ in
    source residue mod 16, length and (dy, dx, flip); the destination
    residue is the dense layout's.  No piece can straddle a trip: a piece of
    126 bytes or less is one tile of ARRAY_TILE (multi-tile pieces are
    array_sample_cases' own).  A third of the samples have their first piece
    wholly above the crop rows, a third their second piece wholly below:
    those tiles take array_tile's early return, which skips both barriers,
    in the first trip of some workgroups (a staging tile follows in the
    second) and in the second or third trip of others."""
    samples, items = plan_array(tier.CAP, tier.mod.ARRAY_TILE)
    size = int(np.prod(ARRAY_SHAPE))
    rng = np.random.default_rng(401)
    imgs = rng.integers(0, 256, (len(samples),) + ARRAY_SHAPE).astype(np.uint8)
    s_offs, s_total = slots([size] * len(samples),
                            [s["sres"] for s in samples])
    scale, bias = asc.norm(asc.IMAGENET_MEAN, asc.IMAGENET_STD, 3)
    c = SampleCall(tier.arena, tier.D, tier.tdev, dst, ARRAY_SHAPE,
                   ARRAY_CROP, [s["aug"] for s in samples], scale, bias,
                   layout, el_off=1)
    c.start(s_total)
    for b in range(len(samples)):
        c.place(int(s_offs[b]), imgs[b])
    for it in items:
        c.piece(int(s_offs[it["row"]]) + it["e0"], it["row"], it["e0"],
                it["n"], imgs[it["row"]])
    assert (c.exp[c.lead:-GUARD] == SENTINEL).sum() > 0
    tier.arena_put(0, c.src_img)
    c.run()
    assert np.array_equal(tier.arena_get(0, s_total), c.src_img), \
        "a source changed"


# ------------------------------------------------------- h: token eos index

import token_pack_cases as pc  # noqa: E402


def case_token_eos(tier, src):
    """Arena.token_eos_index over 2 * CAP + 300 and more short ascending
    spans with gaps of 1 to 3 in tok0, one tile of TOKEN_EOS_TILE each.

    Own slot: the hits are one dense ascending int64 list, so a slot is a
    rank; the list is compared whole with ref_eos between 16 guard bytes, at
    a capacity of the total and at a smaller one, and the total against the
    pure count.  Partners differ in source residue mod 16, length and hits:
    with r = tile % CAP the spans of r % 3 == 0 have no hit, hits, no hit
    over the three trips, those of r % 3 == 1 the reverse, those of
    r % 3 == 2 hold 2, 3 and 4 hits.  Spans of 2 * TOKEN_EOS_TILE + 3 and
    + 5 tokens with hits either side of their tile edges straddle tiles
    CAP-1 | CAP and 2*CAP-1 | 2*CAP."""
    CAP, E = tier.CAP, tier.mod.TOKEN_EOS_TILE
    ss = np.dtype(tc.NP_SRC[src]).itemsize

    def make(tile, r, trip, big, partners):
        def taken(key):
            return {p[key] for p in partners}
        it = {}
        if big:
            it["n"] = pick((2 * E + 3, 2 * E + 5), trip, taken("n"))
            it["hits"] = pick((6, 7, 8), trip, taken("hits"))
        else:
            it["n"] = pick(range(10, 41), 7 * r + 11 * trip, taken("n"))
            it["hits"] = pick(((0, 1 + r % 4, 0), (1 + r % 5, 0, 2),
                               (2, 3, 4))[r % 3][trip:] + (5, 9),
                              0, taken("hits"))
        it["sres"] = pick(range(16), 5 * r + 7 * trip, taken("sres"))
        return it

    items, owner = lay_tiles(CAP, make)
    counted = [-(-it["n"] // E) for it in items]
    check_plan(CAP, items, owner, counted, ["sres", "n", "hits"])
    pairs = {(bool(items[owner[t]]["hits"]), bool(items[owner[t + CAP]]["hits"]))
             for t in range(CAP)}
    assert pairs == {(False, True), (True, False), (True, True)}

    rng = np.random.default_rng(503)
    spans, call, tok0 = [], [], 7
    s_offs, s_total = slots([it["n"] * ss for it in items],
                            [it["sres"] for it in items])
    img = np.full(s_total, 0x5A, dtype=np.uint8)
    for k, it in enumerate(items):
        t = pc.eos_tokens(rng, src, it["n"])
        if it["tiles"] > 1:
            at = [0, E - 1, E, 2 * E - 1, 2 * E, it["n"] - 1, 77, E + 5]
        else:
            at = rng.permutation(it["n"]).tolist()
        t[at[:it["hits"]]] = pc.EOS
        assert int((t == pc.EOS).sum()) == it["hits"]
        raw = np.frombuffer(t.tobytes(), np.uint8)
        img[s_offs[k]:s_offs[k] + len(raw)] = raw
        spans.append((tok0, t))
        call.append((int(s_offs[k]), tok0, it["n"]))
        tok0 += it["n"] + 1 + k % 3
    tier.arena_put(0, img)
    exp = pc.ref_eos(spans, pc.EOS)
    assert len(exp) == sum(it["hits"] for it in items) > CAP
    D = tier.D
    assert tier.arena.token_eos_index(call, D[src], pc.EOS, 0, 0) == len(exp)
    for cap in (len(exp), len(exp) - CAP // 2 - 3):
        out = pc.Buf(tier.device, cap, 8)
        got = tier.arena.token_eos_index(call, D[src], pc.EOS, out.ptr, cap)
        assert got == len(exp), (got, len(exp), cap)
        out.expect(exp[:cap], f"eos index {src} cap={cap}")
    assert np.array_equal(tier.arena_get(0, s_total), img), "a source changed"


# ------------------------------------------------------------ i: token pack

PACK_PAIRS = (("U16", "I32"), ("I32", "I64"))


class PackImageCall(pc.PackCall):
    """token_pack_cases.PackCall with the sources gathered into one image
    and written to the arena once, before the call."""

    def start(self, total):
        self.src_img = np.full(total, 0x5A, dtype=np.uint8)

    def place(self, tokens, phase):
        self.at = (self.at + 63) // 64 * 64 + phase
        off = self.at
        raw = np.frombuffer(tokens.tobytes(), np.uint8)
        self.src_img[off:off + len(raw)] = raw
        self.at += len(raw)
        return off

    def run(self, vocab=0):
        self.arena.write(0, self.src_img.tobytes())
        return super().run(vocab)


def case_token_pack(tier, src, dst):
    """Arena.token_pack with CAP + CAP / 2 tiles of source pieces followed by
    pad segments up to 2 * CAP + 304 tiles, in rows of T = 2 *
    TOKEN_PACK_TILE + 65 columns that hold about a hundred segments each.

    Own slot: four columns or more that no segment covers lie between two
    segments of a row (16 bytes and more), every fifth source segment gets
    only its second piece, and x, y, position ids, document ids and
    cu_seqlens are compared whole between guards with the reference of
    token_pack_cases.PackCall.  Partners differ in length and, piece against
    piece, in source residue mod 16; one-tile partners also in destination
    residue; a source piece's partner in the third trip is a pad segment.
    A source piece of 2 * TOKEN_PACK_TILE + 3 tokens straddles tiles CAP-1 |
    CAP, a pad segment of 2 * TOKEN_PACK_TILE + 3 columns tiles 2*CAP-1 |
    2*CAP.  Vocabulary: ids outside [0, 1000) lie in the first-trip piece
    only, the second-trip piece only, both or neither of a workgroup, by
    tile % 4; the count equals the reference's exactly."""
    CAP, PT = tier.CAP, tier.mod.TOKEN_PACK_TILE
    T = 2 * PT + 65
    ds = np.dtype(tc.NP_DST[dst]).itemsize
    n_src = CAP + CAP // 2
    cur = [0, 0]                                  # row, first free column

    def make(tile, r, trip, big, partners):
        def taken(key):
            return {p[key] for p in partners}
        it = {"pad": tile >= n_src}
        if big:
            it["n"] = pick((2 * PT + 3, 2 * PT + 5), trip, taken("n"))
        elif it["pad"]:
            it["n"] = pick(range(10, 16), 7 * r + 11 * trip, taken("n"))
        else:
            it["n"] = pick(range(1, 9), 7 * r + 11 * trip, taken("n"))
        it["next"] = not it["pad"] and (r + trip) % 3 == 0
        it["second"] = not it["pad"] and not big and r % 5 == 0 and \
            it["n"] + it["next"] >= 2
        it["cut"] = 1 + r % (it["n"] + it["next"] - 1) if it["second"] else 0
        it["k"] = it["n"] + it["next"] - it["cut"]
        while it["k"] in {p["k"] for p in partners}:
            it["cut"] -= 1
            it["k"] += 1
        it["second"] = it["cut"] > 0
        it["sres"] = -1 if it["pad"] else \
            pick(range(16), 5 * r + 7 * trip, taken("sres"))
        def cls(row, col):
            return ((row * T + col) * ds) % 16
        spots = [(cur[0], cur[1] + g) for g in range(4, 8)
                 if cur[1] + g + it["n"] <= T]
        if len(spots) < 4:
            spots = [(cur[0] + 1, g) for g in range(4, 8)]
        free = [s for s in spots if cls(*s) not in taken("dres")] or spots
        it["row"], it["col"] = free[(r + trip) % len(free)]
        cur[0], cur[1] = it["row"], it["col"] + it["n"]
        it["dres"] = cls(it["row"], it["col"])
        it["bad"] = not it["pad"] and (
            (r % 4 in (1, 3)) if trip == 0 else (r % 4 in (2, 3)))
        return it

    items, owner = lay_tiles(CAP, make)
    counted = [-(-(it["n"] if it["pad"] else it["k"]) // PT) for it in items]
    n_tiles = check_plan(CAP, items, owner, counted, ["k", "sres"])
    assert T % 2 == 1
    for t in range(n_tiles - CAP):
        a, b = items[owner[t]], items[owner[t + CAP]]
        assert a["dres"] != b["dres"] or a["tiles"] > 1 or b["tiles"] > 1
    assert items[owner[CAP]]["pad"] is False and items[owner[2 * CAP]]["pad"]
    seen = {(items[owner[t]]["bad"], items[owner[t + CAP]]["bad"])
            for t in range(n_src - CAP)}
    assert seen == {(False, False), (True, False), (False, True), (True, True)}

    rng = np.random.default_rng(601)
    over = {"U16": 0xFFFF, "U32": 2 ** 31, "I32": -1}[src]
    rows = items[-1]["row"] + 1
    c = PackImageCall(tier.arena, tier.D, tier.device, src, dst, rows, T)
    c.start(4 << 20)
    for k, it in enumerate(items):
        if it["pad"]:
            c.pad(it["row"], it["col"], it["n"])
            continue
        d = tc.make_tokens(rng, src, it["n"] + it["next"], below=VOCAB)
        if it["bad"]:
            d[it["cut"] + k % it["k"]] = over
            d[len(d) - 1] = over
        c.seg(it["row"], it["col"], d, it["next"], pos0=k % 50, doc=k % 7,
              cuts=(it["cut"],) if it["second"] else (),
              keep=(1,) if it["second"] else None,
              phase=(it["sres"] - (5 if it["second"] else 0)) % 16)
        assert c.pieces[-1][0] % 16 == it["sres"] and \
            c.pieces[-1][3] == it["k"]
    assert c.at <= len(c.src_img)
    got = c.run(vocab=VOCAB)
    assert got >= CAP // 2
    assert c.run(vocab=0) == 0


def case_token_pack_cu(tier, src, dst):
    """The cu_seqlens loop of token_pack_kernel, i += gridDim.x * 256, runs
    over the segments under the grid of the tiles: one piece (one tile, one
    workgroup) and 600 further segments whose pieces are not passed take it
    round three times.  No other pack case has more segments than
    256 * its grid."""
    rng = np.random.default_rng(607)
    n_segs, T = 601, 9
    c = PackImageCall(tier.arena, tier.D, tier.device, src, dst, n_segs, T)
    c.start(1 << 16)
    for row in range(n_segs):
        n = 1 + row % 5
        c.seg(row, row % 4, tc.make_tokens(rng, src, n), False, doc=row,
              keep=None if row == 300 else ())
    assert len(c.pieces) == 1 and len(c.segs) > 2 * 256
    c.run()


# --------------------------------------------------- f: block absmax scales

# (M, K, (bm, bn)): tiny whole matrices, M * K different in each
BLOCK_SHAPES = ((5, 9, (4, 8)), (3, 17, (2, 8)), (7, 8, (4, 8)),
                (4, 20, (4, 8)), (6, 11, (3, 4)), (1, 40, (1, 16)),
                (9, 6, (2, 2)))
# 36 x 64 under 1 x 2 tiles: 1152 slots, more than one window of
# BLOCK_LDS_SLOTS = 1024, in one tile of CAST_TILE; (r, trip) of such items
BLOCK_WIDE = (36, 64, (1, 2))
BLOCK_WIDE_AT = {(202, 0), (200, 1), (201, 2), (203, 1)}


def case_block_absmax(tier):
    """native.block_absmax_scales over whole tiny matrices, one per tile,
    each with slots of its own in an f32 array pre-filled with 7.0.

    Own slot: as in case_absmax, one float or more that belongs to no
    matrix lies between two slot ranges, scale_slots_kernel gets more than
    2 * CAP ranges, and the whole array is compared: the gaps still read
    7.0.  Partners differ in source dtype, source residue, slot residue,
    shape (M * K differs) and in the tile of the matrix that holds the
    maximum: every matrix holds one value of 3e4 in one of its tiles and
    nothing else above 1e-3, so an LDS word left over from the tile before,
    or a window not zeroed, shows in a scale.  Matrices of 36 x 64 under
    1 x 2 tiles (1152 slots, two LDS windows) run in the first, second and
    third trip of workgroups 200 .. 203.  Matrices of 1 x (2 * CAST_TILE +
    3) and + 5 under 1 x 128 tiles straddle tiles CAP-1 | CAP and 2*CAP-1 |
    2*CAP."""
    CAP, D, cast_tile = tier.CAP, tier.D, tier.mod.CAST_TILE
    lds_slots = 1024

    def make(tile, r, trip, big, partners):
        def taken(key):
            return {p[key] for p in partners}
        it = {"dt": pick(ABSMAX_SRC, r + trip, taken("dt"))}
        if big:
            shape = (1, pick((2 * cast_tile + 3, 2 * cast_tile + 5), trip,
                             {p["K"] for p in partners}), (1, 128))
        elif (r, trip) in BLOCK_WIDE_AT:
            shape = BLOCK_WIDE
        else:
            shape = pick([s for s in BLOCK_SHAPES
                          if s[0] * s[1] not in taken("n")], 7 * r + 11 * trip)
        it["M"], it["K"], (it["bm"], it["bn"]) = shape
        it["n"] = it["M"] * it["K"]
        it["tn"] = -(-it["K"] // it["bn"])
        it["groups"] = -(-it["M"] // it["bm"]) * it["tn"]
        it["peak"] = pick(range(it["groups"]), 3 * r + trip, taken("peak"))
        it["sres"] = pick(residue_options(ISZ[it["dt"]]), 5 * r + 7 * trip,
                          taken("sres"))
        it["ores"] = pick(range(4), r + 3 * trip, taken("ores"))
        return it

    items, owner = lay_tiles(CAP, make)
    counted = [-(-it["n"] // cast_tile) for it in items]
    check_plan(CAP, items, owner, counted,
               ["dt", "sres", "ores", "n", "peak"])
    wide = [it for it in items if it["groups"] > lds_slots and it["tiles"] == 1]
    assert {it["tile"] // CAP for it in wide} == {0, 1, 2}

    at = 0
    for it in items:
        at += 1
        at += (it["ores"] - at) % 4
        it["out"] = at
        at += it["groups"]
    n_out = at + 1
    assert len(items) > 2 * CAP

    rng = np.random.default_rng(701)
    src = [None] * len(items)
    amax = torch.zeros(n_out)
    for dt in ABSMAX_SRC:
        ks = [k for k, it in enumerate(items) if it["dt"] == dt]
        total = sum(items[k]["n"] for k in ks)
        v = ((1e-6 + rng.random(total) * 9e-4) *
             rng.choice([-1.0, 1.0], total)).astype(np.float32)
        at, groups = 0, []
        for k in ks:
            it = items[k]
            e = np.arange(it["n"])
            row, col = e // it["K"], e % it["K"]
            slot = (row // it["bm"]) * it["tn"] + col // it["bn"]
            mine = np.flatnonzero(slot == it["peak"])
            v[at + mine[k % len(mine)]] = 3e4 * (-1.0 if k % 2 else 1.0)
            groups.append(it["out"] + slot)
            at += it["n"]
        t = torch.from_numpy(v).to(TORCH[dt])
        assert bool(torch.isfinite(t.float()).all())
        raw = t.view(torch.uint8).numpy()
        at = 0
        for k in ks:
            nb = items[k]["n"] * ISZ[dt]
            src[k] = raw[at:at + nb]
            at += nb
        # the reference of safetensors_block_cases.ref_scales, every tile of
        # every matrix at once: amax over the tile, clamped, over 448
        amax.scatter_reduce_(0, torch.from_numpy(np.concatenate(groups)),
                             t.float().abs(), "amax")
    scale = (amax.clamp(min=2 ** -40) / 448).numpy()
    exp = np.full(n_out, PREFILL, dtype=np.float32)
    for it in items:
        o, n = it["out"], it["groups"]
        exp[o:o + n] = scale[o:o + n]
        assert int((exp[o:o + n] > 1.0).sum()) == 1 and \
            exp[o + it["peak"]] > 1.0

    s_offs, s_total = slots([len(c) for c in src], [it["sres"] for it in items])
    s_img = image(s_total, s_offs, src, fill=0x5A)
    sbuf = tier.put(s_img)
    obuf = tier.put(np.full(n_out, PREFILL, dtype=np.float32).view(np.uint8))
    segs = [(sbuf.data_ptr() + int(s_offs[k]), it["M"], it["K"],
             it["K"] * ISZ[it["dt"]], D[it["dt"]],
             obuf.data_ptr() + 4 * it["out"], 0, it["K"], it["M"], it["K"],
             it["bm"], it["bn"], it["groups"]) for k, it in enumerate(items)]
    tier.native.block_absmax_scales(tier.device, segs)
    got = tier.get(obuf).view(np.uint32)
    want = exp.view(np.uint32)
    if not np.array_equal(got, want):
        i = int(np.nonzero(got != want)[0][0])
        k = max(j for j, it in enumerate(items) if it["out"] <= i)
        raise AssertionError(
            f"block_absmax_scales: slot {i} is {got[i]:#x}, expected "
            f"{want[i]:#x} ({exp[i]!r}); {int((got != want).sum())} slots "
            f"differ; item {k}, first tile {items[k]['tile']} = "
            f"{items[k]['tile'] // CAP} * CAP + {items[k]['tile'] % CAP}, "
            f"{items[k]['M']} x {items[k]['K']}")
    assert np.array_equal(tier.get(sbuf), s_img), "a source changed"


# ------------------------------------------------------------------- e: MX

import safetensors_mx_cases as mxc  # noqa: E402

MX_MODES = ("scales", "store", "load")
MX_KINDS = tuple((dt, st) for dt in mxc.SOURCES for st in ("F8_E4M3", "F4"))


def case_mx(tier, mode):
    """native.mx_scales ("scales"), the 11-tuple Arena.store_ptr ("store")
    and the 11-tuple Arena.convert_ptr ("load"), one item of 32 to 96
    elements per tile.

    Own slot: every item's E8M0 bytes, MXFP8 / MXFP4 codes or wide elements
    lie in a slot of their own between 16 or more sentinel bytes, the whole
    destination compared.  Partners differ in the (wide dtype, stored
    dtype) pair, source residue, destination residue and length, and their
    block exponents lie binades apart: the scale bytes follow 127 +
    tile % 23 - 11 and the values follow the scales.  "scales" takes whole
    blocks (32, 64 or 96 elements); the pieces of "store" and "load" begin
    mid-block on two items of three (scale_e0 % 32 != 0, even for F4).
    Straddling tiles CAP-1 | CAP and 2*CAP-1 | 2*CAP: 2 * CAST_TILE + 32 and
    + 64 elements for "scales" (whole blocks), 2 * CAST_TILE + 3 and + 5
    MXFP8 elements (+ 4 and + 6 for MXFP4, whole bytes) for the others."""
    CAP, D, cast_tile = tier.CAP, tier.D, tier.mod.CAST_TILE
    whole = mode == "scales"

    def make(tile, r, trip, big, partners):
        def taken(key):
            return {p[key] for p in partners}
        it = {"kind": pick(MX_KINDS, r + trip, taken("kind"))}
        dt, st = it["kind"]
        even = st == "F4"
        if big:
            lens = (2 * cast_tile + 32, 2 * cast_tile + 64) if whole else \
                (2 * cast_tile + 3 + even, 2 * cast_tile + 5 + even)
        elif whole:
            lens = (32, 64, 96)
        else:
            lens = tuple(range(32, 97, 2)) if even else tuple(range(32, 97))
        it["n"] = pick(lens, 7 * r + 11 * trip, taken("n"))
        it["e0"] = 0 if whole or (r + trip) % 3 == 0 else \
            2 * (1 + (3 * r + 5 * trip) % 15)
        it["exp"] = tile % 23 - 11
        src_al = ISZ[dt] if mode != "load" else 1
        dst_al = ISZ[dt] if mode == "load" else 1
        it["sres"] = pick(residue_options(src_al), 5 * r + 7 * trip,
                          taken("sres"))
        it["dres"] = pick(residue_options(dst_al), 3 * r + 5 * trip,
                          taken("dres"))
        return it

    items, owner = lay_tiles(CAP, make)
    counted = [-(-it["n"] // cast_tile) for it in items]
    check_plan(CAP, items, owner, counted,
               ["kind", "sres", "dres", "n", "exp"])
    if not whole:
        assert sum(it["e0"] % 32 != 0 for it in items) > CAP

    rng = np.random.default_rng(801 + MX_MODES.index(mode))
    src, exp, sc = [None] * len(items), [None] * len(items), []
    s_at = 0
    for it in items:                 # the scale bytes of blocks 0 .. last
        nb = (it["e0"] + it["n"] - 1) // 32 + 1
        it["s_at"] = s_at
        sc.append((127 + it["exp"] + np.arange(nb) % 3).astype(np.uint8))
        s_at += nb
    sc = np.concatenate(sc)
    for kind in MX_KINDS:
        dt, st = kind
        ks = [k for k, it in enumerate(items) if it["kind"] == kind]
        total = sum(items[k]["n"] for k in ks)
        s_el = np.concatenate([
            sc[items[k]["s_at"] + (items[k]["e0"] + np.arange(items[k]["n"]))
               // 32] for k in ks])
        wide_b = [items[k]["n"] * ISZ[dt] for k in ks]
        code_b = [items[k]["n"] * mxc.BITS[st] // 8 for k in ks]
        if mode == "load":
            raw = rng.integers(0, 256, sum(code_b), dtype=np.uint8)
            if st == "F8_E4M3":
                raw &= np.uint8(0xBF)
            codes = mxc.unpack(raw.tobytes(), st)
            assert mxc.count_nan(codes, s_el, st) == 0
            out = mxc.ref_dequant(codes, s_el, st, mxc.TDT[dt]) \
                .view(torch.uint8).numpy()
            in_b, out_b = code_b, wide_b
        else:
            v = rng.standard_normal(total) * \
                np.exp2(s_el.astype(np.float64) - 127 +
                        rng.integers(-3, 4, total))
            t = torch.from_numpy(np.clip(v, -6e4, 6e4)).to(mxc.TDT[dt])
            assert bool(torch.isfinite(t.float()).all())
            raw = t.view(torch.uint8).numpy()
            x64 = mxc.widen(t)
            if whole:
                out = mxc.ref_scales(x64, st)
                out_b = [items[k]["n"] // 32 for k in ks]
            else:
                out = np.frombuffer(
                    mxc.pack(mxc.ref_quant(x64, s_el, st), st), np.uint8)
                out_b = code_b
            in_b = wide_b
        a = b = 0
        for k, ni, no in zip(ks, in_b, out_b):
            src[k], exp[k] = raw[a:a + ni], out[b:b + no]
            a, b = a + ni, b + no
        assert a == len(raw) and b == len(out)

    s_offs, s_total = slots([len(c) for c in src], [it["sres"] for it in items])
    d_offs, d_total = slots([len(c) for c in exp], [it["dres"] for it in items])
    s_img = image(s_total, s_offs, src, fill=0x5A)
    exp_img = image(d_total, d_offs, exp)
    blank = np.full(d_total, SENTINEL, dtype=np.uint8)
    scale_buf = tier.put(sc) if not whole else None
    if mode == "load":
        tier.arena_put(0, s_img)
        dbuf = tier.put(blank)
        a0, b0 = 0, dbuf.data_ptr()
    else:
        sbuf = tier.put(s_img)
        if whole:
            dbuf = tier.put(blank)
            b0 = dbuf.data_ptr()
        else:
            tier.arena_put(0, blank)
            b0 = 0
        a0 = sbuf.data_ptr()
    segs = []
    for k, it in enumerate(items):
        dt, st = it["kind"]
        a, b, n = a0 + int(s_offs[k]), b0 + int(d_offs[k]), it["n"]
        if whole:
            segs.append((a, 1, n, n * ISZ[dt], D[dt], D[st], b))
        elif mode == "store":
            segs.append((a, b, 1, n, n * ISZ[dt], D[dt], D[st],
                         scale_buf.data_ptr() + it["s_at"], it["e0"], n, 32))
        else:
            segs.append((a, b, 1, n, n * mxc.BITS[st] // 8, D[st], D[dt],
                         scale_buf.data_ptr() + it["s_at"], it["e0"], n, 32))
    if whole:
        tier.native.mx_scales(tier.device, segs)
    elif mode == "store":
        tier.arena.store_ptr(segs)
    else:
        tier.arena.convert_ptr(segs)
    got = tier.arena_get(0, d_total) if mode == "store" else tier.get(dbuf)
    check_image("mx " + mode, CAP, got, exp_img, items, d_offs,
                [len(c) for c in exp])
    if mode == "load":
        assert np.array_equal(tier.arena_get(0, s_total), s_img)
    else:
        assert np.array_equal(tier.get(sbuf), s_img), "a source changed"


def plan_block_cast(tier, store):
    """Whole tiny matrices (BLOCK_SHAPES) under given f32 tile scales, one
    per tile, for the 14-tuple store_ptr (F32 / F16 / BF16 -> F8_E4M3) and
    convert_ptr (back).  Partners differ in dtype pair, source residue,
    destination residue, shape (M * K differs) and scale (two binades and
    more); every tile of a matrix has a scale of its own.  Matrices of 1 x
    (2 * CAST_TILE + 3) and + 5 under 1 x 128 tiles straddle tiles CAP-1 |
    CAP and 2*CAP-1 | 2*CAP."""
    CAP, cast_tile = tier.CAP, tier.mod.CAST_TILE
    pairs = QUANT_PAIRS if store else DEQUANT_PAIRS

    def make(tile, r, trip, big, partners):
        def taken(key):
            return {p[key] for p in partners}
        it = {"pair": pick(pairs, r + 3 * trip, taken("pair"))}
        s, d = it["pair"]
        if big:
            shape = (1, pick((2 * cast_tile + 3, 2 * cast_tile + 5), trip,
                             {p["K"] for p in partners}), (1, 128))
        else:
            shape = pick([q for q in BLOCK_SHAPES
                          if q[0] * q[1] not in taken("n")], 7 * r + 11 * trip)
        it["M"], it["K"], (it["bm"], it["bn"]) = shape
        it["n"] = it["M"] * it["K"]
        it["tn"] = -(-it["K"] // it["bn"])
        it["groups"] = -(-it["M"] // it["bm"]) * it["tn"]
        it["scale"] = item_scale(tile)
        it["sres"] = pick(residue_options(ISZ[s] if store else 1),
                          5 * r + 7 * trip, taken("sres"))
        it["dres"] = pick(residue_options(ISZ[d]), 3 * r + 5 * trip,
                          taken("dres"))
        return it

    items, owner = lay_tiles(CAP, make)
    counted = [-(-it["n"] // cast_tile) for it in items]
    check_plan(CAP, items, owner, counted,
               ["pair", "sres", "dres", "n", "scale"])
    for t in range(len(owner) - CAP):
        a, b = items[owner[t]]["scale"], items[owner[t + CAP]]["scale"]
        assert max(a, b) / min(a, b) >= 2.0
    return items


def block_groups(items):
    """scaled_groups for whole matrices: the tile of element (row, col) is
    (row // bm) * ceil(K / bn) + col // bn."""
    start, scales, idx = [], [], []
    at = 0
    for it in items:
        e = np.arange(it["n"], dtype=np.int64)
        g = (e // it["K"] // it["bm"]) * it["tn"] + e % it["K"] // it["bn"]
        scales.append(np.float32(it["scale"]) *
                      (1 + 0.25 * (np.arange(it["groups"]) % 4))
                      .astype(np.float32))
        start.append(at)
        idx.append(at + g)
        at += it["groups"]
    return np.concatenate(scales).astype(np.float32), start, idx
