"""Shared cases for the token-window tests (host arena and MI355X).

Nothing here imports project code: the expected x and y come from numpy
`frombuffer(...).astype(...)`, the out-of-range count from a plain loop.
The runners take the arena, the dtype codes and the loader factory from
the test module that calls them, so the host and the GPU file run the same
matrix.  Every comparison is exact integer equality on whole buffers,
guard bytes included."""
import random

import numpy as np
import torch

PAIRS = [("U16", "I32"), ("U16", "I64"), ("U32", "I64"),
         ("I32", "I32"), ("I32", "I64")]
NP_SRC = {"U16": np.uint16, "U32": np.uint32, "I32": np.int32}
NP_DST = {"I32": np.int32, "I64": np.int64}
TORCH_DST = {"I32": torch.int32, "I64": torch.int64}
# a sign extension where a zero extension belongs, and the reverse
SPECIALS = {"U16": [0, 0x7FFF, 0x8000, 0xFFFF],
            "U32": [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF],
            "I32": [0, -1, -2 ** 31, 2 ** 31 - 1]}
SENTINEL = 0xAB
GUARD = 16
T_SMALL = (1, 2, 7, 8, 9, 63, 64, 65)
ROWS = 3


def make_tokens(rng, src, n, below=None):
    """n tokens of `src`: random, the specials spread among them unless
    `below` bounds every value (the vocabulary cases place their own)."""
    info = np.iinfo(NP_SRC[src])
    if below is not None:
        return rng.integers(0, below, n).astype(NP_SRC[src])
    t = rng.integers(info.min, int(info.max) + 1, n).astype(NP_SRC[src])
    sp = SPECIALS[src]
    for i in range(n):
        if i % 3 == 0:
            t[i] = sp[(i // 3) % len(sp)]
    return t


def ref_widen(tokens, dst):
    return tokens.astype(NP_DST[dst])


def ref_count(tokens, src, vocab):
    """The rule, as a plain loop."""
    if vocab == 0:
        return 0
    bad = 0
    for v in tokens.tolist():
        if src == "I32":
            if v < 0 or v >= vocab:
                bad += 1
        elif v >= vocab:
            bad += 1
    return bad


def ref_file_windows(blob, src, dst, header, T, stride=None):
    """(x, y) of every window of one file, [n_windows, T] each."""
    stride = T if stride is None else stride
    item = np.dtype(NP_SRC[src]).itemsize
    n_f = (len(blob) - header) // item
    toks = np.frombuffer(blob, dtype=NP_SRC[src], count=n_f, offset=header)
    if n_f < T + 1:
        z = np.zeros((0, T), NP_DST[dst])
        return z, z, np.zeros((0, T + 1), NP_SRC[src])
    starts = [k * stride for k in range((n_f - T - 1) // stride + 1)]
    w = np.stack([toks[s:s + T + 1] for s in starts])
    return ref_widen(w[:, :-1], dst), ref_widen(w[:, 1:], dst), w


# ------------------------------------------------------------ kernel runner

class Call:
    """One Arena.token_windows call on sentinel-filled destinations."""

    def __init__(self, arena, D, device, src, dst, T, rows=ROWS):
        self.arena, self.D, self.device = arena, D, device
        self.src, self.dst, self.T, self.rows = src, dst, T, rows
        self.ss = np.dtype(NP_SRC[src]).itemsize
        self.ds = np.dtype(NP_DST[dst]).itemsize
        self.lead = GUARD + self.ds          # x, y begin one element in
        self.nbytes = self.lead + rows * T * self.ds + GUARD
        self.xbuf = torch.full((self.nbytes,), SENTINEL, dtype=torch.uint8,
                               device=device)
        self.ybuf = torch.full((self.nbytes,), SENTINEL, dtype=torch.uint8,
                               device=device)
        assert self.xbuf.data_ptr() % 16 == 0 and self.ybuf.data_ptr() % 16 == 0
        self.x_ptr = self.xbuf.data_ptr() + self.lead
        self.y_ptr = self.ybuf.data_ptr() + self.lead
        self.exp_x = np.full(self.nbytes, SENTINEL, np.uint8)
        self.exp_y = np.full(self.nbytes, SENTINEL, np.uint8)
        self.pieces = []
        self.read = []                       # every token the call reads

    def place(self, off, tokens):
        """Source tokens at arena byte `off`."""
        self.arena.write(off, tokens.tobytes())

    def piece(self, off, row, j0, tokens):
        """`tokens` (already placed at `off`) are tokens j0.. of `row`."""
        n = len(tokens)
        self.pieces.append((off, row, j0, n))
        self.read.append(tokens)
        wide = ref_widen(tokens, self.dst)
        T, ds = self.T, self.ds
        nx = min(j0 + n, T) - j0
        if nx > 0:
            a = self.lead + (row * T + j0) * ds
            self.exp_x[a:a + nx * ds] = np.frombuffer(
                wide[:nx].tobytes(), np.uint8)
        y0 = max(j0, 1)
        if j0 + n > y0:
            a = self.lead + (row * T + y0 - 1) * ds
            self.exp_y[a:a + (j0 + n - y0) * ds] = np.frombuffer(
                wide[y0 - j0:].tobytes(), np.uint8)

    def window(self, off, row, tokens, cuts=()):
        """A whole window placed at `off`, cut into pieces at `cuts`."""
        assert len(tokens) == self.T + 1
        self.place(off, tokens)
        edges = [0, *cuts, len(tokens)]
        for a, b in zip(edges, edges[1:]):
            assert a < b
            self.piece(off + a * self.ss, row, a, tokens[a:b])

    def run(self, vocab=0, order=None):
        pieces = self.pieces if order is None else \
            [self.pieces[i] for i in order]
        got = self.arena.token_windows(pieces, self.x_ptr, self.y_ptr,
                                       self.rows, self.T, self.D[self.src],
                                       self.D[self.dst], vocab)
        self.check()
        exp = ref_count(np.concatenate(self.read), self.src, vocab) \
            if self.read else 0
        assert got == exp, (got, exp)
        return got

    def check(self):
        """Written elements, untouched elements and guards, byte for byte."""
        for name, buf, exp in (("x", self.xbuf, self.exp_x),
                               ("y", self.ybuf, self.exp_y)):
            got = buf.cpu().numpy()
            if not np.array_equal(got, exp):
                i = int(np.nonzero(got != exp)[0][0])
                raise AssertionError(
                    f"{name} differs at byte {i} (element "
                    f"{(i - self.lead) // self.ds}): {got[i]:#x} != "
                    f"{exp[i]:#x}; {self.src}->{self.dst} T={self.T} "
                    f"pieces={self.pieces[:6]}")


def interleave(call):
    """Piece order with the rows' pieces interleaved."""
    by_row = {}
    for i, p in enumerate(call.pieces):
        by_row.setdefault(p[1], []).append(i)
    out, lists = [], list(by_row.values())
    while any(lists):
        for lst in lists:
            if lst:
                out.append(lst.pop(0))
    return out


def case_residues(arena, D, device, src, dst):
    """One window per call at source offsets 4096 + r, r in 0..15, for
    every small T; the row cycles so odd T starts rows off the 16-byte
    grid."""
    rng = np.random.default_rng(7)
    for T in T_SMALL:
        for r in range(16):
            c = Call(arena, D, device, src, dst, T)
            c.window(4096 + r, r % ROWS, make_tokens(rng, src, T + 1))
            c.run()


def case_splits(arena, D, device, src, dst):
    """Every two-piece split at j0 in 1, 2, T-1, T (a piece that is only
    token 0, one that is only token T), a three-piece split, all rows in
    one call with their pieces interleaved."""
    rng = np.random.default_rng(11)
    for T in T_SMALL:
        cuts = sorted({j for j in (1, 2, T - 1, T) if 1 <= j <= T})
        for k, j0 in enumerate(cuts):
            c = Call(arena, D, device, src, dst, T)
            for row in range(ROWS):
                j = cuts[(k + row) % len(cuts)]
                c.window(4096 * (row + 1) + 2 * row + 1 + k, row,
                         make_tokens(rng, src, T + 1), (j,))
            c.run(order=interleave(c))
        if T >= 2:
            c = Call(arena, D, device, src, dst, T)
            for row in range(ROWS):
                a = 1 + row % T if T > 2 else 1
                a = min(a, T - 1)
                c.window(4096 * (row + 1) + 3 * row + 1, row,
                         make_tokens(rng, src, T + 1), (a, T))
            c.run(order=interleave(c))


def long_call(arena, D, device, src, dst, tile, tokens_of):
    """Row 0 is one piece longer than two kernel tiles from an odd source
    offset; rows 1 and 2 arrive as short pieces in the same call."""
    T = 2 * tile + 3
    c = Call(arena, D, device, src, dst, T)
    c.window(4097, 0, tokens_of(0, T + 1))
    short = (1, 2, 3, 5, 64, 65, 129, tile - 1, tile, tile + 1)
    for row in (1, 2):
        cuts, at = [], 0
        for k in short[row - 1:]:
            at += k
            if at < T + 1:
                cuts.append(at)
        c.window((row + 1) * (1 << 16) + 2 * row + 1, row,
                 tokens_of(row, T + 1), cuts)
    return c


def case_long(arena, D, device, src, dst, tile):
    rng = np.random.default_rng(13)
    c = long_call(arena, D, device, src, dst, tile,
                  lambda row, n: make_tokens(rng, src, n))
    c.run(order=interleave(c))


VOCAB = 1000


def case_vocab(arena, D, device, src, dst, tile):
    """A known number of offending tokens: the first and the last token of
    windows, both sides of tile and piece edges, in several workgroups."""
    rng = np.random.default_rng(17)
    offenders = [VOCAB] + [v for v in SPECIALS[src] if v < 0 or v >= VOCAB]
    T = 2 * tile + 3

    def tokens_of(row, n):
        t = make_tokens(rng, src, n, below=VOCAB)
        at = [0, T, tile - 1, tile, 2 * tile - 1, 2 * tile, 2 * tile + 1,
              1, 2, 3, 6, 7, 70, 71, 135]
        for k, i in enumerate(at[:len(at) - row]):
            t[i] = offenders[(k + row) % len(offenders)]
        t[T // 2] = VOCAB - 1               # the largest id that passes
        return t

    results = []
    for vocab in (VOCAB, 0):
        c = long_call(arena, D, device, src, dst, tile, tokens_of)
        results.append(c.run(vocab=vocab, order=interleave(c)))
    assert results[0] >= 3 * 12 and results[1] == 0


def case_empty(arena, D, device, src, dst):
    c = Call(arena, D, device, src, dst, 8)
    assert c.run() == 0
    assert c.run(vocab=VOCAB) == 0


def reject_calls(D, cap, T=8, rows=ROWS):
    """(what, pieces, x_shift, y_shift, batch, seq_len, src, dst): calls
    that must raise ValueError; *_shift moves a pointer (None = null).  A
    valid piece comes first in each, so a call that ran anyway would show
    in the destinations.  A shift above 4096 is an absolute address."""
    ok = (4096, 0, 0, T + 1)
    u16, i64, i32 = D["U16"], D["I64"], D["I32"]
    big = 2 ** 64 - 1
    out = [("pair %s->%s" % (s, d), [ok], 0, 0, rows, T, D[s], D[d])
           for s, d in (("U32", "I32"), ("U16", "U16"), ("F32", "I64"),
                        ("U8", "I64"), ("U64", "I64"), ("I64", "I64"),
                        ("U16", "U8"))]
    out += [
        ("unknown src code", [ok], 0, 0, rows, T, 99, i64),
        ("unknown dst code", [ok], 0, 0, rows, T, u16, 99),
        ("seq_len 0", [ok], 0, 0, rows, 0, u16, i64),
        ("batch 0", [ok], 0, 0, 0, T, u16, i64),
        ("n 0", [ok, (4096, 1, 0, 0)], 0, 0, rows, T, u16, i64),
        ("row >= batch", [ok, (4096, rows, 0, 1)], 0, 0, rows, T, u16, i64),
        ("past window", [ok, (4096, 1, 1, T + 1)], 0, 0, rows, T, u16, i64),
        ("j0 past window", [ok, (4096, 1, T + 1, 1)], 0, 0, rows, T, u16, i64),
        ("past arena", [ok, (cap - 2 * T, 1, 0, T + 1)], 0, 0, rows, T,
         u16, i64),
        ("src_off overflow", [ok, (big, 1, 0, 2)], 0, 0, rows, T, u16, i64),
        ("n overflow", [ok, (4096, 1, 0, big)], 0, 0, rows, T, u16, i64),
        ("j0 overflow", [ok, (4096, 1, big, 2)], 0, 0, rows, T, u16, i64),
        ("x null", [ok], None, 0, rows, T, u16, i64),
        ("y null", [ok], 0, None, rows, T, u16, i64),
        ("x misaligned", [ok], 4, 0, rows, T, u16, i64),
        ("y misaligned", [ok], 0, 4, rows, T, u16, i64),
        ("x misaligned i32", [ok], 2, 0, rows, T, u16, i32),
        ("y odd", [ok], 0, 1, rows, T, u16, i32),
        ("size overflow", [ok], 0, 0, 2 ** 62, 2 ** 30, u16, i64),
        ("seq_len overflow", [ok], 0, 0, 1, big, u16, i64),
    ]
    return out


def run_rejects(arena, D, device, cap, raises, extra=()):
    """Every reject raises ValueError and leaves x and y untouched."""
    rng = np.random.default_rng(19)
    for what, pieces, xs, ys, batch, T, sc, dc in \
            list(reject_calls(D, cap)) + list(extra):
        c = Call(arena, D, device, "U16", "I64", 8)
        c.place(4096, make_tokens(rng, "U16", 9))
        x = 0 if xs is None else (xs if xs > 4096 else c.x_ptr + xs)
        y = 0 if ys is None else (ys if ys > 4096 else c.y_ptr + ys)
        with raises(ValueError):
            arena.token_windows(pieces, x, y, batch, T, sc, dc, 0)
            raise AssertionError(f"accepted: {what}")
        c.check()


# ------------------------------------------------------------- end to end

E2E = dict(src="U16", header=3, T=33, batch=4)


def e2e_files():
    """Two U16 files behind a 3-byte header: every token sits at an odd
    address and straddles each even block boundary it meets."""
    rng = np.random.default_rng(23)
    files = []
    for n in (1500, 700):
        toks = make_tokens(rng, "U16", n)
        files.append(bytes([1, 2, 3]) + toks.tobytes())
    return files


def e2e_reference(files, dst="I64"):
    xs, ys, ws = zip(*(ref_file_windows(b, E2E["src"], dst, E2E["header"],
                                        E2E["T"]) for b in files))
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ws)


def collect(loader):
    xs, ys = [], []
    for x, y in loader:
        assert x.is_contiguous() and y.is_contiguous()
        assert x.shape == y.shape and x.shape[1] == loader.seq_len
        xs.append(x.cpu().numpy())
        ys.append(y.cpu().numpy())
    return xs, ys


def check_order(loader, ref, order, drop_last=True):
    """The loader's batches are ref[order] cut into batches."""
    X, Y, _ = ref
    bs = E2E["batch"]
    xs, ys = collect(loader)
    n = len(order) // bs * bs if drop_last else len(order)
    assert len(xs) == len(loader) == -(-n // bs)
    assert sum(len(x) for x in xs) == n
    got_x, got_y = np.concatenate(xs), np.concatenate(ys)
    assert got_x.dtype == X.dtype
    assert np.array_equal(got_x, X[order[:n]])
    assert np.array_equal(got_y, Y[order[:n]])
    return xs


def check_loader(make, ref, raises_invalid):
    """The loader properties every tier has to show.  make(**kw) builds a
    loader over the two files; the caller closes what make returns via
    make.close_all()."""
    X, Y, W = ref
    n, bs = len(X), E2E["batch"]
    assert n % bs, "the short batch must exist"
    ident = list(range(n))

    ld = make()
    assert ld.num_windows == n
    check_order(ld, ref, ident)
    check_order(ld, ref, ident)             # replayed plans

    ld = make(drop_last=False)
    xs = check_order(ld, ref, ident, drop_last=False)
    assert len(xs[-1]) == n % bs

    ld = make(shuffle=True, seed=5)
    orders = []
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        order = list(range(n))
        random.Random(5 + epoch).shuffle(order)
        check_order(ld, ref, order)
        orders.append(order)
    assert orders[0] != orders[1]

    seen = []
    for rank in (0, 1):
        ld = make(rank=rank, world=2)
        cut = ident[:n - n % 2]
        mine = cut[rank::2]
        assert ld.num_windows == len(mine)
        check_order(ld, ref, mine)
        seen += mine
    assert sorted(seen) == ident[:n - n % 2]

    top = int(W.max())
    ld = make(vocab_size=top + 1)
    check_order(ld, ref, ident)
    ld = make(vocab_size=top)
    per_batch = [ref_count(W[b:b + bs].ravel(), E2E["src"], top)
                 for b in range(0, n - n % bs, bs)]
    first = next(i for i, c in enumerate(per_batch) if c)
    got = []
    with raises_invalid() as ei:
        for x, _y in ld:
            got.append(x)
    assert len(got) == first
    msg = str(ei.value)
    assert str(per_batch[first]) in msg and f"batch {first}" in msg, msg
