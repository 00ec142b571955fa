"""Shared cases for the packed-token tests (host twins and MI355X).

Nothing here imports project code: the expected eos indices and the five
tensors of a packed batch come from numpy, written from the definitions
(`flatnonzero`; x = d[i], y = d[i+1] or ignore, position_ids = pos0 + i,
doc_ids = doc, cu_seqlens[seq] = row*T + col).  The runners take the arena,
the dtype codes and the tile constants from the test module that calls
them, so the host and the GPU file run the same matrix; `device` is -1 with
CPU buffers or a GPU index with cuda buffers.  Every comparison is exact
equality on whole buffers, guard bytes included."""
import numpy as np

import token_doc_cases as dc
import token_window_cases as tc

Buf = dc.Buf
SOURCES = ("U16", "U32", "I32")
PAIRS = tc.PAIRS
NEXT, PAD = 1, 2
EOS = 5
OUTS = ("y", "pos", "doc", "cu")
ALL = frozenset(OUTS)
ARENA_AT = 4096                 # the cases place their sources from here on


def np_fill(n, dtype):
    """n elements whose bytes are the sentinel."""
    return np.full(n * np.dtype(dtype).itemsize, dc.SENTINEL,
                   np.uint8).view(dtype)


# ------------------------------------------------------------------ eos index

def eos_tokens(rng, src, n):
    """Random ids that are never EOS."""
    return rng.integers(EOS + 1, 30000, n).astype(tc.NP_SRC[src])


def ref_eos(spans, eos):
    """spans = [(tok0, tokens)]: the ascending file indices of eos."""
    out = [np.flatnonzero(t.astype(np.int64) == eos) + tok0
           for tok0, t in spans]
    return np.concatenate(out).astype(np.int64) if out else \
        np.zeros(0, np.int64)


def run_eos(arena, D, device, src, spans, eos=EOS, phase=1, capacities=None):
    """spans = [(tok0, tokens)] placed in the arena `phase` bytes past a
    64-byte boundary each: the pure count, then a write at every capacity
    (default: the total + 3)."""
    at = ARENA_AT
    call = []
    for tok0, t in spans:
        at = (at + 63) // 64 * 64 + phase
        arena.write(at, t.tobytes())
        call.append((at, tok0, len(t)))
        at += t.nbytes
    exp = ref_eos(spans, eos)
    tag = f"{src} phase={phase} n={[len(t) for _, t in spans]}"
    assert arena.token_eos_index(call, D[src], eos, 0, 0) == len(exp), tag
    for cap in (len(exp) + 3,) if capacities is None else capacities:
        out = Buf(device, cap, 8)
        got = arena.token_eos_index(call, D[src], eos, out.ptr if cap else 0,
                                    cap)
        assert got == len(exp), (got, len(exp), tag)
        out.expect(exp[:cap], f"eos index cap={cap} " + tag)


def eos_sizes(C):
    return (1, 2, C - 1, C, C + 1, 2 * C + 3)


def case_eos_sizes(arena, D, device, src, C):
    """Every span length: no eos, every token, the first and the last
    token, density ~1/8 with runs."""
    rng = np.random.default_rng(61)
    for n in eos_sizes(C):
        base = eos_tokens(rng, src, n)
        run_eos(arena, D, device, src, [(0, base)])
        run_eos(arena, D, device, src, [(7, np.full_like(base, EOS))])
        t = base.copy()
        t[[0, n - 1]] = EOS
        run_eos(arena, D, device, src, [(0, t)], phase=0)
        t = base.copy()
        t[rng.integers(0, 8, n) == 0] = EOS
        t[n // 2:n // 2 + 5] = EOS                 # a run of eos
        run_eos(arena, D, device, src, [(3, t)])


def case_eos_phases(arena, D, device, src, C):
    """The source at each of the 16 byte phases."""
    rng = np.random.default_rng(67)
    for phase in range(16):
        for n in (19, C + 1):
            t = eos_tokens(rng, src, n)
            t[rng.integers(0, 6, n) == 0] = EOS
            t[[0, n - 1]] = EOS
            run_eos(arena, D, device, src, [(0, t)], phase=phase)


def case_eos_edges(arena, D, device, src, C):
    """eos on both sides of a tile edge; three spans with gaps in tok0; a
    capacity below the total and a null pointer."""
    rng = np.random.default_rng(71)
    for cols in ((C - 1,), (C,), (C - 1, C), (C - 2, C - 1, C, C + 1)):
        t = eos_tokens(rng, src, 2 * C + 3)
        t[list(cols)] = EOS
        run_eos(arena, D, device, src, [(0, t)], phase=3)
    spans = []
    for tok0, n in ((10, C + 1), (10 + C + 1, 2), (5 * C, C - 1)):
        t = eos_tokens(rng, src, n)
        t[rng.integers(0, 4, n) == 0] = EOS
        t[[0, n - 1]] = EOS
        spans.append((tok0, t))
    total = len(ref_eos(spans, EOS))
    assert total > 8
    run_eos(arena, D, device, src, spans, phase=2,
            capacities=(total, total + 3, total - 1, 5, 1, 0))


def case_eos_long(arena, D, device, C, wg=256):
    """More tiles than one pass of the offsets workgroup holds, mostly
    without hits."""
    rng = np.random.default_rng(73)
    n = (wg + 3) * C + 5
    t = eos_tokens(rng, "U16", n)
    t[[0, C - 1, C, 17 * C + 3, wg * C - 1, wg * C, n - 1]] = EOS
    run_eos(arena, D, device, "U16", [(0, t)], phase=1)


def case_eos_full_width(arena, D, device):
    """A U32 eos above 2^31, and negative I32 ids next to a matching one:
    the low bits alone never match."""
    big = 2 ** 31 + EOS
    t = np.array([EOS, big, 2 ** 32 - 1, big, 7, big - 2 ** 31], np.uint32)
    run_eos(arena, D, device, "U32", [(0, t)], eos=big)
    run_eos(arena, D, device, "U32", [(0, t)], eos=2 ** 32 - 1)
    t = np.array([-1, EOS, EOS - 2 ** 31, -EOS, EOS, -2 ** 31, 0], np.int32)
    run_eos(arena, D, device, "I32", [(0, t)])
    run_eos(arena, D, device, "I32", [(0, t)], eos=0)
    t = np.array([0xFFFF, EOS, 0x8005, 0xFFFF], np.uint16)
    run_eos(arena, D, device, "U16", [(0, t)], eos=0xFFFF)


def eos_rejects(D, cap):
    """(what, spans, dtype code, eos, out shift or None, capacity)."""
    u16 = D["U16"]
    return [
        ("unknown dtype", [(0, 0, 4)], 99, EOS, 0, 4),
        ("dtype F32", [(0, 0, 4)], D["F32"], EOS, 0, 4),
        ("dtype I64", [(0, 0, 4)], D["I64"], EOS, 0, 4),
        ("eos negative", [(0, 0, 4)], u16, -1, 0, 4),
        ("eos past u16", [(0, 0, 4)], u16, 2 ** 16, 0, 4),
        ("eos past i32", [(0, 0, 4)], D["I32"], 2 ** 31, 0, 4),
        ("eos past u32", [(0, 0, 4)], D["U32"], 2 ** 32, 0, 4),
        ("empty span", [(0, 0, 0)], u16, EOS, 0, 4),
        ("out of bounds", [(cap - 6, 0, 4)], u16, EOS, 0, 4),
        ("src overflow", [(2 ** 64 - 2, 0, 4)], u16, EOS, 0, 4),
        ("n overflow", [(0, 0, 2 ** 63)], u16, EOS, 0, 4),
        ("tok0 overflow", [(0, 2 ** 64 - 2, 4)], u16, EOS, 0, 4),
        ("descending", [(0, 8, 4), (64, 0, 4)], u16, EOS, 0, 4),
        ("overlapping", [(0, 0, 4), (64, 3, 4)], u16, EOS, 0, 4),
        ("null out", [(0, 0, 4)], u16, EOS, None, 4),
        ("misaligned out", [(0, 0, 4)], u16, EOS, 4, 4),
        ("capacity overflow", [(0, 0, 4)], u16, EOS, 0, 2 ** 61),
    ]


def run_eos_rejects(arena, D, device, cap, raises, extra=()):
    """Every reject raises ValueError and leaves the output as it was.
    `extra` entries carry an absolute pointer in place of the shift."""
    arena.write(0, np.full(64, EOS, np.uint16).tobytes())
    for what, spans, code, eos, shift, capacity in \
            list(eos_rejects(D, cap)) + list(extra):
        out = Buf(device, 8, 8)
        ptr = 0 if shift is None else \
            (shift if shift > 4096 else out.ptr + shift)
        with raises(ValueError):
            arena.token_eos_index(spans, code, eos, ptr, capacity)
            raise AssertionError(f"accepted: {what}")
        out.expect(np.zeros(0, np.int64), "out after " + what)


# ----------------------------------------------------------------- pack kernel

class PackCall:
    """One Arena.token_pack call on sentinel-filled outputs.  The expected
    tensors are built piece by piece from the definitions."""

    def __init__(self, arena, D, device, src, dst, rows, T, want=ALL,
                 pad_id=-7, ignore=-100, lead_el=1):
        self.arena, self.D, self.device = arena, D, device
        self.src, self.dst, self.rows, self.T = src, dst, rows, T
        self.want, self.pad_id, self.ignore = want, pad_id, ignore
        self.lead_el = lead_el
        self.ss = np.dtype(tc.NP_SRC[src]).itemsize
        self.dt = tc.NP_DST[dst]
        self.segs, self.pieces, self.read = [], [], []
        self.at = ARENA_AT
        n = rows * T
        self.x, self.y = np_fill(n, self.dt), np_fill(n, self.dt)
        self.pos, self.doc = np_fill(n, self.dt), np_fill(n, self.dt)

    def place(self, tokens, phase):
        """Source tokens `phase` bytes past a 64-byte boundary."""
        self.at = (self.at + 63) // 64 * 64 + phase
        off = self.at
        self.arena.write(off, tokens.tobytes())
        self.at += tokens.nbytes
        return off

    def seg(self, row, col, d, has_next, pos0=0, doc=0, cuts=(), phase=1,
            keep=None):
        """A source segment whose tokens d (n of them, +1 with has_next)
        are cut into pieces at `cuts`, each piece placed on its own at a
        byte phase that walks on from `phase`; keep: the pieces passed."""
        n = len(d) - int(has_next)
        si = len(self.segs)
        self.segs.append([row, col, n, pos0, doc, si, NEXT if has_next else 0])
        edges = [0, *cuts, len(d)]
        at = row * self.T + col
        wide = tc.ref_widen(d, self.dst)
        for i, (a, b) in enumerate(zip(edges, edges[1:])):
            assert a < b
            if keep is not None and i not in keep:
                continue
            off = self.place(d[a:b], (phase + 5 * i) % 16)
            self.pieces.append((off, si, a, b - a))
            self.read.append(d[a:b])
            for j in range(a, b):
                if j < n:
                    self.x[at + j] = wide[j]
                    self.pos[at + j] = pos0 + j
                    self.doc[at + j] = doc
                if j >= 1:
                    self.y[at + j - 1] = wide[j]
            if not has_next and a <= n - 1 < b:
                self.y[at + n - 1] = self.ignore
        return si

    def pad(self, row, col, n):
        self.segs.append([row, col, n, 0, 0, len(self.segs), PAD])
        at = row * self.T + col
        self.x[at:at + n] = self.pad_id
        self.y[at:at + n] = self.ignore
        self.pos[at:at + n] = np.arange(n)
        self.doc[at:at + n] = -1

    def run(self, vocab=0):
        n, item = self.rows * self.T, np.dtype(self.dt).itemsize
        le = self.lead_el
        # the segments may be listed in any order: seq says where cu goes
        order = sorted(range(len(self.segs)),
                       key=lambda i: (self.segs[i][0], self.segs[i][1]))
        for seq, i in enumerate(order):
            self.segs[i][5] = seq
        cu = np_fill(len(self.segs) + 1, np.int32)
        for s in self.segs:
            cu[s[5]] = s[0] * self.T + s[1]
        cu[len(self.segs)] = self.rows * self.T
        xb = Buf(self.device, n, item, le)
        yb = Buf(self.device, n, item, le + 1) if "y" in self.want else None
        pb = Buf(self.device, n, item, le + 2) if "pos" in self.want else None
        db = Buf(self.device, n, item, le + 3) if "doc" in self.want else None
        cb = Buf(self.device, len(cu), 4, le) if "cu" in self.want else None
        got = self.arena.token_pack(
            [tuple(s) for s in self.segs], self.pieces, xb.ptr,
            yb.ptr if yb else 0, pb.ptr if pb else 0, db.ptr if db else 0,
            cb.ptr if cb else 0, self.rows, self.T, self.D[self.src],
            self.D[self.dst], self.pad_id, self.ignore, vocab)
        tag = (f"{self.src}->{self.dst} rows={self.rows} T={self.T} "
               f"want={sorted(self.want)} lead={le}")
        xb.expect(self.x, "x " + tag)
        for b, exp, name in ((yb, self.y, "y"), (pb, self.pos, "pos"),
                             (db, self.doc, "doc"), (cb, cu, "cu")):
            if b:
                b.expect(exp, f"{name} {tag}")
        exp = tc.ref_count(np.concatenate(self.read), self.src, vocab) \
            if self.read else 0
        assert got == exp, (got, exp, tag)
        return got


def seg_sizes(dst, C):
    K = 16 // np.dtype(tc.NP_DST[dst]).itemsize
    return sorted({1, 2, K - 1, K, K + 1, C - 1, C, C + 1})


def case_pack_sizes(arena, D, device, src, dst, C):
    """Every n of the matrix, has_next on and off, in a row of its own at
    a column that walks through the phases, padding in front and behind;
    a pad segment of one column and one of a whole row.  T is odd, so the
    rows start at every 16-byte phase.  Both signs of pad_id and
    ignore_index."""
    rng = np.random.default_rng(83)
    ns = seg_sizes(dst, C)
    T = C + 5
    assert T % 2 == 1
    for has_next, pad_id, ignore in ((False, -7, -100), (True, 3, 12345)):
        c = PackCall(arena, D, device, src, dst, len(ns) + 2, T,
                     pad_id=pad_id, ignore=ignore)
        for r, n in enumerate(ns):
            col = min(r % 5, T - n)
            if col:
                c.pad(r, 0, col)
            c.seg(r, col, tc.make_tokens(rng, src, n + int(has_next)),
                  has_next, pos0=r * T, doc=r + 1, phase=(3 * r + 1) % 16)
            if col + n < T:
                c.pad(r, col + n, T - col - n)
        c.seg(len(ns), 0, tc.make_tokens(rng, src, T - 1 + int(has_next)),
              has_next, phase=0)
        c.pad(len(ns), T - 1, 1)
        c.pad(len(ns) + 1, 0, T)
        c.run()


def case_pack_phases(arena, D, device, src, dst):
    """The outputs 0..3 elements past the 16-byte grid and col at every
    phase of it, segments side by side in a row."""
    rng = np.random.default_rng(89)
    K = 16 // np.dtype(tc.NP_DST[dst]).itemsize
    T = 4 * K + 9
    for lead_el in range(4):
        c = PackCall(arena, D, device, src, dst, K + 1, T, lead_el=lead_el)
        for r in range(K + 1):
            if r:
                c.seg(r, 0, tc.make_tokens(rng, src, r), False, doc=0)
            n = 2 * K + 1
            c.seg(r, r, tc.make_tokens(rng, src, n + 1), True, pos0=T,
                  doc=1, phase=r)
            c.seg(r, r + n, tc.make_tokens(rng, src, T - r - n), False,
                  pos0=3, doc=2, phase=15 - r)
        c.run()


def case_pack_cuts(arena, D, device, src, dst, C):
    """A segment cut into two pieces at every position, into single
    tokens, and a long one cut after its first token and before token n:
    the x-only first token and the y-only token n are pieces of their own.
    The pieces sit at odd and even byte offsets."""
    rng = np.random.default_rng(97)
    n = 9
    for has_next in (False, True):
        tok = n + int(has_next)
        T = n + 2
        c = PackCall(arena, D, device, src, dst, tok + 1, T)
        for r, cut in enumerate(range(1, tok)):
            c.seg(r, 1, tc.make_tokens(rng, src, tok), has_next, doc=r,
                  cuts=(cut,), phase=r % 16)
            c.pad(r, 0, 1)
            c.pad(r, n + 1, 1)
        for r in (tok - 1, tok):
            c.seg(r, 2, tc.make_tokens(rng, src, tok), has_next,
                  cuts=tuple(range(1, tok)), phase=7 + r)
        c.run()
        # pieces passed in part: the rest of the segment stays untouched
        c = PackCall(arena, D, device, src, dst, 3, T)
        for r, keep in enumerate(((0,), (2,), (1,))):
            c.seg(r, 1, tc.make_tokens(rng, src, tok), has_next,
                  cuts=(1, tok - 1), keep=keep)
        c.run()
        long_n = 2 * C + 3
        c = PackCall(arena, D, device, src, dst, 2, long_n + 1)
        c.seg(0, 1, tc.make_tokens(rng, src, long_n + int(has_next)),
              has_next, pos0=7, cuts=(1, long_n - 1 + int(has_next)))
        c.seg(1, 0, tc.make_tokens(rng, src, long_n + int(has_next)),
              has_next, cuts=(C - 1, C + 2), phase=3)
        c.run()


def case_pack_outputs(arena, D, device, src, dst, C):
    """Each optional output null in turn, and all of them."""
    rng = np.random.default_rng(101)
    T = C + 3
    for want in ([ALL - {o} for o in OUTS] + [frozenset()]):
        c = PackCall(arena, D, device, src, dst, 2, T, want=want)
        c.seg(0, 0, tc.make_tokens(rng, src, 6), True, cuts=(1, 5))
        c.seg(0, 5, tc.make_tokens(rng, src, T - 8), False, doc=1)
        c.pad(0, T - 3, 3)
        c.seg(1, 0, tc.make_tokens(rng, src, T), False, phase=2)
        c.run()


def case_pack_vocab(arena, D, device, src, dst, C):
    """The count: offenders in the body of a tile, at its edges, as the
    x-only and the y-only token; a token that goes to x and y counts once,
    the token two segments share is read twice and counts twice."""
    rng = np.random.default_rng(103)
    V = tc.VOCAB
    over = {"U16": 0xFFFF, "U32": 2 ** 31, "I32": -1}[src]
    T = C + 9
    for spots in ((), (0,), (T,), (3, 4, C - 1, C, C + 1), tuple(range(T + 1))):
        c = PackCall(arena, D, device, src, dst, 3, T)
        d = tc.make_tokens(rng, src, T + 1, below=V)
        d[list(spots)] = over
        c.seg(0, 0, d, True, cuts=(1, T))
        e = tc.make_tokens(rng, src, 8, below=V)
        e[0] = d[T]                                   # the shared token
        c.seg(1, 0, e, False, pos0=T)
        c.pad(1, 8, T - 8)
        c.pad(2, 0, T)
        assert c.run(vocab=V) == len(spots) + (1 if T in spots else 0)
        assert c.run(vocab=0) == 0


def pack_rejects(D, cap, rows=3, T=8):
    """(what, kw): changes to a valid call that must raise ValueError.
    Shifts move a pointer off its buffer's start; None is the null
    pointer."""
    u16, i64, i32 = D["U16"], D["I64"], D["I32"]
    big = 2 ** 64 - 1
    seg = (0, 0, 4, 0, 0, 0, NEXT)
    pad = (0, 4, 4, 0, 0, 1, PAD)

    def segs(s=seg, p=pad):
        return dict(segments=[s, p])
    return [
        ("unknown src", dict(sdt=99)),
        ("unknown dst", dict(ddt=99)),
        ("U32 -> I32", dict(sdt=D["U32"], ddt=i32)),
        ("F32 source", dict(sdt=D["F32"])),
        ("U16 target", dict(ddt=u16)),
        ("rows 0", dict(rows=0)),
        ("seq_len 0", dict(T=0)),
        ("segment n 0", segs((0, 0, 0, 0, 0, 0, 0))),
        ("segment row", segs((rows, 0, 4, 0, 0, 0, NEXT))),
        ("segment past its row", segs((0, 1, T, 0, 0, 0, NEXT))),
        ("segment col overflow", segs((0, big, 2, 0, 0, 0, NEXT))),
        ("seq outside", segs((0, 0, 4, 0, 0, 2, NEXT))),
        ("flags 3", segs((0, 0, 4, 0, 0, 0, 3))),
        ("pos0 overflow", segs((0, 0, 4, big, 0, 0, NEXT))),
        ("pos0 past i32", dict(ddt=i32, sdt=u16,
                               segments=[(0, 0, 4, 2 ** 31 - 2, 0, 0, NEXT),
                                         pad])),
        ("piece segment", dict(pieces=[(0, 2, 0, 4)])),
        ("piece k 0", dict(pieces=[(0, 0, 0, 0)])),
        ("piece past n + next", dict(pieces=[(0, 0, 0, 6)])),
        ("piece past n", dict(pieces=[(0, 0, 1, 4)],
                              segments=[(0, 0, 4, 0, 0, 0, 0), pad])),
        ("piece j0 overflow", dict(pieces=[(0, 0, big, 2)])),
        ("piece on a pad", dict(pieces=[(0, 1, 0, 2)])),
        ("arena bounds", dict(pieces=[(cap - 6, 0, 0, 4)])),
        ("arena overflow", dict(pieces=[(big - 1, 0, 0, 4)])),
        ("size overflow", dict(rows=2 ** 62, T=2 ** 30)),
        ("bytes overflow", dict(rows=1, T=2 ** 61)),
        ("x null", dict(x=None)),
        ("x misaligned", dict(x=4)),
        ("y misaligned", dict(y=4)),
        ("pos misaligned", dict(pos=2)),
        ("doc misaligned", dict(doc=1)),
        ("cu misaligned", dict(cu=2)),
        ("cu needs < 2^31", dict(rows=2 ** 16, T=2 ** 15, y=None, pos=None,
                                 doc=None)),
        ("pad_id past i32", dict(ddt=i32, pad_id=2 ** 31)),
        ("ignore past i32", dict(ddt=i32, ignore=-2 ** 31 - 1)),
    ]


def run_pack_rejects(arena, D, device, cap, raises, extra=()):
    """Every reject raises ValueError and leaves all five buffers as they
    were.  `extra` entries carry absolute pointers in place of shifts."""
    rows, T = 3, 8
    arena.write(0, np.arange(64, dtype=np.uint16).tobytes())
    base = dict(segments=[(0, 0, 4, 0, 0, 0, NEXT), (0, 4, 4, 0, 0, 1, PAD)],
                pieces=[(0, 0, 0, 5)], x=0, y=0, pos=0, doc=0, cu=0,
                rows=rows, T=T, sdt=D["U16"], ddt=D["I64"], pad_id=0,
                ignore=-100, vocab=0)
    for what, kw in list(pack_rejects(D, cap, rows, T)) + list(extra):
        a = dict(base)
        a.update(kw)
        bufs = {k: Buf(device, rows * T, 8) for k in ("x", "y", "pos", "doc")}
        bufs["cu"] = Buf(device, 3, 4)

        def at(name):
            shift = a[name]
            if shift is None:
                return 0
            return shift if shift > 4096 else bufs[name].ptr + shift
        with raises(ValueError):
            arena.token_pack(a["segments"], a["pieces"], at("x"), at("y"),
                             at("pos"), at("doc"), at("cu"), a["rows"], a["T"],
                             a["sdt"], a["ddt"], a["pad_id"], a["ignore"],
                             a["vocab"])
            raise AssertionError(f"accepted: {what}")
        for name, b in bufs.items():
            b.expect(np.zeros(0, np.uint8), f"{name} after {what}")
    # the valid call is accepted
    bufs = {k: Buf(device, rows * T, 8) for k in ("x", "y", "pos", "doc")}
    bufs["cu"] = Buf(device, 3, 4)
    arena.token_pack(base["segments"], base["pieces"],
                     *(bufs[k].ptr for k in ("x", "y", "pos", "doc", "cu")),
                     rows, T, base["sdt"], base["ddt"], 0, -100, 0)


# ------------------------------------------------------------------ end to end

E2E = dict(T=8, batch=3, src="U16", header=3, eos=0, pad=0, ignore=-100)


def e2e_docs():
    """The documents of the two files: lengths 1, T and 2T+1, consecutive
    eos, and an unterminated tail in each file."""
    rng = np.random.default_rng(107)
    T = E2E["T"]
    files = []
    for lens, tail in (((5, 1, 1, T, 2 * T + 1, 3, 1, T - 1, 2, T + 1), 4),
                       ((2 * T, 1, 7, 3 * T + 2, 6, T, 1, 1), 2 * T + 3)):
        docs = []
        for n in lens:
            d = rng.integers(1, 60000, n).astype(np.uint16)
            d[-1] = E2E["eos"]
            docs.append(d)
        docs.append(rng.integers(1, 60000, tail).astype(np.uint16))
        files.append(docs)
    return files


def e2e_files(files):
    return [b"\x01" * E2E["header"] + np.concatenate(docs).tobytes()
            for docs in files]


def doc_chunks(docs, T, ignore):
    """The chunks (pos0, x, y) every document has to appear as, sorted."""
    out = []
    for d in docs:
        d = d.astype(np.int64)
        for t0 in range(0, len(d), T):
            x = d[t0:t0 + T]
            y = np.append(d[t0 + 1:t0 + T + 1], [ignore])[:len(x)]
            out.append((t0, tuple(x.tolist()), tuple(y.tolist())))
    return sorted(out)


def batch_chunks(x, y, docs, T, B, pad_id, ignore):
    """The chunks of one yielded batch, read in (row, col) order and split
    at doc_ids; checks the padding on the way."""
    x, y = x.cpu().numpy().astype(np.int64), y.cpu().numpy().astype(np.int64)
    pos = docs["position_ids"].cpu().numpy().astype(np.int64)
    doc = docs["doc_ids"].cpu().numpy().astype(np.int64)
    cu = docs["cu_seqlens"].cpu().numpy().astype(np.int64)
    out, starts = [], []
    for r in range(B):
        c = 0
        while c < T:
            e = c
            while e < T and doc[r, e] == doc[r, c]:
                e += 1
            starts.append(r * T + c)
            if doc[r, c] == -1:
                assert e == T, "padding sits at the row's tail"
                assert (x[r, c:] == pad_id).all()
                assert (y[r, c:] == ignore).all()
                assert (pos[r, c:] == np.arange(T - c)).all()
            else:
                assert (np.diff(pos[r, c:e]) == 1).all()
                out.append((int(pos[r, c]), tuple(x[r, c:e].tolist()),
                            tuple(y[r, c:e].tolist())))
            c = e
    assert cu.tolist() == starts + [B * T]
    assert docs["max_seqlen"] == int(np.diff(cu).max())
    return out
