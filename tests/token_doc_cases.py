"""Shared cases for the token-document tests (host twin and MI355X).

Nothing here imports project code: the expected position ids, document ids
and cu_seqlens come from numpy (`cumsum`, `maximum.accumulate`,
`flatnonzero`).  The runners take the entry point, the dtype codes and the
chunk constant from the test module that calls them, so the host and the GPU
file run the same matrix; `device` is -1 with CPU tensors or a GPU index with
cuda tensors.  Every comparison is exact integer equality on whole buffers,
guard bytes included."""
import numpy as np
import torch

DTYPES = ("I32", "I64")
NP = {"I32": np.int32, "I64": np.int64}
TORCH = {"I32": torch.int32, "I64": torch.int64}
SENTINEL = 0xAB
GUARD = 16
EOS = 5
ROWS = (1, 3)
OUTPUTS = ("pos", "doc", "cu")
ALL = frozenset(OUTPUTS)


def sizes(C):
    return (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1,
            2 * C + 3)


# ------------------------------------------------------------- reference

def reference(x, eos):
    """x: [rows, T] integer array.  Returns position_ids, doc_ids (x's
    dtype), cu_seqlens (int32), n_seqs, max_seqlen."""
    rows, T = x.shape
    is_eos = x == eos
    ind = is_eos.astype(np.int64)
    doc = np.cumsum(ind, axis=1) - ind
    shifted = np.zeros_like(is_eos)
    shifted[:, 1:] = is_eos[:, :-1]
    col = np.broadcast_to(np.arange(T, dtype=np.int64), (rows, T))
    start = np.maximum.accumulate(np.where(shifted, col, 0), axis=1)
    pos = col - start
    first = shifted.copy()
    first[:, 0] = True
    starts = np.flatnonzero(first.ravel())
    cu = np.concatenate([starts, [rows * T]]).astype(np.int32)
    return (pos.astype(x.dtype), doc.astype(x.dtype), cu, len(starts),
            int(np.diff(cu.astype(np.int64)).max()))


# ----------------------------------------------------------------- runner

def tdev(device):
    return "cpu" if device < 0 else f"cuda:{device}"


class Buf:
    """`n` elements of `itemsize` bytes between sentinel guards, starting
    `lead_el` elements past a 16-byte boundary."""

    def __init__(self, device, n, itemsize, lead_el=1):
        self.lead = GUARD + lead_el * itemsize
        self.n, self.itemsize = n, itemsize
        self.nbytes = self.lead + n * itemsize + GUARD
        self.t = torch.full((self.nbytes,), SENTINEL, dtype=torch.uint8,
                            device=tdev(device))
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lead

    def put(self, arr):
        raw = torch.from_numpy(np.frombuffer(arr.tobytes(), np.uint8).copy())
        self.t[self.lead:self.lead + raw.numel()] = raw.to(self.t.device)

    def expect(self, arr, what):
        """The first len(arr) elements are arr; every other byte is still
        the sentinel."""
        exp = np.full(self.nbytes, SENTINEL, np.uint8)
        raw = np.frombuffer(arr.tobytes(), np.uint8)
        exp[self.lead:self.lead + len(raw)] = raw
        got = self.t.cpu().numpy()
        if not np.array_equal(got, exp):
            i = int(np.nonzero(got != exp)[0][0])
            raise AssertionError(
                f"{what} differs at byte {i} (element "
                f"{(i - self.lead) // self.itemsize}): {got[i]:#x} != "
                f"{exp[i]:#x}")


def run_case(fn, D, device, dt, x, eos=EOS, want=ALL, lead_el=1):
    """One token_docs call on sentinel-filled outputs; x too sits one
    element (lead_el) past the 16-byte grid of a larger buffer."""
    x = np.ascontiguousarray(x.astype(NP[dt]))
    rows, T = x.shape
    item = x.dtype.itemsize
    xb = Buf(device, rows * T, item, lead_el)
    xb.put(x)
    pb = Buf(device, rows * T, item, lead_el) if "pos" in want else None
    db = Buf(device, rows * T, item, lead_el + 1) if "doc" in want else None
    cb = Buf(device, rows * T + 1, 4, lead_el) if "cu" in want else None
    got = fn(device, xb.ptr, rows, T, D[dt], eos,
             pb.ptr if pb else 0, db.ptr if db else 0, cb.ptr if cb else 0)
    pos, doc, cu, n_seqs, max_seqlen = reference(x, eos)
    tag = f"{dt} rows={rows} T={T} want={sorted(want)}"
    assert tuple(got) == (n_seqs, max_seqlen), (got, n_seqs, max_seqlen, tag)
    xb.expect(x, "x " + tag)
    if pb:
        pb.expect(pos, "position_ids " + tag)
    if db:
        db.expect(doc, "doc_ids " + tag)
    if cb:
        cb.expect(cu, "cu_seqlens " + tag)


def filler(rng, rows, T, dt):
    """Random ids that are never EOS."""
    x = rng.integers(EOS + 1, 30000, (rows, T))
    return x.astype(NP[dt])


def case_sizes(fn, D, device, dt, C):
    """Every T of the matrix, rows 1 and 3: no eos, every token, column 0
    only, column T-1 only, density ~1/8 and ~1/300.  Odd T with 3 rows puts
    the rows at different 16-byte phases."""
    rng = np.random.default_rng(31)
    for T in sizes(C):
        for rows in ROWS:
            base = filler(rng, rows, T, dt)
            run_case(fn, D, device, dt, base)
            run_case(fn, D, device, dt, np.full((rows, T), EOS))
            x = base.copy()
            x[:, 0] = EOS
            run_case(fn, D, device, dt, x)
            x = base.copy()
            x[:, T - 1] = EOS
            run_case(fn, D, device, dt, x)
            for every in (8, 300):
                x = base.copy()
                x[rng.integers(0, every, (rows, T)) == 0] = EOS
                run_case(fn, D, device, dt, x)


def case_phases(fn, D, device, dt, C):
    """x and the outputs starting 0..3 elements past the 16-byte grid, with
    T that walks the rows through the phases."""
    rng = np.random.default_rng(37)
    for lead_el in range(4):
        for T in (9, 257, C + 1):
            x = filler(rng, 3, T, dt)
            x[rng.integers(0, 8, (3, T)) == 0] = EOS
            run_case(fn, D, device, dt, x, lead_el=lead_el)


def case_chunk_edges(fn, D, device, dt, C):
    """A boundary exactly at a chunk edge: eos at C-1, at C, at both; one
    eos in chunk 0 of a three-chunk row (the carry crosses an eos-free
    chunk); eos in row 0 only of three rows (carries reset per row, the
    sequence count does not)."""
    rng = np.random.default_rng(41)
    T = 2 * C + 3
    for rows in ROWS:
        for cols in ((C - 1,), (C,), (C - 1, C), (3,), (C - 1, 2 * C - 1, 2 * C)):
            x = filler(rng, rows, T, dt)
            for c in cols:
                x[:, c] = EOS
            run_case(fn, D, device, dt, x)
    x = filler(rng, 3, T, dt)
    x[0, [2, C - 1, C + 7, 2 * C + 2]] = EOS
    run_case(fn, D, device, dt, x)
    x = filler(rng, 3, T, dt)
    x[1, T - 1] = EOS                       # an eos in column T-1 starts nothing
    x[2, 0] = EOS
    run_case(fn, D, device, dt, x)


def case_single_outputs(fn, D, device, dt, C):
    """Each output alone, each pair, and none: skipped ones are passed as 0
    and the returned pair does not change."""
    rng = np.random.default_rng(43)
    for T in (65, C + 1):
        x = filler(rng, 3, T, dt)
        x[rng.integers(0, 8, (3, T)) == 0] = EOS
        for want in ((), ("pos",), ("doc",), ("cu",), ("pos", "doc"),
                     ("pos", "cu"), ("doc", "cu")):
            run_case(fn, D, device, dt, x, want=frozenset(want))


def case_full_width(fn, D, device, C):
    """I64 ids holding eos + 2**32 and negative values, I32 negative values:
    none of them is an eos.  An eos with high bits set in I64."""
    rng = np.random.default_rng(47)
    T = 300
    x = filler(rng, 3, T, "I64")
    x[:, 10::7] = EOS + 2 ** 32
    x[:, 11::13] = -1
    x[:, 12::17] = EOS - 2 ** 32
    x[:, 13::19] = -(2 ** 63)
    x[1, [20, 21, 150]] = EOS
    run_case(fn, D, device, "I64", x)
    big = EOS + 2 ** 32
    run_case(fn, D, device, "I64", x, eos=big)
    run_case(fn, D, device, "I64", x, eos=2 ** 63 - 1)
    x = filler(rng, 3, T, "I32")
    x[:, 11::13] = -1
    x[:, 12::17] = -(2 ** 31)
    x[:, 13::19] = EOS - 2 ** 31
    x[2, [0, 1, 299]] = EOS
    run_case(fn, D, device, "I32", x)
    x[0, 5] = 2 ** 31 - 1
    run_case(fn, D, device, "I32", x, eos=2 ** 31 - 1)
    run_case(fn, D, device, "I32", x, eos=0)


def case_long_table(fn, D, device, C):
    """600 rows of C+1 columns: 1200 chunks, more than one pass of the
    offsets workgroup; eos around the chunk edge and at the row ends."""
    rng = np.random.default_rng(53)
    rows, T = 600, C + 1
    x = filler(rng, rows, T, "I64")
    x[rng.integers(0, 300, (rows, T)) == 0] = EOS
    x[::3, C - 1] = EOS
    x[1::5, C] = EOS
    x[2::7, 0] = EOS
    run_case(fn, D, device, "I64", x)


def reject_calls(D):
    """(what, dtype code, rows, T, eos, x_shift, pos_shift, doc_shift,
    cu_shift): calls that must raise ValueError.  A shift moves a pointer
    off its buffer's start; None is the null pointer."""
    i32, i64 = D["I32"], D["I64"]
    big = 2 ** 64 - 1
    return [
        ("unknown dtype", 99, 3, 8, EOS, 0, 0, 0, 0),
        ("dtype U16", D["U16"], 3, 8, EOS, 0, 0, 0, 0),
        ("dtype U32", D["U32"], 3, 8, EOS, 0, 0, 0, 0),
        ("dtype U64", D["U64"], 3, 8, EOS, 0, 0, 0, 0),
        ("dtype F32", D["F32"], 3, 8, EOS, 0, 0, 0, 0),
        ("rows 0", i64, 0, 8, EOS, 0, 0, 0, 0),
        ("seq_len 0", i64, 3, 0, EOS, 0, 0, 0, 0),
        ("size overflow", i64, 2 ** 62, 2 ** 30, EOS, 0, 0, 0, 0),
        ("seq_len overflow", i64, 1, big, EOS, 0, 0, 0, 0),
        ("bytes overflow", i64, 1, 2 ** 61, EOS, 0, 0, 0, 0),
        ("cu needs < 2^31", i64, 2 ** 16, 2 ** 15, EOS, 0, None, None, 0),
        ("x null", i64, 3, 8, EOS, None, 0, 0, 0),
        ("x misaligned", i64, 3, 8, EOS, 4, 0, 0, 0),
        ("x misaligned i32", i32, 3, 8, EOS, 2, 0, 0, 0),
        ("pos misaligned", i64, 3, 8, EOS, 0, 4, 0, 0),
        ("doc misaligned", i64, 3, 8, EOS, 0, 0, 4, 0),
        ("doc odd i32", i32, 3, 8, EOS, 0, 0, 1, 0),
        ("cu misaligned", i64, 3, 8, EOS, 0, 0, 0, 2),
        ("eos negative", i64, 3, 8, -1, 0, 0, 0, 0),
        ("eos negative i32", i32, 3, 8, -5, 0, 0, 0, 0),
        ("eos past i32", i32, 3, 8, 2 ** 31, 0, 0, 0, 0),
        ("eos 2^32 + 5 in i32", i32, 3, 8, 2 ** 32 + EOS, 0, 0, 0, 0),
    ]


def run_rejects(fn, D, device, raises, extra=()):
    """Every reject raises ValueError and leaves all four buffers as they
    were.  `extra` entries carry absolute pointers in place of shifts > 4096
    (what, code, rows, T, eos, x, pos, doc, cu)."""
    x = np.full((3, 8), EOS, np.int64)
    for what, code, rows, T, eos, xs, ps, dsh, cs in \
            list(reject_calls(D)) + list(extra):
        xb = Buf(device, 24, 8)
        xb.put(x)
        pb, db, cb = Buf(device, 24, 8), Buf(device, 24, 8), Buf(device, 25, 4)

        def at(buf, shift):
            if shift is None:
                return 0
            return shift if shift > 4096 else buf.ptr + shift
        with raises(ValueError):
            fn(device, at(xb, xs), rows, T, code, eos, at(pb, ps),
               at(db, dsh), at(cb, cs))
            raise AssertionError(f"accepted: {what}")
        xb.expect(x, "x after " + what)
        for b, name in ((pb, "position_ids"), (db, "doc_ids"),
                        (cb, "cu_seqlens")):
            b.expect(np.zeros(0, np.uint8), f"{name} after {what}")


# ------------------------------------------------------------- end to end

DOCS = ("position_ids", "doc_ids", "cu_seqlens")


def check_docs(docs, x_ref, eos, names, torch_dtype, device_type):
    """One batch's docs against the reference applied to the reference x."""
    pos, doc, cu, n_seqs, max_seqlen = reference(x_ref, eos)
    keys = set(names) | ({"max_seqlen"} if "cu_seqlens" in names else set())
    assert set(docs) == keys, (set(docs), keys)
    for name, exp in (("position_ids", pos), ("doc_ids", doc)):
        if name in names:
            t = docs[name]
            assert t.device.type == device_type and t.dtype == torch_dtype
            assert t.shape == x_ref.shape and t.is_contiguous()
            assert np.array_equal(t.cpu().numpy(), exp), name
    if "cu_seqlens" in names:
        t = docs["cu_seqlens"]
        assert t.device.type == device_type and t.dtype == torch.int32
        assert t.shape == (n_seqs + 1,)
        assert np.array_equal(t.cpu().numpy(), cu)
        assert type(docs["max_seqlen"]) is int
        assert docs["max_seqlen"] == max_seqlen


def check_doc_loader(make, X, eos, device_type, batch):
    """make(**kw) builds a loader over the e2e files (drop_last False).
    X: the reference x of every window, in order."""
    assert (X == eos).any(), "the eos id has to occur in the files"
    assert ((X == eos).sum(axis=1) >= 2).any()
    for names in (DOCS, ("doc_ids",), ("cu_seqlens",), ("position_ids",),
                  ("cu_seqlens", "position_ids")):
        ld = make(eos_id=eos, documents=names)
        at = 0
        for out in ld:
            assert len(out) == 3
            x, y, docs = out
            ref = X[at:at + len(x)]
            assert np.array_equal(x.cpu().numpy(), ref)
            check_docs(docs, ref, eos, names, x.dtype, device_type)
            at += len(x)
        assert at == len(X) and len(X) % batch, "the short batch must exist"
    # without documents nothing changes, with or without an eos id
    for kw in ({}, dict(eos_id=eos), dict(documents=())):
        ld = make(**kw)
        outs = list(ld)
        assert outs and all(len(o) == 2 for o in outs)
        assert np.array_equal(
            np.concatenate([o[0].cpu().numpy() for o in outs]), X)


def check_doc_loader_errors(make, raises_invalid):
    """The construction errors."""
    for kw in (dict(eos_id=1, documents=("positions",)),
               dict(eos_id=1, documents=("doc_ids", "mask")),
               dict(documents=("doc_ids",)),
               dict(eos_id=-1, documents=("doc_ids",)),
               dict(eos_id=-1),
               dict(eos_id=100, vocab_size=100, documents=("doc_ids",)),
               dict(eos_id=70000, vocab_size=65536),
               dict(eos_id=1, documents=("cu_seqlens",), seq_len=2 ** 16,
                    batch_size=2 ** 15)):
        with raises_invalid():
            make(**kw)
            raise AssertionError(f"accepted: {kw}")
