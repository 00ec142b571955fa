"""Packed token batches without a GPU: the host twins of the eos-index and
pack kernels on a host arena, the argument errors, pack_segments, and
CurvinePackedTokenLoader over MEM-tier files with device="cpu".  Expected
values come from token_pack_cases (numpy only); comparisons are exact."""
import array

import numpy as np
import pytest
import torch

from curvine_amd import errors as err
from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.client.reader import SyncLocalReader
from curvine_amd.sdk import CurvinePackedTokenLoader, pack_segments
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

import token_pack_cases as pc
import token_window_cases as tc

D = native.DTYPES
MiB = 1 << 20
CAP = 4 * MiB
BLOCK = 64


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(-1, CAP)
    yield a
    a.close()


def eos_tile():
    return native.load().TOKEN_EOS_TILE


def pack_tile():
    return native.load().TOKEN_PACK_TILE


def test_constants():
    n = native.load()
    assert eos_tile() >= 64 and pack_tile() >= 64
    assert (n.TOKEN_SEG_NEXT, n.TOKEN_SEG_PAD) == (pc.NEXT, pc.PAD)
    assert (native.TOKEN_SEG_NEXT, native.TOKEN_SEG_PAD) == (pc.NEXT, pc.PAD)


# ---------------------------------------------------------------- eos index

@pytest.mark.parametrize("src", pc.SOURCES)
def test_eos_sizes(arena, src):
    pc.case_eos_sizes(arena, D, -1, src, eos_tile())


@pytest.mark.parametrize("src", pc.SOURCES)
def test_eos_phases(arena, src):
    pc.case_eos_phases(arena, D, -1, src, eos_tile())


@pytest.mark.parametrize("src", pc.SOURCES)
def test_eos_edges(arena, src):
    pc.case_eos_edges(arena, D, -1, src, eos_tile())


def test_eos_long(arena):
    pc.case_eos_long(arena, D, -1, eos_tile())


def test_eos_full_width(arena):
    pc.case_eos_full_width(arena, D, -1)


def test_eos_rejects(arena):
    pc.run_eos_rejects(arena, D, -1, CAP, pytest.raises)


@pytest.mark.parametrize("src", pc.SOURCES)
def test_eos_index_host(src):
    rng = np.random.default_rng(5)
    t = pc.eos_tokens(rng, src, 41)
    t[[0, 7, 8, 40]] = pc.EOS
    for shift in (0, 1):                    # an odd source address too
        raw = bytearray(shift) + bytearray(t.tobytes())
        out = native.token_eos_index_host(memoryview(raw)[shift:], D[src],
                                          pc.EOS, 100, len(t))
        assert np.frombuffer(out, np.int64).tolist() == [100, 107, 108, 140]
    assert native.token_eos_index_host(b"", D[src], pc.EOS, 0, 0) == b""
    with pytest.raises(ValueError):
        native.token_eos_index_host(t.tobytes(), D[src], pc.EOS, 0, len(t) + 1)
    with pytest.raises(ValueError):
        native.token_eos_index_host(t.tobytes(), D[src], -1, 0, 1)


# -------------------------------------------------------------- pack kernel

@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_sizes(arena, src, dst):
    pc.case_pack_sizes(arena, D, -1, src, dst, pack_tile())


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_phases(arena, src, dst):
    pc.case_pack_phases(arena, D, -1, src, dst)


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_cuts(arena, src, dst):
    pc.case_pack_cuts(arena, D, -1, src, dst, pack_tile())


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_outputs(arena, src, dst):
    pc.case_pack_outputs(arena, D, -1, src, dst, pack_tile())


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_vocab(arena, src, dst):
    pc.case_pack_vocab(arena, D, -1, src, dst, pack_tile())


def test_pack_rejects(arena):
    pc.run_pack_rejects(arena, D, -1, CAP, pytest.raises)


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_piece_host(src, dst):
    """The slow path's routine against the same definitions: every piece
    [a, b) of a segment, with and without has_next, and a pad segment."""
    rng = np.random.default_rng(7)
    dt = tc.NP_DST[dst]
    n, pos0, doc, ign = 6, 40, 3, -100
    for has_next in (False, True):
        d = tc.make_tokens(rng, src, n + int(has_next))
        wide = tc.ref_widen(d, dst)
        flags = pc.NEXT if has_next else 0
        for a in range(len(d)):
            for b in range(a + 1, len(d) + 1):
                raw = bytearray(1) + bytearray(d[a:b].tobytes())
                x, y, pos, dc_, bad = native.token_pack_piece_host(
                    memoryview(raw)[1:], n, pos0, doc, flags, a, b - a,
                    D[src], D[dst], 0, ign, tc.VOCAB)
                nx = max(0, min(b, n) - a)
                ey = wide[max(a, 1):b].tolist()
                if not has_next and b == n:
                    ey.append(ign)
                assert np.frombuffer(x, dt).tolist() == wide[a:a + nx].tolist()
                assert np.frombuffer(y, dt).tolist() == ey
                assert np.frombuffer(pos, dt).tolist() == \
                    list(range(pos0 + a, pos0 + a + nx))
                assert np.frombuffer(dc_, dt).tolist() == [doc] * nx
                assert bad == tc.ref_count(d[a:b], src, tc.VOCAB)
    x, y, pos, dc_, bad = native.token_pack_piece_host(
        b"", 5, 0, 0, pc.PAD, 0, 5, D[src], D[dst], 9, ign, 0)
    assert np.frombuffer(x, dt).tolist() == [9] * 5
    assert np.frombuffer(y, dt).tolist() == [ign] * 5
    assert np.frombuffer(pos, dt).tolist() == list(range(5))
    assert np.frombuffer(dc_, dt).tolist() == [-1] * 5 and bad == 0
    for bad_call in ((b"\0" * 4, 4, 0, 0, 0, 0, 5),      # past n
                     (b"\0" * 4, 4, 0, 0, 0, 0, 0),      # k 0
                     (b"\0" * 2, 4, 0, 0, 0, 0, 4),      # short source
                     (b"", 4, 0, 0, pc.PAD, 1, 3)):      # a pad in part
        with pytest.raises(ValueError):
            native.token_pack_piece_host(*bad_call, D[src], D[dst], 0, ign, 0)


# ---------------------------------------------------------- packing function

def check_packing(lengths, T, B):
    """The properties of pack_segments, and its first-fit order by a
    straight re-run of the rule."""
    batches = pack_segments(lengths, T, B)
    seen = {d: np.zeros(L, np.int32) for d, L in enumerate(lengths)}
    expect = []                   # the segments in order: (d, t0, n, next)
    for d, L in enumerate(lengths):
        for t0 in range(0, L, T):
            expect.append((d, t0, min(T, L - t0), t0 + T < L))
    at = 0
    for segments, sources in batches:
        assert len(segments) == len(sources)
        cover = np.zeros((B, T), np.int32)
        free = [T] * B            # first-fit replay of this batch
        docs = [0] * B
        placed = {}
        while at < len(expect):
            d, t0, n, nxt = expect[at]
            row = next((r for r in range(B) if free[r] >= n), None)
            if row is None:
                break
            placed[(d, t0)] = (row, T - free[row], n, t0, docs[row],
                               pc.NEXT if nxt else 0)
            free[row] -= n
            docs[row] += 1
            at += 1
        assert placed, "a batch holds at least one segment"
        order = sorted(range(len(segments)),
                       key=lambda i: (segments[i][0], segments[i][1]))
        assert order == list(range(len(segments))), "row-major order"
        n_src = 0
        for i, (seg, src) in enumerate(zip(segments, sources)):
            row, col, n, pos0, doc, seq, flags = seg
            assert n >= 1 and row < B and col + n <= T and seq == i
            cover[row, col:col + n] += 1
            if src is None:
                assert flags == pc.PAD and col + n == T
                assert col == T - free[row]
                continue
            n_src += 1
            assert placed[src] == (row, col, n, pos0, doc, flags), (src, seg)
            seen[src[0]][src[1]:src[1] + n] += 1
        assert n_src == len(placed)
        assert (cover == 1).all(), "rows never overlap and are full"
        cu = [s[0] * T + s[1] for s in segments] + [B * T]
        assert all(a < b for a, b in zip(cu, cu[1:]))
    assert at == len(expect)
    for d, L in enumerate(lengths):
        assert (seen[d] == 1).all(), "every token lands exactly once"
    return batches


def test_pack_segments():
    T, B = 8, 3
    for lengths in ([1], [T - 1], [T], [T + 1], [2 * T], [2 * T + 1],
                    [1] * (B * T + 1), [T] * B, [T] * (B + 1),
                    [T - 1, 2, 1, 2 * T + 1, 3, T, T + 1, 1, 1, 5, 2 * T, 7],
                    [5, 5, 5, 3, 3, 3, 1, 1, 1, 1], []):
        batches = check_packing(lengths, T, B)
        assert bool(batches) == bool(lengths)
    rng = np.random.default_rng(11)
    for T, B in ((5, 1), (7, 4), (16, 2)):
        check_packing(rng.integers(1, 3 * T, 60).tolist(), T, B)
    # the tail of a long document goes back into the first row with room
    segments, sources = pack_segments([3, 2 * 8 + 1], 8, 3)[0]
    assert [(s[0], s[1], s[2], s[3], s[6]) for s in segments] == [
        (0, 0, 3, 0, 0), (0, 3, 1, 16, 0), (0, 4, 4, 0, pc.PAD),
        (1, 0, 8, 0, pc.NEXT), (2, 0, 8, 8, pc.NEXT)]
    assert sources == [(0, 0), (1, 16), None, (1, 0), (1, 8)]
    with pytest.raises(ValueError):
        pack_segments([3], 0, 2)


# -------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def cluster(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("packed"))
    smc = SyncMiniCluster(conf=make_conf(tmp), tmp_dir=tmp).start()
    sf = SyncFs(smc.client_conf())
    docs = pc.e2e_docs()
    paths = []
    for i, blob in enumerate(pc.e2e_files(docs)):
        paths.append(f"/packed/f{i}.bin")
        sf.write_file(paths[-1], blob, storage_tier="MEM", block_size=BLOCK)
    sf.write_file("/packed/five.bin", b"12345", storage_tier="MEM")
    yield smc, docs, paths
    sf.shutdown()
    smc.stop()


def make_loader(smc, paths, made, **kw):
    args = dict(seq_len=pc.E2E["T"], batch_size=pc.E2E["batch"],
                eos_id=pc.E2E["eos"], device="cpu", src_dtype=pc.E2E["src"],
                header_bytes=pc.E2E["header"])
    args.update(kw)
    ld = CurvinePackedTokenLoader(smc.client_conf(), paths, **args)
    made.append(ld)
    return ld


def check_epoch(ld, all_docs, device_type="cpu", dtype=torch.int64):
    """One epoch with world 1: every document exactly once, masked
    targets, continued positions, cu_seqlens and max_seqlen."""
    T, B, ign = ld.seq_len, ld.batch_size, ld.ignore_index
    got, n = [], 0
    for x, y, docs in ld:
        assert set(docs) == {"position_ids", "doc_ids", "cu_seqlens",
                             "max_seqlen"}
        for t in (x, y, docs["position_ids"], docs["doc_ids"]):
            assert t.shape == (B, T) and t.dtype == dtype
            assert t.device.type == device_type and t.is_contiguous()
        assert docs["cu_seqlens"].dtype == torch.int32
        assert type(docs["max_seqlen"]) is int
        got += pc.batch_chunks(x, y, docs, T, B, ld.pad_id, ign)
        n += 1
    assert n == len(ld) and n > 1
    assert sorted(got) == pc.doc_chunks(all_docs, T, ign)
    real = sum(len(c[1]) for c in got)
    assert ld.pack_efficiency == real / (n * B * T)


def test_end_to_end_mem(cluster, monkeypatch):
    smc, docs, paths = cluster
    all_docs = [d for f in docs for d in f]
    calls, slows, scans = [], [], []
    orig = native.Arena.token_pack
    orig_exec = SyncLocalReader.exec_token_pack

    def spy(self, segments, pieces, *a, **kw):
        calls.append((self.device, list(pieces)))
        return orig(self, segments, pieces, *a, **kw)

    def spy_exec(self, groups, slow, *a, **kw):
        slows.append(list(slow))
        return orig_exec(self, groups, slow, *a, **kw)

    def spy_docs(*a, **kw):
        scans.append(a)
        raise AssertionError("the packed loader scans nothing per batch")
    monkeypatch.setattr(native.Arena, "token_pack", spy)
    monkeypatch.setattr(SyncLocalReader, "exec_token_pack", spy_exec)
    monkeypatch.setattr(native, "token_docs", spy_docs)
    made = []
    try:
        ld = make_loader(smc, paths, made)
        assert ld.num_documents == len(all_docs)
        check_epoch(ld, all_docs)
        # one host-arena call per batch (the worker has one MEM arena); the
        # tokens cut by a block boundary went the slow way, one at a time
        assert len(calls) == len(ld) and all(d == -1 for d, _ in calls)
        assert any(p[2] > 0 for _, ps in calls for p in ps)
        assert any(s for s in slows)
        assert all(k == 1 for s in slows for _o, _s, _j, k in s)
        assert not scans
        del calls[:]
        check_epoch(ld, all_docs)           # the plans are replayed
        assert len(calls) == len(ld)

        ld = make_loader(smc, paths, made, out_dtype=torch.int32, pad_id=77,
                         ignore_index=-1)
        check_epoch(ld, all_docs, dtype=torch.int32)
        ld = make_loader(smc, paths, made, outputs=("doc_ids",))
        x, y, docs_ = next(iter(ld))
        assert set(docs_) == {"doc_ids"}
        ld = make_loader(smc, paths, made, outputs=())
        assert all(d == {} for _x, _y, d in ld)

        # a vocabulary the files do not fit raises instead of yielding
        ld = make_loader(smc, paths, made, vocab_size=1000)
        with pytest.raises(err.InvalidArgument):
            list(ld)
        ld = make_loader(smc, paths, made, vocab_size=65536)
        check_epoch(ld, all_docs)
    finally:
        for ld in made:
            ld.close()


def rank_docs(ld):
    """The documents (as tuples) a rank yields in one epoch, chunks joined
    in position order."""
    chunks = []
    for x, y, docs in ld:
        chunks += pc.batch_chunks(x, y, docs, ld.seq_len, ld.batch_size,
                                  ld.pad_id, ld.ignore_index)
    return chunks


def test_world_and_shuffle(cluster):
    smc, docs, paths = cluster
    all_docs = [d for f in docs for d in f]
    T, ign = pc.E2E["T"], pc.E2E["ignore"]
    made = []
    try:
        r0 = make_loader(smc, paths, made, rank=0, world=2)
        r1 = make_loader(smc, paths, made, rank=1, world=2)
        assert len(r0) == len(r1) > 0
        keep = len(all_docs) - len(all_docs) % 2
        exp0 = pc.doc_chunks(all_docs[0:keep:2], T, ign)
        exp1 = pc.doc_chunks(all_docs[1:keep:2], T, ign)
        got0, got1 = rank_docs(r0), rank_docs(r1)
        # a rank with more batches than the common length drops its last
        # ones: what it yields is a part of its own documents' chunks
        for got, exp in ((got0, exp0), (got1, exp1)):
            left = list(exp)
            for c in got:
                left.remove(c)                  # ValueError: not its own
            assert len(got) > 0
        # the one-token documents (an eos alone) look alike; all others are
        # random and tell the ranks apart
        lone = (pc.E2E["eos"],)
        assert not {c for c in got0 if c[1] != lone} & set(got1), \
            "the ranks' documents are disjoint"

        a = make_loader(smc, paths, made, shuffle=True, seed=3)
        b = make_loader(smc, paths, made, shuffle=True, seed=3)
        ea, eb = rank_docs(a), rank_docs(b)
        assert ea == eb, "deterministic per (seed, epoch)"
        assert sorted(ea) == pc.doc_chunks(all_docs, T, ign)
        a.set_epoch(1)
        e1 = rank_docs(a)
        assert sorted(e1) == sorted(ea) and e1 != ea
        b.set_epoch(1)
        assert rank_docs(b) == e1
    finally:
        for ld in made:
            ld.close()


def test_loader_argument_errors(cluster):
    smc, _docs, paths = cluster
    made = []
    try:
        for kw in (dict(seq_len=0), dict(seq_len=-1), dict(batch_size=0),
                   dict(rank=2, world=2), dict(rank=-1), dict(world=0),
                   dict(header_bytes=-1), dict(vocab_size=-1),
                   dict(eos_id=-1), dict(eos_id=None), dict(eos_id=2 ** 16),
                   dict(eos_id=100, vocab_size=100),
                   dict(outputs=("positions",)),
                   dict(pad_id=2 ** 31, out_dtype=torch.int32),
                   dict(ignore_index=-2 ** 31 - 1, out_dtype=torch.int32),
                   dict(seq_len=2 ** 16, batch_size=2 ** 15),
                   dict(header_bytes=2)):          # an odd number of bytes
            with pytest.raises(err.InvalidArgument):
                make_loader(smc, paths, made, **kw)
        with pytest.raises(err.InvalidArgument):
            make_loader(smc, ["/packed/five.bin"], made, header_bytes=7)
        for kw in (dict(src_dtype="U32", out_dtype=torch.int32),
                   dict(src_dtype="U8"), dict(out_dtype=torch.int16)):
            with pytest.raises(err.Unsupported):
                make_loader(smc, paths, made, **kw)
    finally:
        for ld in made:
            ld.close()


def test_reader_eos_index(cluster):
    """SyncLocalReader.token_eos_index over a MEM-tier file cut into
    64-byte blocks at an odd header: arena spans on the host side, the
    straddling tokens through pread, merged in order; and all of it through
    pread when the destinations are on the other side."""
    smc, docs, paths = cluster
    sf = SyncFs(smc.client_conf())
    try:
        for f, path in zip(docs, paths):
            toks = np.concatenate(f)
            exp = np.flatnonzero(toks == pc.E2E["eos"]).tolist()
            r = SyncLocalReader(sf.call(sf.fs.client.open(path)))
            try:
                for on_dev in (False, True):
                    got = r.token_eos_index("U16", pc.E2E["header"],
                                            pc.E2E["eos"], on_dev)
                    assert isinstance(got, array.array) and got.typecode == "q"
                    assert got.tolist() == exp
                assert r.token_eos_index("U16", pc.E2E["header"], 1,
                                         False).tolist() == []
            finally:
                r.close()
    finally:
        sf.shutdown()
