"""Packed token batches on the MI355X: the eos-index kernels and
token_pack_kernel on a device arena over the case matrix of
token_pack_cases, the argument errors (buffers untouched afterwards), and
CurvinePackedTokenLoader over HBM-tier files and over MEM-tier files with
cuda destinations.  Comparisons are exact."""
import numpy as np
import pytest
import torch

from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.client.reader import SyncLocalReader
from curvine_amd.sdk import CurvinePackedTokenLoader
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

import token_doc_cases as dc
import token_pack_cases as pc

pytestmark = pytest.mark.gpu

D = native.DTYPES
DEV = 0
MiB = 1 << 20
CAP = 4 * MiB
BLOCK = 64


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(DEV, CAP)
    yield a
    a.close()


@pytest.fixture(scope="module")
def host_arena():
    a = native.Arena(-1, 1 * MiB)
    yield a
    a.close()


def eos_tile():
    return native.load().TOKEN_EOS_TILE


def pack_tile():
    return native.load().TOKEN_PACK_TILE


# ---------------------------------------------------------------- eos index

@pytest.mark.parametrize("src", pc.SOURCES)
def test_eos_sizes(arena, src):
    pc.case_eos_sizes(arena, D, DEV, src, eos_tile())


@pytest.mark.parametrize("src", pc.SOURCES)
def test_eos_phases(arena, src):
    pc.case_eos_phases(arena, D, DEV, src, eos_tile())


@pytest.mark.parametrize("src", pc.SOURCES)
def test_eos_edges(arena, src):
    pc.case_eos_edges(arena, D, DEV, src, eos_tile())


def test_eos_long(arena):
    pc.case_eos_long(arena, D, DEV, eos_tile())


def test_eos_full_width(arena):
    pc.case_eos_full_width(arena, D, DEV)


def host_pointer():
    host = torch.full((4096 + 1024,), dc.SENTINEL, dtype=torch.uint8)
    return host, (host.data_ptr() + 4096 + 15) // 16 * 16


def test_eos_rejects(arena, host_arena):
    host, hp = host_pointer()
    extra = [("out on the host", [(0, 0, 4)], D["U16"], pc.EOS, hp, 4)]
    pc.run_eos_rejects(arena, D, DEV, CAP, pytest.raises, extra)
    assert bool((host == dc.SENTINEL).all())
    # and a device pointer with a host arena
    out = pc.Buf(DEV, 8, 8)
    host_arena.write(0, np.full(8, pc.EOS, np.uint16).tobytes())
    with pytest.raises(ValueError):
        host_arena.token_eos_index([(0, 0, 4)], D["U16"], pc.EOS, out.ptr, 4)
    out.expect(np.zeros(0, np.int64), "device out on a host arena")


# -------------------------------------------------------------- pack kernel

@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_sizes(arena, src, dst):
    pc.case_pack_sizes(arena, D, DEV, src, dst, pack_tile())


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_phases(arena, src, dst):
    pc.case_pack_phases(arena, D, DEV, src, dst)


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_cuts(arena, src, dst):
    pc.case_pack_cuts(arena, D, DEV, src, dst, pack_tile())


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_outputs(arena, src, dst):
    pc.case_pack_outputs(arena, D, DEV, src, dst, pack_tile())


@pytest.mark.parametrize("src,dst", pc.PAIRS)
def test_pack_vocab(arena, src, dst):
    pc.case_pack_vocab(arena, D, DEV, src, dst, pack_tile())


def test_pack_rejects(arena, host_arena):
    host, hp = host_pointer()
    extra = [(f"{name} on the host", {name: hp})
             for name in ("x", "y", "pos", "doc", "cu")]
    pc.run_pack_rejects(arena, D, DEV, CAP, pytest.raises, extra)
    assert bool((host == dc.SENTINEL).all())
    # and each pointer on the device with a host arena
    host_arena.write(0, np.arange(64, dtype=np.uint16).tobytes())
    names = ("x", "y", "pos", "doc", "cu")
    for k in names:
        bufs = {n: pc.Buf(DEV if n == k else -1, 3 if n == "cu" else 24,
                          4 if n == "cu" else 8) for n in names}
        with pytest.raises(ValueError):
            host_arena.token_pack(
                [(0, 0, 4, 0, 0, 0, pc.NEXT), (0, 4, 4, 0, 0, 1, pc.PAD)],
                [(0, 0, 0, 5)], *(bufs[n].ptr for n in names), 3, 8,
                D["U16"], D["I64"], 0, -100, 0)
        for n, b in bufs.items():
            b.expect(np.zeros(0, np.uint8), f"{n} with {k} on the device")


# -------------------------------------------------------------- end to end

def test_end_to_end_hbm_and_mem(tmp_path, monkeypatch):
    docs = pc.e2e_docs()
    all_docs = [d for f in docs for d in f]
    T, B, ign = pc.E2E["T"], pc.E2E["batch"], pc.E2E["ignore"]
    conf = make_conf(str(tmp_path))
    smc = SyncMiniCluster(conf=conf, tmp_dir=str(tmp_path),
                          worker_dirs=[["[HBM:512MB:0]gpu0",
                                        "[MEM:64MB]mem0"]]).start()
    made = []
    sf = None
    try:
        sf = SyncFs(smc.client_conf())
        hbm, mem = [], []
        for i, blob in enumerate(pc.e2e_files(docs)):
            hbm.append(f"/packed/hbm{i}.bin")
            sf.write_file(hbm[-1], blob, storage_tier="HBM", block_size=BLOCK)
            mem.append(f"/packed/mem{i}.bin")
            sf.write_file(mem[-1], blob, storage_tier="MEM", block_size=BLOCK)

        calls, scans, index_calls = [], [], []
        orig = native.Arena.token_pack
        orig_index = native.Arena.token_eos_index

        def spy(self, segments, pieces, *a, **kw):
            calls.append(self.device)
            return orig(self, segments, pieces, *a, **kw)

        def spy_index(self, *a, **kw):
            index_calls.append(self.device)
            return orig_index(self, *a, **kw)

        def spy_docs(*a, **kw):
            scans.append(a)
            raise AssertionError("the packed loader scans nothing per batch")
        monkeypatch.setattr(native.Arena, "token_pack", spy)
        monkeypatch.setattr(native.Arena, "token_eos_index", spy_index)
        monkeypatch.setattr(native, "token_docs", spy_docs)

        def make(paths, **kw):
            args = dict(seq_len=T, batch_size=B, eos_id=pc.E2E["eos"],
                        device="cuda:0", src_dtype=pc.E2E["src"],
                        header_bytes=pc.E2E["header"])
            args.update(kw)
            ld = CurvinePackedTokenLoader(smc.client_conf(), paths, **args)
            made.append(ld)
            return ld

        def epoch(ld, dtype=torch.int64):
            got, n = [], 0
            for x, y, dd in ld:
                for t in (x, y, dd["position_ids"], dd["doc_ids"]):
                    assert t.shape == (B, T) and t.dtype == dtype
                    assert t.device.type == "cuda" and t.is_contiguous()
                assert dd["cu_seqlens"].device.type == "cuda"
                got += pc.batch_chunks(x, y, dd, T, B, ld.pad_id, ign)
                n += 1
            assert n == len(ld) and n > 1
            assert sorted(got) == pc.doc_chunks(all_docs, T, ign)
            return n

        # HBM tier: the index kernels, then one pack launch per batch
        ld = make(hbm)
        assert index_calls and all(d == DEV for d in index_calls)
        assert ld.num_documents == len(all_docs)
        n = epoch(ld)
        assert calls == [DEV] * n and not scans
        ld = make(hbm, out_dtype=torch.int32, pad_id=77)
        epoch(ld, torch.int32)

        # MEM tier with cuda destinations: everything goes the slow way
        del calls[:], index_calls[:]
        ld = make(mem)
        assert not index_calls and ld.num_documents == len(all_docs)
        epoch(ld)
        assert not calls and not scans

        # the reader's index on both tiers
        for paths in (hbm, mem):
            for f, path in zip(docs, paths):
                r = SyncLocalReader(sf.call(sf.fs.client.open(path)))
                try:
                    got = r.token_eos_index("U16", pc.E2E["header"],
                                            pc.E2E["eos"], True)
                finally:
                    r.close()
                assert got.tolist() == np.flatnonzero(
                    np.concatenate(f) == pc.E2E["eos"]).tolist()
    finally:
        for ld in made:
            ld.close()
        if sf is not None:
            sf.shutdown()
        smc.stop()
