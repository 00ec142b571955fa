"""Native ranged pread (reader_pread), the pinned-buffer pool behind
PinnedBuffer and the stream pool behind the per-thread copy streams.

CPU cases run on the MEM tier (host arenas, 1 MiB blocks) and on malloc'd
"pinned" buffers: the same C++ paths as on a GPU, minus the DMA.  GPU cases
are marked `gpu` and use one 16 MiB HBM arena."""
import ctypes
import os
import threading

import pytest

from curvine_amd import native

MIB = 1 << 20
FILE_LEN = 3 * MIB + 777


def _stats():
    return native.hip_pool_stats()


# --------------------------------------------------------------- CPU: reader

@pytest.fixture(scope="module")
def mem_cluster(tmp_path_factory):
    """One MEM-tier cluster for the module: a dense file of 3 MiB + 777
    bytes in 1 MiB blocks, and a file whose length was grown past its only
    block (a tail hole)."""
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.testing import SyncMiniCluster, test_conf

    tmp = str(tmp_path_factory.mktemp("seqread"))
    conf = test_conf(tmp)
    conf.master.block_size = MIB
    conf.client.block_size = MIB
    smc = SyncMiniCluster(conf=conf, tmp_dir=tmp).start()
    try:
        sf = SyncFs(smc.client_conf())
        data = os.urandom(FILE_LEN)
        sf.write_file("/sr/dense", data)
        head = os.urandom(MIB // 2 + 33)
        sf.write_file("/sr/holey", head)
        sf.resize("/sr/holey", 2 * MIB + 5)
        yield sf, data, head
        sf.shutdown()
    finally:
        smc.stop()


def _open_sync(sf, path):
    from curvine_amd.client.reader import SyncLocalReader
    r = SyncLocalReader(sf.call(sf.fs.client.open(path)))
    assert r._native_rid is not None, "registration should engage"
    return r


DENSE_CASES = [
    ("inside a block", 300 * 1024, 64 * 1024),
    ("straddles 1 MiB", MIB - 32 * 1024, 64 * 1024),
    ("straddles two boundaries", MIB - 100, MIB + 200),
    ("clamped tail", FILE_LEN - 1000, 64 * 1024),
    ("off == length", FILE_LEN, 4096),
    ("off > length", FILE_LEN + 12345, 4096),
]


@pytest.mark.parametrize("name,off,n", DENSE_CASES,
                         ids=[c[0] for c in DENSE_CASES])
def test_pread_into_ptr_native(mem_cluster, name, off, n):
    sf, data, _ = mem_cluster
    r = _open_sync(sf, "/sr/dense")
    buf = native.PinnedBuffer(MIB + 4096)
    try:
        buf.view[:] = b"\xa5" * buf.nbytes
        want = data[off:off + n]
        before = _stats()["reader_pread_calls"]
        got = r.pread_into_ptr(off, buf.ptr, n)
        assert _stats()["reader_pread_calls"] == before + 1
        assert got == len(want)
        assert bytes(buf.view[:got]) == want
        # nothing written past the bytes served
        assert bytes(buf.view[got:got + 64]) == b"\xa5" * 64
        # the native call itself served it: no fallback hid a -1
        assert native.load().reader_pread(r._native_rid, off, n,
                                          buf.ptr) == len(want)
    finally:
        r.close()
        buf.close()


def test_pread_into_ptr_hole_falls_back(mem_cluster):
    """A file grown past its block: the native call answers -1 for every
    range that touches the hole and the Python loop fills zeros, exactly as
    pread_into does."""
    sf, _, head = mem_cluster
    r = _open_sync(sf, "/sr/holey")
    length = 2 * MIB + 5
    assert r.length == length
    expect = head + b"\0" * (length - len(head))
    buf = native.PinnedBuffer(MIB)
    try:
        for off, n, native_ok in [
                (100, 4096, True),                     # data only
                (len(head) - 50, 4096, False),         # data then hole
                (MIB + 7, 64 * 1024, False),           # hole only
                (length - 100, 4096, False)]:          # clamped, in the hole
            ref = bytearray(n)
            ref_got = r.pread_into(off, ref, 0, n)
            buf.view[:n] = b"\xa5" * n
            raw = native.load().reader_pread(r._native_rid, off, n, buf.ptr)
            if native_ok:
                assert raw == n
            else:
                assert raw == -1
                # -1 issues nothing
                assert bytes(buf.view[:n]) == b"\xa5" * n
            got = r.pread_into_ptr(off, buf.ptr, n)
            assert got == ref_got == len(expect[off:off + n])
            assert bytes(buf.view[:got]) == bytes(ref[:got]) \
                == expect[off:off + n]
    finally:
        r.close()
        buf.close()


def test_reader_pread_gap_between_extents():
    """Two registered extents with a gap: a range inside either is served,
    one that crosses the gap is refused whole."""
    mod = native.load()
    arena = native.Arena(-1, 64 * 1024)
    buf = native.PinnedBuffer(16 * 1024)
    rid = None
    try:
        a = os.urandom(4096)
        b = os.urandom(4096)
        arena.write(0, a)
        arena.write(8192, b)
        # file [0, 4096) -> arena 0; file [8192, 12288) -> arena 8192
        rid = mod.reader_register([(0, 4096, arena.handle, 0),
                                   (8192, 4096, arena.handle, 8192)], 12288)
        assert mod.reader_pread(rid, 1000, 2000, buf.ptr) == 2000
        assert bytes(buf.view[:2000]) == a[1000:3000]
        assert mod.reader_pread(rid, 8192 + 4000, 4096, buf.ptr) == 96
        assert bytes(buf.view[:96]) == b[4000:]
        buf.view[:] = b"\x5a" * buf.nbytes
        assert mod.reader_pread(rid, 4000, 5000, buf.ptr) == -1
        assert mod.reader_pread(rid, 5000, 100, buf.ptr) == -1
        assert bytes(buf.view[:]) == b"\x5a" * buf.nbytes
    finally:
        if rid is not None:
            mod.reader_unregister(rid)
        buf.close()
        arena.close()


def test_reader_pread_unknown_id_raises():
    buf = native.PinnedBuffer(4096)
    try:
        with pytest.raises(RuntimeError):
            native.load().reader_pread(1 << 40, 0, 4096, buf.ptr)
    finally:
        buf.close()


# ----------------------------------------------------------------- CPU: pool

def test_pool_reuses_same_size():
    mod = native.load()
    a = mod.pinned_alloc(4096)
    ptr = mod.pinned_ptr(a)
    mod.pinned_free(a)
    before = _stats()
    b = mod.pinned_alloc(4096)
    after = _stats()
    try:
        assert after["pinned_reused"] == before["pinned_reused"] + 1
        assert after["pinned_created"] == before["pinned_created"]
        assert mod.pinned_ptr(b) == ptr
    finally:
        mod.pinned_free(b)


def test_pool_other_size_gets_new_buffer():
    mod = native.load()
    a = mod.pinned_alloc(4096)
    ptr = mod.pinned_ptr(a)
    mod.pinned_free(a)
    # 8200: a size nothing else asks for, so it cannot come from the pool
    before = _stats()
    b = mod.pinned_alloc(8200)
    try:
        assert _stats()["pinned_created"] == before["pinned_created"] + 1
        assert mod.pinned_ptr(b) != ptr
        view = mod.pinned_view(b)
        assert view.nbytes == 8200
        pat = bytes(range(256)) * 33
        view[:] = pat[:8200]
        assert ctypes.string_at(mod.pinned_ptr(b), 8200) == pat[:8200]
        del view
    finally:
        mod.pinned_free(b)


def test_pool_count_cap():
    mod = native.load()
    cap = _stats()["pinned_pool_max_count"]
    ids = [mod.pinned_alloc(4096) for _ in range(cap + 8)]
    # older parked buffers leave first, so once `cap` of these are parked
    # the pool holds nothing else and its size stands still
    seen = []
    for i in ids:
        mod.pinned_free(i)
        seen.append(_stats())
    assert seen[cap - 1]["pinned_parked_count"] == cap
    assert seen[cap - 1]["pinned_parked_bytes"] == cap * 4096
    for s in seen[cap:]:
        assert s["pinned_parked_count"] == cap
        assert s["pinned_parked_bytes"] == cap * 4096
    assert seen[-1]["pinned_parked_bytes"] <= seen[-1]["pinned_pool_max_bytes"]


def test_pool_skips_oversized_buffer():
    mod = native.load()
    big = _stats()["pinned_pool_max_buffer"] + 4096
    a = mod.pinned_alloc(big)
    before = _stats()
    mod.pinned_free(a)
    after = _stats()
    assert after["pinned_parked_bytes"] == before["pinned_parked_bytes"]
    assert after["pinned_parked_count"] == before["pinned_parked_count"]
    b = mod.pinned_alloc(big)
    try:
        assert _stats()["pinned_reused"] == after["pinned_reused"]
    finally:
        mod.pinned_free(b)


def test_freed_id_is_invalid():
    mod = native.load()
    a = mod.pinned_alloc(4096)
    mod.pinned_free(a)
    with pytest.raises(RuntimeError):
        mod.pinned_ptr(a)
    with pytest.raises(RuntimeError):
        mod.pinned_view(a)
    mod.pinned_free(a)      # a second free stays a no-op
    b = mod.pinned_alloc(4096)
    assert mod.pinned_ptr(b)
    mod.pinned_free(b)


# ----------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def hbm_reader():
    """16 MiB HBM arena holding a "file" of two 1 MiB extents plus a 4 KiB
    tail, registered as a native reader; the extents sit apart in the arena
    so a straddling read cannot pass by reading on linearly."""
    mod = native.load()
    arena = native.Arena(0, 16 * MIB)
    data = os.urandom(2 * MIB + 4096)
    slots = [(0, MIB, 5 * MIB), (MIB, MIB, 2 * MIB), (2 * MIB, 4096, 9 * MIB)]
    for foff, ln, aoff in slots:
        arena.write(aoff, data[foff:foff + ln])
    rid = mod.reader_register(
        [(foff, ln, arena.handle, aoff) for foff, ln, aoff in slots],
        len(data))
    yield mod, rid, data
    mod.reader_unregister(rid)
    arena.close()


@pytest.mark.gpu
def test_gpu_reader_pread_straddle_and_tail(hbm_reader):
    mod, rid, data = hbm_reader
    buf = native.PinnedBuffer(MIB + 4096)
    try:
        for off, n in [(300 * 1024, 64 * 1024),
                       (MIB - 32 * 1024, 64 * 1024),
                       (MIB - 100, MIB + 200),
                       (2 * MIB - 1000, 64 * 1024),       # into the tail, clamped
                       (len(data), 4096),
                       (len(data) + 1, 4096)]:
            want = data[off:off + n]
            buf.view[:] = b"\xa5" * buf.nbytes
            assert mod.reader_pread(rid, off, n, buf.ptr) == len(want)
            assert bytes(buf.view[:len(want)]) == want, (off, n)
            assert bytes(buf.view[len(want):len(want) + 64]) == b"\xa5" * 64
    finally:
        buf.close()


@pytest.mark.gpu
def test_gpu_short_threads_share_streams(hbm_reader):
    mod, rid, data = hbm_reader
    before = _stats()["streams_created"]
    bad = []

    def one(k):
        buf = native.PinnedBuffer(4096)
        try:
            off = k * 200_000 + 17
            got = mod.reader_pread(rid, off, 4096, buf.ptr)
            if got != 4096 or bytes(buf.view[:4096]) != data[off:off + 4096]:
                bad.append(k)
        except Exception as e:  # noqa: BLE001
            bad.append((k, e))
        finally:
            buf.close()

    for _ in range(3):
        ths = [threading.Thread(target=one, args=(k,)) for k in range(8)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    assert not bad
    assert _stats()["streams_created"] - before <= 8


@pytest.mark.gpu
def test_gpu_pinned_buffer_reused_across_threads(hbm_reader):
    mod, rid, data = hbm_reader
    before = _stats()["pinned_created"]
    bad = []

    def one(k):
        buf = native.PinnedBuffer(64 * 1024)
        try:
            off = MIB - 1000 + k * 4096      # every read straddles 1 MiB
            got = mod.reader_pread(rid, off, 64 * 1024, buf.ptr)
            if got != 64 * 1024 or \
                    bytes(buf.view[:got]) != data[off:off + got]:
                bad.append(k)
        except Exception as e:  # noqa: BLE001
            bad.append((k, e))
        finally:
            buf.close()

    # two threads in turn, three rounds: at most one buffer is out at a time
    for k in range(6):
        t = threading.Thread(target=one, args=(k,), name=f"turn-{k % 2}")
        t.start()
        t.join()
    assert not bad
    assert _stats()["pinned_created"] - before <= 2
