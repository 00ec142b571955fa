"""LZ4 through the block path on host memory: Arena.lz4_compress /
lz4_decompress_into on a host arena, BlockReader.read_lz4 /
BlockWriter.write_lz4 on MEM and SSD tiers, the WriteBlockLz4 stream and
the LZ4 replication push between two workers.

The pure-Python decoder (kernel_refs.cvlz_decode_ref) is the oracle for
bytes, and the host decoder (native.lz4_decompress) must agree with it; the
strict checker (lz4_checks.py) enforces the LZ4 end-of-block rules.  The
crafted edge cases of the host compressor are in test_lz4_compress_cases.py.
"""
import asyncio
import os
import struct

import pytest

from curvine_amd import native
from kernel_refs import cvlz_decode_ref
from lz4_checks import (CPU_KINDS, rand_bytes, strict_check, text8,
                        zero_first_match_offset)

SIZES = (0, 1, 12, 13, 65535, 65536, 65537, 2 * 65536 + 13)
OFF = 4099


@pytest.fixture(scope="module")
def host_arena():
    a = native.Arena(-1, 8 << 20)
    yield a
    a.close()


@pytest.mark.parametrize("kind", list(CPU_KINDS))
def test_host_arena_compress(host_arena, kind):
    for n in SIZES:
        data = CPU_KINDS[kind](n)
        if n:
            host_arena.write(OFF, data, 0, n)
        c = host_arena.lz4_compress(OFF, n)
        strict_check(c, n)
        assert cvlz_decode_ref(c) == data, f"{kind} n={n}"
        assert native.lz4_decompress(c) == data, f"{kind} n={n}"


def test_host_arena_compress_range(host_arena):
    with pytest.raises(RuntimeError, match="out of bounds"):
        host_arena.lz4_compress((8 << 20) - 10, 11)


def test_decompress_into(host_arena):
    n = 2 * 65536 + 13
    data = text8(n)
    c = native.lz4_compress(data)
    host_arena.fill(0, 8 << 20, 0xEE)
    assert host_arena.lz4_decompress_into(OFF, c) == n
    assert host_arena.read_bytes(OFF, n) == data
    assert host_arena.read_bytes(OFF + n, 4) == b"\xee" * 4
    # raw_size past the arena end
    with pytest.raises(RuntimeError, match="out of bounds"):
        host_arena.lz4_decompress_into((8 << 20) - n + 1, c)
    # a match offset of 0
    with pytest.raises(RuntimeError, match="corrupt"):
        host_arena.lz4_decompress_into(OFF, zero_first_match_offset(c))
    # truncated: payload, sizes table, header
    for cut in (len(c) - 1, len(c) // 2, 27, 19):
        with pytest.raises(RuntimeError, match="lz4"):
            host_arena.lz4_decompress_into(OFF, c[:cut])
    # a header announcing more raw bytes than its chunks hold
    lie = bytearray(c)
    struct.pack_into("<Q", lie, 4, n + 65536)
    with pytest.raises(RuntimeError, match="lz4"):
        host_arena.lz4_decompress_into(OFF, bytes(lie))


@pytest.mark.parametrize("tier", ["MEM", "SSD"])
def test_block_read_write_lz4(tmp_path, tier):
    from curvine_amd import errors as err
    from curvine_amd.conf import WorkerConf
    from curvine_amd.worker.block_store import BlockStore
    size = "64MB" if tier == "MEM" else "1GB"
    store = BlockStore(WorkerConf(
        data_dirs=[f"[{tier}:{size}]{tmp_path}/{tier.lower()}"]))
    try:
        seg = (1 << 20) + 5
        src = text8(2 * seg, seed=3) + rand_bytes(seg, 36)
        w = store.create_writer(1, 4 << 20, tier)
        for i in range(3):
            c = native.lz4_compress(src[i * seg:(i + 1) * seg])
            assert w.write_lz4(c) == seg
        assert w.pos == 3 * seg
        assert store.finalize(1, w.pos) == tier
        assert store.block_crc(1) == native.crc32c(src)
        r = store.open_reader(1)
        try:
            assert r.read(0, len(src)) == src
            # read_lz4: any window, clamped at the block end
            for off, n in ((0, seg), (seg - 7, 65536 + 20), (3 * seg - 9, 100)):
                c = r.read_lz4(off, n)
                want = src[off:off + n]
                strict_check(c, len(want))
                assert cvlz_decode_ref(c) == want
                assert native.lz4_decompress(c) == want
        finally:
            r.close()
        # a container larger than the reservation: refused, nothing written
        w2 = store.create_writer(2, 1 << 20, tier)
        with pytest.raises(err.InvalidArgument):
            w2.write_lz4(native.lz4_compress(src[:seg]))
        assert w2.pos == 0
        if tier == "SSD":
            w2.meta["_f"].flush()
            assert os.path.getsize(w2.meta["path"]) == 0
        # ... also when only the tail would not fit
        w2.write(b"x" * 10)
        with pytest.raises(err.InvalidArgument):
            w2.write_lz4(native.lz4_compress(bytes((1 << 20) - 9)))
        assert w2.pos == 10
        store.abort(2)
        store.delete(1)
        assert store.block_count() == 0
        assert store.storages()[0].used == 0
    finally:
        store.close()


def test_replication_codec_setting():
    from curvine_amd.conf import ClusterConf, WorkerConf
    assert WorkerConf().replication_codec == ""
    assert ClusterConf.from_dict(
        {"worker": {"replication_codec": "lz4"}}).worker.replication_codec \
        == "lz4"
    with pytest.raises(ValueError, match="replication_codec"):
        ClusterConf.from_dict({"worker": {"replication_codec": "zstd"}})


# ---------------------------------------------------------------------------
# two workers
# ---------------------------------------------------------------------------

MIXED = text8(2 << 20, seed=11) + rand_bytes(1 << 20, 37)


def _run(tmp_path, codec, body):
    from curvine_amd.testing import MiniCluster, test_conf

    async def main():
        conf = test_conf(str(tmp_path))
        conf.worker.replication_codec = codec
        mc = MiniCluster(conf=conf, tmp_dir=str(tmp_path), workers=2)
        await mc.start()
        try:
            await body(mc)
        finally:
            await mc.stop()

    asyncio.new_event_loop().run_until_complete(main())


async def _write_and_replicate(mc):
    fs = mc.fs()
    await fs.write_all("/r.bin", MIXED, storage_tier="MEM", replicas=1)
    await fs.close()
    src = next(w for w in mc.workers if w.store.block_count())
    dst = next(w for w in mc.workers if w is not src)
    bid = next(iter(src.store.blocks))
    await src._replicate({"cmd": "replicate", "block_id": bid, "job_id": 1,
                          "targets": [dst.address().to_dict()],
                          "tier": "MEM"})
    r = dst.store.open_reader(bid)
    try:
        assert r.read(0, len(MIXED)) == MIXED
    finally:
        r.close()
    assert dst.store.blocks[bid].layout.tier == "MEM"
    assert dst.store.block_crc(bid) == src.store.block_crc(bid) \
        == native.crc32c(MIXED)
    return src, dst


def test_replication_lz4(tmp_path, monkeypatch):
    import curvine_amd.worker.server as ws
    assert ws.REPLICATION_LZ4_SEGMENT == 8 << 20
    monkeypatch.setattr(ws, "REPLICATION_LZ4_SEGMENT", 1 << 20)

    async def body(mc):
        src, dst = await _write_and_replicate(mc)
        c = src.counters.snapshot()
        assert c["replication_raw_bytes"] == len(MIXED)
        assert c["replication_wire_bytes"] < c["replication_raw_bytes"]
        assert c["replication_lz4_segments"] >= 1
        assert c["replication_raw_segments"] >= 1
        assert c["replication_lz4_segments"] + \
            c["replication_raw_segments"] == 3
        assert not any(dst.counters.snapshot().values())
        # the counters are on the worker's prometheus and JSON endpoints
        import json
        from curvine_amd.web.server import WebServer
        web = WebServer(src.conf, worker=src, port=0)
        assert json.loads(web._route("/api/worker-counters")[2]) == c
        prom = web._route("/metrics")[2].decode()
        for name, value in c.items():
            assert f"curvine_worker_{name} {value}\n" in prom

    _run(tmp_path, "lz4", body)


def test_replication_default_is_raw(tmp_path):
    async def body(mc):
        src, dst = await _write_and_replicate(mc)
        assert not any(src.counters.snapshot().values())
        assert not any(dst.counters.snapshot().values())

    _run(tmp_path, "", body)


def _assert_empty(worker):
    assert worker.store.block_count() == 0
    assert all(s.used == 0 for s in worker.store.storages())


async def _until_empty(worker):
    # the server aborts on its side of the connection: yield until it has
    for _ in range(500):
        if worker.store.block_count() == 0:
            break
        await asyncio.sleep(0.01)
    _assert_empty(worker)


def test_failed_stream_leaves_nothing(tmp_path):
    from curvine_amd import errors as err
    from curvine_amd.client.block_client import BlockWriterLz4Remote
    good = native.lz4_compress(text8(1 << 20, seed=5))
    raw_crc = native.crc32c(text8(1 << 20, seed=5))

    async def body(mc):
        target = mc.workers[1]
        addr = target.address()

        # a corrupt container mid-stream
        w = BlockWriterLz4Remote(addr, 101, 4 << 20, "MEM")
        await w.write_segment(good, "cvlz")
        with pytest.raises(err.FsError, match="corrupt"):
            await w.write_segment(zero_first_match_offset(good), "cvlz")
            await w.commit(2 << 20, None)
        await w.abort()
        _assert_empty(target)

        # a segment that passes the reservation
        w = BlockWriterLz4Remote(addr, 102, 1 << 20, "MEM")
        with pytest.raises(err.FsError, match="reservation"):
            await w.write_segment(good, "cvlz")
            await w.write_segment(good, "cvlz")
            await w.commit(2 << 20, None)
        await w.abort()
        _assert_empty(target)

        # a Complete whose crc32c is wrong
        w = BlockWriterLz4Remote(addr, 103, 4 << 20, "MEM")
        await w.write_segment(good, "cvlz")
        with pytest.raises(err.ChecksumMismatch):
            await w.commit(1 << 20, raw_crc ^ 1)
        _assert_empty(target)

        # explicit cancel
        w = BlockWriterLz4Remote(addr, 104, 4 << 20, "MEM")
        await w.write_segment(good, "cvlz")
        await w.write_segment(b"tail", "raw")
        await w.abort()
        await _until_empty(target)

        # the connection closes mid-stream
        w = BlockWriterLz4Remote(addr, 105, 4 << 20, "MEM")
        await w.write_segment(good, "cvlz")
        await w.stream.recv()          # the segment is in the block
        assert target.store.block_count() == 1
        await w.stream.client.close()
        await _until_empty(target)

        # and a good stream still commits afterwards
        w = BlockWriterLz4Remote(addr, 106, 4 << 20, "MEM")
        await w.write_segment(good, "cvlz")
        assert await w.commit(1 << 20, raw_crc) == "MEM"
        assert w.last_crc == raw_crc
        assert target.store.block_count() == 1

    _run(tmp_path, "lz4", body)
