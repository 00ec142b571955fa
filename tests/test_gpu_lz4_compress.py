"""GPU tests (MI355X) for the device LZ4 compressor and the LZ4 replication
push between HBM tiers.

The pure-Python decoder (kernel_refs.cvlz_decode_ref) is the oracle for
bytes, and the host decoder (native.lz4_decompress) must agree with it; the
strict checker in lz4_checks.py enforces the LZ4 end-of-block rules on what
the kernel emits.  The crafted edge cases are in
test_gpu_lz4_compress_edges.py.
"""
import asyncio

import pytest

from curvine_amd import native
from kernel_refs import cvlz_decode_ref
from lz4_checks import (CHUNK, pattern, rand_bytes, strict_check, text8,
                        worst_case)

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 12, 13, 64, 65535, 65536, 65537, 2 * 65536 + 13, (1 << 20) + 5)
OFFSETS = (4099, 65536)

# device container may exceed the host compressor's by this fraction on the
# text and pattern123 cases: twice the worst excess observed on an MI355X,
# 1.000134 for text8 at 1 MiB + 5 (profiles/lz4_device_compress.json,
# "size_vs_host"); the kernel is deterministic and the data seeded
SIZE_MARGIN = 0.00027


def _period1_then_random(n):
    tail = min(n, 1000)
    return b"\xa5" * (n - tail) + rand_bytes(tail, 31)


def _repeat_32k(n):
    half = rand_bytes(32768, 32)
    return (half * (n // 32768 + 1))[:n]


def _far_offset(n):
    """Random bytes whose first 20 bytes recur at 65500: with 64 KiB chunks
    and the rule that no match starts in a chunk's last 12 bytes, 65523 is
    the largest offset a block can hold, so this sits next to the format's
    limit.  The same bytes recur at 65535 as well, straddling the chunk
    boundary, where no match may be made."""
    b = bytearray(rand_bytes(n, 33))
    for c in range(0, n, CHUNK):
        if c + 65520 <= n:
            b[c + 65500:c + 65520] = b[c:c + 20]
        if c + 65551 <= n:
            b[c + 65535:c + 65551] = b[c:c + 16]
    return bytes(b)


KINDS = {
    "zeros": lambda n: bytes(n),
    "urandom": lambda n: rand_bytes(n, 34),
    "text8": text8,
    "pattern123": pattern,
    "period1_then_random": _period1_then_random,
    "repeat_32k": _repeat_32k,
    "far_offset": _far_offset,
}

_data_cache = {}


def _data(kind, n):
    key = (kind, n)
    if key not in _data_cache:
        _data_cache[key] = KINDS[kind](n)
    return _data_cache[key]


@pytest.fixture(scope="module")
def arena():
    assert native.gpu_available(), "GPU required: _native must see a device"
    a = native.Arena(0, 64 << 20, staging_bytes=4 << 20, staging_count=4)
    yield a
    a.close()


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_compress_matrix(arena, kind, off):
    for n in SIZES:
        data = _data(kind, n)
        if n:
            arena.write(off, data, 0, n)
        c = arena.lz4_compress(off, n)
        strict_check(c, n)
        assert cvlz_decode_ref(c) == data, f"{kind} n={n} off={off}"
        assert native.lz4_decompress(c) == data, f"{kind} n={n} off={off}"
        assert len(c) <= worst_case(n), f"{kind} n={n}: {len(c)}"


def test_deterministic(arena):
    n = 1 << 20
    data = _data("text8", n)
    arena.write(4099, data, 0, n)
    first = arena.lz4_compress(4099, n)
    assert arena.lz4_compress(4099, n) == first
    assert arena.lz4_compress(4099, n) == first


def test_size_bounds(arena):
    n = 1 << 20
    arena.write(4099, _data("zeros", n), 0, n)
    c = arena.lz4_compress(4099, n)
    assert len(c) <= 20 + 4 * 16 + 16 * 1024, len(c)
    arena.write(4099, _data("urandom", n), 0, n)
    assert len(arena.lz4_compress(4099, n)) <= worst_case(n)
    for kind in ("text8", "pattern123"):
        for m in ((1 << 20) + 5, 2 * 65536 + 13, 65536):
            data = _data(kind, m)
            arena.write(4099, data, 0, m)
            dev = len(arena.lz4_compress(4099, m))
            host = len(native.lz4_compress(data))
            print(f"size_vs_host {kind} n={m}: device {dev} host {host} "
                  f"ratio {dev / host:.4f}")
            assert dev <= host * (1 + SIZE_MARGIN), (kind, m, dev, host)


def test_device_round_trip(arena):
    """compress from one extent, decompress into another: raw bytes never
    visit the host."""
    n = (1 << 20) + 5
    data = _data("text8", n)
    arena.write(4099, data, 0, n)
    c = arena.lz4_compress(4099, n)
    assert len(c) < n
    dst = (8 << 20) + 8      # the CRC kernel wants an 8 B-aligned offset
    arena.fill(dst - 8, n + 64, 0xEE)
    assert arena.lz4_decompress_into(dst, c) == n
    assert arena.crc32c(dst, n) == native.crc32c(data)
    assert arena.read_bytes(dst - 8, 8) == arena.read_bytes(dst + n, 8) \
        == b"\xee" * 8


def test_range_checks(arena):
    with pytest.raises(RuntimeError, match="out of bounds"):
        arena.lz4_compress((64 << 20) - 100, 101)
    with pytest.raises(RuntimeError, match="per-call limit"):
        arena.lz4_compress(0, (16 << 20) + 1)
    # the largest call still works
    assert len(arena.lz4_compress(0, 16 << 20)) <= worst_case(16 << 20)


def test_replication_hbm_to_hbm(tmp_path):
    from curvine_amd.testing import MiniCluster, test_conf

    data = text8(2 << 20, seed=11) + rand_bytes(1 << 20, 35)

    async def main():
        conf = test_conf(str(tmp_path))
        conf.worker.replication_codec = "lz4"
        mc = MiniCluster(conf=conf, tmp_dir=str(tmp_path), workers=2,
                         worker_dirs=[["[HBM:64MB:0]gpu0"],
                                      ["[HBM:64MB:0]gpu1"]])
        await mc.start()
        try:
            fs = mc.fs()
            await fs.write_all("/r.bin", data, storage_tier="HBM", replicas=1)
            await fs.close()
            src = next(w for w in mc.workers if w.store.block_count())
            dst = next(w for w in mc.workers if w is not src)
            bid = next(iter(src.store.blocks))
            await src._replicate({"cmd": "replicate", "block_id": bid,
                                  "job_id": 1,
                                  "targets": [dst.address().to_dict()],
                                  "tier": "HBM"})
            assert dst.store.blocks[bid].layout.tier == "HBM"
            r = dst.store.open_reader(bid)
            try:
                assert r.read(0, len(data)) == data
            finally:
                r.close()
            assert dst.store.block_crc(bid) == src.store.block_crc(bid) \
                == native.crc32c(data)
            raw = src.counters.get("replication_raw_bytes")
            wire = src.counters.get("replication_wire_bytes")
            assert raw == len(data)
            assert wire < raw
        finally:
            await mc.stop()

    asyncio.new_event_loop().run_until_complete(main())
