"""Cases for the plumbing the native kernel entry points share: the scratch
carver, the tile tables and the per-device CRC tables.  Written once against
the Arena interface, as kernel_edge_cases.py is: test_native_plumbing.py runs
them on a host arena (device -1) and, marked gpu, on device 0.  Every
comparison is bitwise.
"""
import numpy as np

from curvine_amd import native
from kernel_edge_cases import GUARD

MIB = 1 << 20
CHUNK = 65536               # LZ4 chunk

SRC_OFF, SRC_N = 0, 2 * MIB
CAST_OFF = 2 * MIB
LZ4_OFF = 3 * MIB
LZ4_DST = 4 * MIB + 7
GATHER = ((3, 1), (1001, 65537), (200001, 4096))
CRC_OFF, CRC_N = 5, 4096 * 257 + 3


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _gather(arena, src):
    total = sum(n for _, n in GATHER)
    out = np.full(total + 32, GUARD, dtype=np.uint8)
    arena.gather(list(GATHER), out, 16)
    guard = np.full(16, GUARD, dtype=np.uint8)
    want = np.concatenate([guard] + [src[o:o + n] for o, n in GATHER] + [guard])
    assert np.array_equal(out, want)


def scratch_reuse(arena, dst_factory):
    """One 8 MiB arena, six calls that lay its scratch out five ways and
    grow it twice (gather -> LZ4 slots -> the CRC partials with the staging
    slack).  A region carved wrongly, or a pointer kept across a regrow,
    comes out as a wrong byte in one of the results."""
    src = _rand(SRC_N, 51)
    arena.write(SRC_OFF, src, 0, SRC_N)
    _gather(arena, src)

    n_el = native.load().CAST_TILE + 1
    f32 = np.random.default_rng(52).standard_normal(n_el).astype(np.float32)
    arena.write(CAST_OFF, f32.view(np.uint8), 0, 4 * n_el)
    dst = dst_factory(2 * n_el + 64, GUARD)
    F32, BF16 = native.DTYPES["F32"], native.DTYPES["BF16"]
    arena.convert_ptr([(CAST_OFF, dst.ptr + 32, 1, n_el, 4 * n_el, F32, BF16)])
    got = dst.numpy()
    assert got[32:32 + 2 * n_el].tobytes() == \
        native.convert_host(f32.view(np.uint8), F32, BF16, n_el)
    assert (got[:32] == GUARD).all() and (got[32 + 2 * n_el:] == GUARD).all()

    raw = (b"the quick brown fox jumps over the lazy dog; " * 3000)[:2 * CHUNK + 1]
    assert len(raw) == 2 * CHUNK + 1
    arena.write(LZ4_OFF, raw, 0, len(raw))
    container = arena.lz4_compress(LZ4_OFF, len(raw))
    assert len(container) < len(raw)
    assert native.lz4_decompress(container) == raw

    assert arena.lz4_decompress_into(LZ4_DST, container) == len(raw)
    assert arena.read_bytes(LZ4_DST, len(raw)) == raw

    assert arena.crc32c(CRC_OFF, CRC_N) == \
        native.crc32c(src[CRC_OFF:CRC_OFF + CRC_N])

    _gather(arena, src)


def crc_two_arenas(device):
    """Two arenas on one device share that device's CRC tables: the second
    arena's first CRC must not disturb, or depend on, the first arena's."""
    n = 65536 + 5
    arenas = [native.Arena(device, MIB, staging_bytes=MIB, staging_count=2)
              for _ in range(2)]
    try:
        data = [_rand(n, 53), _rand(n, 54)]
        for a, d in zip(arenas, data):
            a.write(0, d, 0, n)
        for i in (1, 0, 1):
            assert arenas[i].crc32c(0, n) == native.crc32c(data[i]), i
    finally:
        for a in arenas:
            a.close()
