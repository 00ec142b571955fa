"""block_absmax_kernel, block_store_kernel and block_load_kernel
(csrc/block_cast.hip) on the MI355X, then save_file(quantize="block") and
load(dequantize=True) through the HBM tier.  Every expected value is the
torch-CPU reference of safetensors_block_cases; comparisons are bitwise,
and sentinel bytes stay on both sides of every destination."""
import numpy as np
import pytest
import torch

from curvine_amd import native
from curvine_amd.testing import test_conf as make_conf

from safetensors_block_cases import (F8, SOURCES, distinct_scales,
                                     expected_block_file, peaked_weights,
                                     random_weights, ref_dequant, ref_quant,
                                     ref_scales, scale_shape)
from safetensors_cases import TORCH, assert_bits_equal
from safetensors_save_cases import check_file, raw_bytes

pytestmark = pytest.mark.gpu

D = native.DTYPES
MiB = 1 << 20
SENTINEL = 0xAB
# (shape, block): edge tiles both ways and many tiles per workgroup; the
# real block size with edge tiles 2 rows high and 72 columns wide; a batch
# of matrices
GEOMETRIES = (((10, 40), (4, 16)), ((130, 200), (128, 128)),
              ((3, 20, 48), (16, 16)))


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(0, 16 * MiB)
    yield a
    a.close()


def tile_elems():
    return native.load().CAST_TILE


def on_gpu(t, elem_off=0):
    """a cuda copy of the cpu tensor `t`, flattened, that begins `elem_off`
    elements into its storage"""
    t = t.reshape(-1)
    buf = torch.zeros(t.numel() + elem_off + 8, dtype=t.dtype,
                      device="cuda:0")
    buf[elem_off:elem_off + t.numel()] = t.to("cuda:0")
    torch.cuda.synchronize()
    return buf[elem_off:elem_off + t.numel()]


def src_name(t):
    return {v: k for k, v in TORCH.items()}[t.dtype]


def big_case(src):
    """more than two workgroup tiles, rows of 100: units cross row ends
    and tile-column edges at every phase"""
    shape, block = (2 * tile_elems() // 100 + 2, 100), (16, 32)
    rng = np.random.default_rng(70)
    w = random_weights(rng, src, shape, block)
    assert w.numel() > 2 * tile_elems() + 100
    assert distinct_scales(w, block) >= 10
    return w, block


def gpu_scales(dev, rows, run, pitch, shape, block):
    """tile scales of rows x run elements whose dense shape is `shape`,
    sentinels checked on both sides"""
    n = int(np.prod(scale_shape(shape, block)))
    out = torch.full((4 * n + 32,), SENTINEL, dtype=torch.uint8,
                     device="cuda:0")
    torch.cuda.synchronize()
    native.block_absmax_scales(0, [(
        dev.data_ptr(), rows, run, pitch * dev.element_size(),
        D[src_name(dev)], out.data_ptr() + 16, 0, run, shape[-2], shape[-1],
        block[0], block[1], n)])
    got = out.cpu()
    assert (got[:16] == SENTINEL).all() and (got[-16:] == SENTINEL).all()
    return got[16:-16].view(torch.float32).reshape(scale_shape(shape, block))


# ------------------------------------------------------------------ absmax

@pytest.mark.parametrize("src", SOURCES)
def test_absmax_geometries(src):
    """tile i has its maximum at in-tile position i: every lane of a unit
    and both sides of each unit and tile edge; then random tiles binades
    apart (a wrong `row % M` shows as the neighbouring matrix's scale)"""
    rng = np.random.default_rng(71)
    for shape, block in GEOMETRIES:
        n = int(np.prod(shape))
        tiles = int(np.prod(scale_shape(shape, block)))
        for w in (peaked_weights(src, shape, block),
                  random_weights(rng, src, shape, block)):
            exp = ref_scales(w, block)
            assert exp.unique().numel() >= min(tiles, 10)
            for elem_off in (0, 1):  # vector loads; a source 1 element in
                got = gpu_scales(on_gpu(w, elem_off), 1, n, n, shape, block)
                assert_bits_equal(got, exp, 0)


@pytest.mark.parametrize("src", SOURCES)
def test_absmax_tiles_and_strided_rows(src):
    w, block = big_case(src)
    w[0, 5], w[3, 77] = float("nan"), float("inf")
    got = gpu_scales(on_gpu(w, 1), 1, w.numel(), w.numel(), w.shape, block)
    assert_bits_equal(got, ref_scales(w, block), 0)
    # a strided view: the gaps hold larger values than any selected element
    rng = np.random.default_rng(72)
    w = random_weights(rng, src, (9, 96), (4, 16))
    w[:, :24] = 30000.0
    w[:, 90:] = -30000.0
    v = w[:, 24:90]
    dev = on_gpu(w, 1)
    got = gpu_scales(dev[24:], 9, 66, 96, (9, 66), (4, 16))
    assert_bits_equal(got, ref_scales(v, (4, 16)), 0)


def special_tensor():
    """NaN and +-Inf beside a finite value, an all-zero tile, f32 max, a
    subnormal-only tile"""
    big = float(np.finfo(np.float32).max)
    w = torch.zeros((8, 48))
    w[0:4, 0:16] = torch.tensor([float("nan"), float("inf"), float("-inf"),
                                 3.0] * 4)
    w[4, 0] = -big
    w[5, 17] = 2.0 ** -140
    w[6, 18] = -(2.0 ** -149)
    w[1, 33], w[2, 40] = 7.0, -0.3
    return w


def test_absmax_special_values():
    w = special_tensor()
    block = (4, 16)
    got = gpu_scales(on_gpu(w), 1, w.numel(), w.numel(), w.shape, block)
    exp = ref_scales(w, block)
    assert_bits_equal(got, exp, 0)
    floor = torch.tensor(2.0 ** -40) / 448
    assert got[0, 0] == torch.tensor(3.0) / 448       # NaN, Inf left out
    assert got[0, 1] == floor and got[1, 1] == floor  # zeros; subnormals


# ------------------------------------------------------------------- store

def store_and_check(arena, dev, w, block, pieces):
    """pieces: [(e0, n, dst_off)] of the flat dense tensor `w` (cpu) whose
    cuda copy is `dev`; scales from the reference; one call, then every
    piece and the bytes between them"""
    s = ref_scales(w, block)
    q = raw_bytes(ref_quant(w, s, block))
    dscale = s.contiguous().to("cuda:0")
    ss = dev.element_size()
    geom = tuple(w.shape[-2:]) + tuple(block)
    top = max(off + n for _, n, off in pieces) + 64
    arena.fill(0, top, SENTINEL)
    torch.cuda.synchronize()
    arena.store_ptr([(dev.data_ptr() + e0 * ss, off, 1, n, n * ss,
                      D[src_name(dev)], D["F8_E4M3"], dscale.data_ptr(), e0,
                      n) + geom for e0, n, off in pieces])
    got = arena.read_bytes(0, top)
    prev = 0
    for e0, n, off in sorted(pieces, key=lambda p: p[2]):
        assert got[prev:off] == bytes([SENTINEL]) * (off - prev), (e0, n, off)
        assert off - prev >= 16
        exp = q[e0:e0 + n]
        if got[off:off + n] != exp:
            g = np.frombuffer(got[off:off + n], dtype=np.uint8)
            bad = np.nonzero(g != np.frombuffer(exp, dtype=np.uint8))[0]
            raise AssertionError(
                f"piece e0={e0} n={n} at {off}: {bad.size} bytes differ, "
                f"first at {bad[0]}: got {g[bad[0]]:#x} expected "
                f"{exp[bad[0]]:#x}")
        prev = off + n
    assert got[prev:] == bytes([SENTINEL]) * (top - prev)


@pytest.mark.parametrize("src", SOURCES)
def test_store_geometries_offsets_and_pieces(arena, src):
    """destination offsets 0..7 x pieces that begin and end mid-row and
    mid-tile, a source one element into its storage"""
    rng = np.random.default_rng(73)
    for shape, block in GEOMETRIES:
        w = random_weights(rng, src, shape, block)
        n = w.numel()
        pieces, off = [], 4096
        for e0, cnt in ((0, n), (7, 50), (n // 2 + 3, n // 3), (41, 2),
                        (n - 9, 9)):
            for d in range(8):
                pieces.append((e0, cnt, off + d))
                off += (cnt + 127) // 64 * 64
        for elem_off in (0, 1):
            store_and_check(arena, on_gpu(w, elem_off), w, block, pieces)


@pytest.mark.parametrize("src", SOURCES)
def test_store_tiles_and_special_values(arena, src):
    w, block = big_case(src)
    w[0, 9], w[2, 41] = float("nan"), float("-inf")
    n = w.numel()
    store_and_check(arena, on_gpu(w, 1), w, block,
                    [(0, n, 4099), (13, tile_elems() + 10, 65536 + 5)])
    if src != "F32":
        return
    w = special_tensor()
    s = ref_scales(w, (4, 16))
    w[1, 34] = float(s[0, 2] * 448)           # exactly 448 times the scale
    assert_bits_equal(ref_scales(w, (4, 16)), s, 0)
    store_and_check(arena, on_gpu(w), w, (4, 16), [(0, w.numel(), 4101)])


def test_store_strided_rows_and_rejects(arena):
    rng = np.random.default_rng(74)
    block = (4, 16)
    w = random_weights(rng, "BF16", (9, 96), block)
    w[:, :24] = 30000.0                       # the gaps: ignored
    v = w[:, 24:90]
    s = ref_scales(v, block)
    q = ref_quant(v, s, block)
    dev = on_gpu(w, 1)
    dscale = s.contiguous().to("cuda:0")
    geom = (9, 66, 4, 16)
    arena.fill(0, 8192, SENTINEL)
    torch.cuda.synchronize()
    # rows 1.. of the view: the piece begins 66 elements in
    arena.store_ptr([(dev.data_ptr() + (96 + 24) * 2, 4101, 8, 66, 96 * 2,
                      D["BF16"], D["F8_E4M3"], dscale.data_ptr(), 66, 66)
                     + geom])
    exp = raw_bytes(q[1:])
    got = arena.read_bytes(4101 - 16, len(exp) + 32)
    assert got[16:-16] == exp
    assert got[:16] == got[-16:] == bytes([SENTINEL]) * 16
    arena.fill(0, 8192, SENTINEL)
    host, hs = torch.ones(64), torch.ones(8)
    torch.cuda.synchronize()
    p, sp, bf, e4 = dev.data_ptr(), dscale.data_ptr(), D["BF16"], D["F8_E4M3"]
    good = (p, 64, 1, 64, 128, bf, e4, sp, 0, 64) + geom
    for seg in [(p, 0, 1, 64, 128, bf, e4, 0, 0, 64) + geom,
                (p, 0, 1, 64, 128, bf, e4, sp + 2, 0, 64) + geom,
                (p, 0, 1, 64, 128, bf, D["F8_E5M2"], sp, 0, 64) + geom,
                (p, 0, 1, 64, 128, D["U8"], e4, sp, 0, 64) + geom,
                (p, 0, 1, 64, 128, bf, e4, sp, 0, 64, 9, 0, 4, 16),
                (p, 0, 1, 64, 128, bf, e4, sp, 0, 64, 9, 66, 0, 16),
                (p, 0, 1, 64, 128, bf, e4, sp, 0, 64, 9, 66, 4, 0),
                (p + 1, 0, 1, 64, 128, bf, e4, sp, 0, 64) + geom,
                (p, 16 * MiB - 8, 1, 64, 128, bf, e4, sp, 0, 64) + geom,
                (p, 0, 1, 64, 128, bf, e4, sp, 1 << 40, 64) + geom,  # scales
                (host.data_ptr(), 0, 1, 64, 128, D["F32"], e4, sp, 0, 64)
                + geom,
                (p, 0, 1, 64, 128, bf, e4, hs.data_ptr(), 0, 64) + geom]:
        with pytest.raises(ValueError):
            arena.store_ptr([good, seg])
    assert arena.read_bytes(0, 8192) == bytes([SENTINEL]) * 8192
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    o = out.data_ptr()
    for seg in [(p, 1, 64, 128, D["U8"], o, 0, 64, 9, 66, 4, 16, 15),
                (p, 1, 64, 128, bf, 0, 0, 64, 9, 66, 4, 16, 15),
                (p, 1, 64, 128, bf, o, 0, 64, 9, 66, 4, 16, 4),   # 5 tiles
                (p, 1, 64, 128, bf, o, 0, 64, 9, 0, 4, 16, 15),
                (host.data_ptr(), 1, 64, 256, D["F32"], o, 0, 64, 9, 66, 4,
                 16, 15),
                (p, 1, 64, 128, bf, hs.data_ptr(), 0, 64, 9, 66, 4, 16, 8)]:
        with pytest.raises(ValueError):
            native.block_absmax_scales(0, [seg])
    assert (out.cpu() == SENTINEL).all()           # refused before launch


# -------------------------------------------------------------------- load

def load_and_check(arena, off, rows, run, pitch_b, dst, dscale, e0, spitch,
                   geom, exp, dst_off=1):
    n = rows * run
    out = torch.zeros(n + 16, dtype=TORCH[dst], device="cuda:0")
    out.view(torch.uint8).fill_(SENTINEL)
    torch.cuda.synchronize()
    arena.convert_ptr([(off, out.data_ptr() + dst_off * out.element_size(),
                        rows, run, pitch_b, D["F8_E4M3"], D[dst],
                        dscale.data_ptr(), e0, spitch) + geom])
    assert_bits_equal(out[dst_off:dst_off + n], exp.reshape(-1), 0)
    side = out.view(torch.uint8).cpu()
    isz = out.element_size()
    assert (side[:dst_off * isz] == SENTINEL).all()
    assert (side[(dst_off + n) * isz:] == SENTINEL).all()


def random_codes(rng, shape):
    codes = rng.integers(0, 256, shape, dtype=np.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x7E               # no NaN code
    return torch.from_numpy(codes).view(F8)


def random_scales(rng, shape):
    """any positive f32 scale, tiles binades apart"""
    return torch.from_numpy(
        (rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(-12, 9, shape)))
        .astype(np.float32))


@pytest.mark.parametrize("dst", SOURCES)
def test_load_geometries_shards_and_pieces(arena, dst):
    """whole tensors from arena offsets 0..3 (odd ones among them) into
    destinations that start inside a 16-byte line; shards along every
    dimension whose parts cut tiles; pieces as a file cut leaves them"""
    rng = np.random.default_rng(75)
    for shape, block in GEOMETRIES:
        q = random_codes(rng, shape)
        s = random_scales(rng, scale_shape(shape, block))
        assert s.unique().numel() >= min(s.numel(), 10)
        full = ref_dequant(q, s, block, TORCH[dst])
        dscale = s.to("cuda:0")
        geom = tuple(shape[-2:]) + tuple(block)
        n, k = q.numel(), shape[-1]
        for a in range(4):
            arena.write(8192 + a, raw_bytes(q))
            load_and_check(arena, 8192 + a, 1, n, n, dst, dscale, 0, n, geom,
                           full, dst_off=1 + a)
        arena.write(8195, raw_bytes(q))
        flat = full.reshape(-1)
        # last-dimension shard 1 of 2: rows of k/2 inside rows of k
        load_and_check(arena, 8195 + k // 2, n // k, k // 2, k, dst, dscale,
                       k // 2, k, geom,
                       full[..., k // 2:].contiguous(), dst_off=0)
        # dim -2 shard 1 of 2 of every matrix
        m = shape[-2]
        load_and_check(arena, 8195 + m // 2 * k, n // (m * k), m // 2 * k,
                       m * k, dst, dscale, m // 2 * k, m * k, geom,
                       full[..., m // 2:, :].contiguous(), dst_off=3)
        for e0, cnt in ((7, 50), (n // 2 + 3, n // 3), (41, 2), (n - 9, 9)):
            load_and_check(arena, 8195 + e0, 1, cnt, cnt, dst, dscale, e0,
                           cnt, geom, flat[e0:e0 + cnt], dst_off=5)


@pytest.mark.parametrize("dst", SOURCES)
def test_load_tiles(arena, dst):
    rng = np.random.default_rng(76)
    shape, block = (2 * tile_elems() // 100 + 2, 100), (16, 32)
    q = random_codes(rng, shape)
    s = random_scales(rng, scale_shape(shape, block))
    full = ref_dequant(q, s, block, TORCH[dst])
    n = q.numel()
    arena.write(8193, raw_bytes(q))
    load_and_check(arena, 8193, 1, n, n, dst, s.to("cuda:0"), 0, n,
                   (shape[0], 100, 16, 32), full, dst_off=1)
    load_and_check(arena, 8193 + 50, shape[0], 50, 100, dst, s.to("cuda:0"),
                   50, 100, (shape[0], 100, 16, 32),
                   full[:, 50:].contiguous(), dst_off=2)


def test_load_rejects(arena):
    out = torch.zeros(128, device="cuda:0")
    sc = torch.ones(8, device="cuda:0")
    host = torch.zeros(128)
    torch.cuda.synchronize()
    p, q, f32, e4 = out.data_ptr(), sc.data_ptr(), D["F32"], D["F8_E4M3"]
    geom = (4, 16, 2, 8)
    good = (0, p, 1, 64, 64, e4, f32, q, 0, 64) + geom
    for seg in [(0, p, 1, 64, 64, e4, D["F64"], q, 0, 64) + geom,
                (0, p, 1, 64, 64, D["F8_E5M2"], f32, q, 0, 64) + geom,
                (0, p, 1, 64, 64, D["F4"], f32, q, 0, 64) + geom,
                (0, p + 2, 1, 64, 64, e4, f32, q, 0, 64) + geom,
                (0, 0, 1, 64, 64, e4, f32, q, 0, 64) + geom,
                (0, p, 1, 64, 64, e4, f32, 0, 0, 64) + geom,
                (0, p, 1, 64, 64, e4, f32, q + 1, 0, 64) + geom,
                (0, p, 1, 64, 64, e4, f32, q, 0, 64, 4, 0, 2, 8),
                (0, p, 1, 64, 64, e4, f32, q, 0, 64, 4, 16, 0, 8),
                (0, p, 1, 64, 64, e4, f32, q, 0, 64, 4, 16, 2, 0),
                (16 * MiB - 8, p, 1, 64, 64, e4, f32, q, 0, 64) + geom,
                (0, p, 1, 1 << 20, 1 << 20, e4, f32, q, 0, 64) + geom,
                (0, p, 1, 64, 64, e4, f32, q, 1 << 40, 64) + geom,
                (0, host.data_ptr(), 1, 64, 64, e4, f32, q, 0, 64) + geom]:
        with pytest.raises(ValueError):
            arena.convert_ptr([good, seg])
    assert (out.cpu() == 0).all()                  # refused before launch


# -------------------------------------------------------------- end to end

def test_end_to_end_hbm(tmp_path, monkeypatch):
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors, save_file
    from curvine_amd.testing import SyncMiniCluster

    rng = np.random.default_rng(77)
    block = (128, 128)
    small = (4, 16)
    w = random_weights(rng, "F32", (9, 96), small)
    cpu = {"b": random_weights(rng, "BF16", (130, 200), block),
           "h": random_weights(rng, "F16", (3, 20, 48), block),
           "bias": random_weights(rng, "F32", (67,), block, spread=False)}
    cpu_small = {"a": random_weights(rng, "F32", (10, 72), small),
                 "h": random_weights(rng, "F16", (3, 20, 48), small),
                 "cols": w[:, 24:90],
                 "b": random_weights(rng, "BF16", (130, 72), small)}
    for name in cpu_small:
        assert distinct_scales(cpu_small[name], small) >= 10
    dev = {k: v.to("cuda:0") for k, v in cpu.items()}
    w_dev = w.to("cuda:0")
    dev_small = {k: v.to("cuda:0") for k, v in cpu_small.items()
                 if k != "cols"}
    dev_small["cols"] = w_dev[:, 24:90]

    conf = make_conf(str(tmp_path))
    smc = SyncMiniCluster(conf=conf, tmp_dir=str(tmp_path),
                          worker_dirs=[["[HBM:512MB:0]gpu0",
                                        "[MEM:64MB]mem0"]]).start()
    try:
        sf = SyncFs(smc.client_conf())
        calls = []
        orig = native.Arena.store_ptr

        def spy(self, segs):
            calls.append((self.device, list(segs)))
            return orig(self, segs)
        monkeypatch.setattr(native.Arena, "store_ptr", spy)
        # block_size 4112 cuts tensors mid-row and mid-tile between blocks
        blob, _start, stored, order = expected_block_file(cpu_small, small)
        assert len(blob) > 3 * 4112
        for bs in (8192, 4112):
            path = f"/blk/dev-small-{bs}.safetensors"
            save_file(sf, dev_small, path, storage_tier="HBM", block_size=bs,
                      quantize="block", quantize_block=small)
            check_file(smc, sf, path, blob)
        blk = [s for d, segs in calls for s in segs if d == 0 and len(s) == 14]
        # typed stores on the GPU, some beginning mid-row and mid-tile
        assert blk and any(s[8] % s[11] and s[8] % s[11] % s[13] for s in blk)
        n_gpu = sum(d == 0 for d, _ in calls)
        save_file(sf, cpu_small, "/blk/cpu-small.safetensors",
                  storage_tier="MEM", block_size=4112, quantize="block",
                  quantize_block=small)
        assert sum(d == 0 for d, _ in calls) == n_gpu
        check_file(smc, sf, "/blk/cpu-small.safetensors", blob)

        blob, _start, stored, order = expected_block_file(cpu)
        save_file(sf, dev, "/blk/dev.safetensors", storage_tier="HBM",
                  block_size=8192, quantize="block", quantize_block=block)
        check_file(smc, sf, "/blk/dev.safetensors", blob)
        save_file(sf, cpu, "/blk/cpu.safetensors", storage_tier="MEM",
                  quantize="block", quantize_block=block)
        check_file(smc, sf, "/blk/cpu.safetensors", blob)

        with CurvineSafetensors(sf, "/blk/dev.safetensors") as f:
            assert f.keys() == order
            for dt in (torch.float32, torch.bfloat16):
                full = {k: ref_dequant(stored[k], stored[k + "_scale_inv"],
                                       block, dt) for k in ("b", "h")}
                out = f.load(device="cuda:0", dtype=dt, dequantize=True)
                assert set(out) == set(cpu)
                for k in full:
                    assert out[k].is_cuda
                    assert_bits_equal(out[k], full[k], 0)
                assert_bits_equal(out["bias"], cpu["bias"].to(dt), 0)
                # world 2 on each dim of (130, 200): parts cut the tiles
                for r in range(2):
                    t = f.get_tensor("b", device="cuda:0", dtype=dt,
                                     shard=(0, r, 2), dequantize=True)
                    assert_bits_equal(t, full["b"][r * 65:(r + 1) * 65], 0)
                    t = f.get_tensor("b", device="cuda:0", dtype=dt,
                                     shard=(1, r, 2), dequantize=True)
                    assert_bits_equal(
                        t, full["b"][:, r * 100:(r + 1) * 100].contiguous(),
                        0)
                into = torch.zeros((3, 10, 48), dtype=dt, device="cuda:0")
                f.load_into("h", into, shard=(1, 1, 2), dequantize=True)
                assert_bits_equal(into, full["h"][:, 10:].contiguous(), 0)
            plain = f.load(device="cuda:0")       # raw fp8 + F32 scales
            assert plain["b"].dtype == F8
            assert_bits_equal(plain["b_scale_inv"], stored["b_scale_inv"], 0)
        with CurvineSafetensors(
                sf, "/blk/dev-small-4112.safetensors") as f:
            assert f.metadata() == {"weight_block_size": "4,16"}
            out = f.load(device="cuda:0", dtype=torch.bfloat16,
                         dequantize=True)     # the block from the metadata
            st = expected_block_file(cpu_small, small)[2]
            for k in cpu_small:
                assert_bits_equal(out[k], ref_dequant(
                    st[k], st[k + "_scale_inv"], small, torch.bfloat16), 0)
        sf.shutdown()
    finally:
        smc.stop()
