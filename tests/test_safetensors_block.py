"""Block-scaled FP8 safetensors (F8_E4M3 + F32 `_scale_inv`, one scale per
bm x bn tile) without a GPU: the host twins of the block_cast kernels on
host memory, save_file(quantize="block") into the MEM tier from cpu tensors
and load(dequantize=True) back.  Every expected value is the torch-CPU
reference of safetensors_block_cases; comparisons are bitwise."""
import json
import struct

import numpy as np
import pytest
import torch

from curvine_amd import errors as err
from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.sdk import CurvineSafetensors, load_file, save_file
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

from safetensors_block_cases import (F8, META_KEY, SOURCES, distinct_scales,
                                     expected_block_file, peaked_weights,
                                     per_element, random_weights, ref_dequant,
                                     ref_quant, ref_scales, scale_shape)
from safetensors_cases import TORCH, assert_bits_equal
from safetensors_save_cases import check_file, raw_bytes

D = native.DTYPES
MiB = 1 << 20
SENTINEL = 0xAB
BLOCK = (4, 16)


@pytest.fixture(scope="module")
def fsx(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("stblk"))
    smc = SyncMiniCluster(conf=make_conf(tmp), tmp_dir=tmp, workers=2).start()
    sf = SyncFs(smc.client_conf())
    yield smc, sf
    sf.shutdown()
    smc.stop()


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(-1, 4 * MiB)
    yield a
    a.close()


@pytest.fixture(scope="module")
def model():
    """block (4, 16): edge tiles in both directions, a batch of matrices,
    a strided view, and tensors the default selection leaves alone"""
    rng = np.random.default_rng(61)
    w = random_weights(rng, "F32", (9, 96), BLOCK)
    m = {"a": random_weights(rng, "F32", (10, 72), BLOCK),
         "b": random_weights(rng, "BF16", (130, 72), BLOCK),
         "h": random_weights(rng, "F16", (3, 20, 48), BLOCK),
         "cols": w[:, 24:90],
         "bias": random_weights(rng, "F32", (67,), BLOCK, spread=False),
         "ids": torch.arange(33, dtype=torch.int64)}
    for name in ("a", "b", "h", "cols"):
        assert distinct_scales(m[name], BLOCK) >= 10, name
    return m


def host_scales(t, block, rows=None, run=None, pitch=None, shape=None):
    """block_absmax_scales on the host for a contiguous or row-strided cpu
    tensor whose dense shape is `shape`"""
    shape = tuple(shape or t.shape)
    rows = 1 if rows is None else rows
    run = int(np.prod(shape)) if run is None else run
    n = int(np.prod(scale_shape(shape, block)))
    out = torch.full((n + 2,), float("nan"))
    src = {v: k for k, v in TORCH.items()}[t.dtype]
    native.block_absmax_scales(-1, [(
        t.data_ptr(), rows, run, (pitch or run) * t.element_size(), D[src],
        out[1:].data_ptr(), 0, run, shape[-2], shape[-1], block[0], block[1],
        n)])
    assert out[0].isnan() and out[-1].isnan()
    return out[1:-1].reshape(scale_shape(shape, block))


# ----------------------------------------------------------- the reference

def test_reference_runs_and_inputs_have_many_scales():
    """the cases module under torch CPU, and its generators: at least ten
    distinct scales per tensor (all tiles where a tensor has fewer), so a
    constant scale cannot pass"""
    rng = np.random.default_rng(60)
    for shape, block in (((10, 40), (4, 16)), ((130, 200), (128, 128)),
                         ((3, 20, 48), (16, 16)), ((64, 200), (4, 16))):
        tiles = int(np.prod(scale_shape(shape, block)))
        for src in SOURCES:
            for w in (peaked_weights(src, shape, block),
                      random_weights(rng, src, shape, block)):
                s = ref_scales(w, block)
                assert s.shape == scale_shape(shape, block)
                assert s.dtype == torch.float32
                q = ref_quant(w, s, block)
                assert q.dtype == F8 and q.shape == w.shape
                y = ref_dequant(q, s, block, torch.bfloat16)
                assert y.shape == w.shape and y.isfinite().all()
                # every tile's maximum lands on the largest code
                assert int((q.view(torch.uint8) & 0x7F).max()) == 0x7E
            # the peaks: 24 magnitudes, one per tile in turn
            assert distinct_scales(peaked_weights(src, shape, block),
                                   block) == min(tiles, 24)
        assert distinct_scales(random_weights(rng, "F32", (64, 200), (4, 16)),
                               (4, 16)) >= 10
    s = torch.arange(6.0).reshape(2, 3)
    e = per_element(s, (3, 40), (2, 16))
    assert e.shape == (3, 40) and e[2, 39] == 5 and e[1, 16] == 1


# --------------------------------------------------------- the host twins

@pytest.mark.parametrize("src", SOURCES)
def test_host_scales(src):
    rng = np.random.default_rng(62)
    for shape, block in (((10, 40), (4, 16)), ((130, 200), (128, 128)),
                         ((3, 20, 48), (16, 16)), ((5, 7), (1, 1))):
        for w in (peaked_weights(src, shape, block),
                  random_weights(rng, src, shape, block)):
            assert_bits_equal(host_scales(w, block), ref_scales(w, block), 0)
    # a strided view: the gaps hold larger values than any selected element
    w = random_weights(rng, src, (9, 96), BLOCK)
    w[:, :24] = 30000.0
    w[:, 90:] = -30000.0
    v = w[:, 24:90]
    got = host_scales(v, BLOCK, 9, 66, 96, (9, 66))
    assert_bits_equal(got, ref_scales(v, BLOCK), 0)


def test_host_scales_special_values():
    big = float(np.finfo(np.float32).max)
    w = torch.zeros((8, 32))
    w[0:4, 0:16] = torch.tensor([float("nan"), float("inf"), float("-inf"),
                                 3.0] * 4)
    # tile (0, 1): all zero -> the floor; tile (1, 0): f32 max
    w[4, 0] = -big
    w[5, 17] = 2.0 ** -140                # tile (1, 1): subnormal only
    got = host_scales(w, BLOCK)
    exp = ref_scales(w, BLOCK)
    assert_bits_equal(got, exp, 0)
    floor = torch.tensor(2.0 ** -40) / 448
    assert got[0, 0] == torch.tensor(3.0) / 448 and got[0, 1] == floor
    assert got[1, 1] == floor and got[1, 0] == torch.tensor(big) / 448


@pytest.mark.parametrize("src", SOURCES)
def test_convert_host_both_ways(src):
    """block_convert_host with pieces that start and end mid-row and
    mid-tile, a scale buffer that starts at a later tile row, and the
    special values"""
    rng = np.random.default_rng(63)
    shape, block = (3, 10, 40), (4, 16)
    w = random_weights(rng, src, shape, block)
    w[0, 0, 0], w[0, 0, 1], w[0, 0, 2], w[0, 1, 3] = \
        float("nan"), float("inf"), -0.0, float("-inf")
    if src == "F32":
        w[2, 9, 30:40] = torch.from_numpy(
            rng.integers(1, 1 << 23, 10).astype(np.uint32).view(np.float32))
    s = ref_scales(w, block)
    # a value at exactly 448 times its tile's scale
    w[1, 5, 20] = (s[1, 1, 1] * 448).to(w.dtype)
    assert_bits_equal(ref_scales(w, block), s, 0)
    q = ref_quant(w, s, block)
    flat, qflat, sn = w.reshape(-1), q.reshape(-1), s.reshape(-1).numpy()
    n = flat.numel()
    for e0, cnt in ((0, n), (7, 50), (395, 30), (41, 700)):
        raw = flat[e0:e0 + cnt].contiguous().view(torch.uint8).numpy()
        got = native.block_convert_host(raw, D[src], D["F8_E4M3"], cnt, sn,
                                        e0, 10, 40, 4, 16)
        assert got == raw_bytes(qflat[e0:e0 + cnt]), (e0, cnt)
    for dst in SOURCES:
        full = ref_dequant(q, s, block, TORCH[dst]).reshape(-1)
        for e0, cnt in ((0, n), (7, 50), (395, 30), (41, 700)):
            got = native.block_convert_host(
                raw_bytes(qflat[e0:e0 + cnt]), D["F8_E4M3"], D[dst], cnt, sn,
                e0, 10, 40, 4, 16)
            assert_bits_equal(
                torch.frombuffer(bytearray(got), dtype=TORCH[dst]),
                full[e0:e0 + cnt], 1 if e0 == 0 else 0)
        # the scales of matrix 1 on only: tile rows 3.., index 9
        e0, cnt = 400 + 45, 300
        got = native.block_convert_host(
            raw_bytes(qflat[e0:e0 + cnt]), D["F8_E4M3"], D[dst], cnt, sn[9:],
            e0, 10, 40, 4, 16, 9)
        assert_bits_equal(torch.frombuffer(bytearray(got), dtype=TORCH[dst]),
                          full[e0:e0 + cnt], 0)
    with pytest.raises(ValueError):           # the buffer misses tile row 2
        native.block_convert_host(raw_bytes(qflat[300:400]), D["F8_E4M3"],
                                  D["F32"], 100, sn[9:], 300, 10, 40, 4, 16, 9)
    with pytest.raises(ValueError):
        native.block_convert_host(raw_bytes(qflat[:100]), D["F8_E4M3"],
                                  D["F32"], 100, sn[:2], 0, 10, 40, 4, 16)


def test_support_tables():
    assert native.BLOCK_DEFAULT == (128, 128)
    assert native.block_quantize_supported("BF16")
    assert not native.block_quantize_supported("F64")
    assert not native.block_quantize_supported("F8_E4M3")
    assert native.block_dequantize_supported("F16")
    assert not native.block_dequantize_supported("F64")
    assert native.block_scale_shape((3, 130, 200), (128, 128)) == (3, 2, 2)


def test_native_rejects(arena):
    x = torch.ones(64)
    s = torch.ones(8)
    p, q = x.data_ptr(), s.data_ptr()
    arena.fill(0, 4096, SENTINEL)
    f32, e4 = D["F32"], D["F8_E4M3"]
    good = (p, 64, 1, 64, 256, f32, e4, q, 0, 64, 4, 16, 2, 8)
    for seg in [(p, 0, 1, 64, 256, D["I32"], e4, q, 0, 64, 4, 16, 2, 8),
                (p, 0, 1, 64, 256, f32, D["F8_E5M2"], q, 0, 64, 4, 16, 2, 8),
                (p, 0, 1, 64, 256, f32, D["F4"], q, 0, 64, 4, 16, 2, 8),
                (p, 0, 1, 64, 256, f32, e4, 0, 0, 64, 4, 16, 2, 8),
                (p, 0, 1, 64, 256, f32, e4, q + 2, 0, 64, 4, 16, 2, 8),
                (p, 0, 1, 64, 256, f32, e4, q, 0, 64, 4, 0, 2, 8),   # K
                (p, 0, 1, 64, 256, f32, e4, q, 0, 64, 0, 16, 2, 8),  # M
                (p, 0, 1, 64, 256, f32, e4, q, 0, 64, 4, 16, 0, 8),  # bm
                (p, 0, 1, 64, 256, f32, e4, q, 0, 64, 4, 16, 2, 0),  # bn
                (0, 0, 1, 64, 256, f32, e4, q, 0, 64, 4, 16, 2, 8),
                (p + 2, 0, 1, 32, 256, f32, e4, q, 0, 64, 4, 16, 2, 8),
                (p, 4 * MiB - 8, 1, 64, 256, f32, e4, q, 0, 64, 4, 16, 2, 8),
                (p, 0, 2, 32, 64, f32, e4, q, 0, 32, 4, 16, 2, 8),   # overlap
                (p, 0, 2, 32, 128, f32, e4, q, 0, 16, 4, 16, 2, 8)]:
        with pytest.raises(ValueError):
            arena.store_ptr([good, seg])
    assert arena.read_bytes(0, 4096) == bytes([SENTINEL]) * 4096
    for seg in [(0, p, 1, 64, 64, e4, D["F64"], q, 0, 64, 4, 16, 2, 8),
                (0, p, 1, 64, 64, D["F8_E5M2"], f32, q, 0, 64, 4, 16, 2, 8),
                (0, p + 2, 1, 32, 32, e4, f32, q, 0, 64, 4, 16, 2, 8),
                (0, 0, 1, 32, 32, e4, f32, q, 0, 64, 4, 16, 2, 8),
                (4 * MiB - 8, p, 1, 64, 64, e4, f32, q, 0, 64, 4, 16, 2, 8),
                (0, p, 1, 64, 64, e4, f32, q, 0, 64, 4, 16, 2, 0)]:
        with pytest.raises(ValueError):
            arena.convert_ptr([seg])
    assert torch.equal(x, torch.ones(64))
    before = s.clone()
    for seg in [(p, 1, 64, 256, D["U8"], q, 0, 64, 4, 16, 2, 8, 4),
                (p, 1, 64, 256, f32, 0, 0, 64, 4, 16, 2, 8, 4),
                (p, 1, 64, 256, f32, q + 1, 0, 64, 4, 16, 2, 8, 4),
                (p, 1, 64, 256, f32, q, 0, 64, 4, 16, 2, 8, 0),
                (p, 1, 64, 256, f32, q, 0, 64, 4, 16, 2, 8, 3),   # 4 tiles
                (p, 1, 64, 256, f32, q, 0, 64, 4, 0, 2, 8, 4),
                (p + 1, 1, 64, 256, f32, q, 0, 64, 4, 16, 2, 8, 4)]:
        with pytest.raises(ValueError):
            native.block_absmax_scales(-1, [seg])
    assert torch.equal(s, before)


@pytest.mark.parametrize("src", SOURCES)
def test_host_arena_store_and_load(arena, src):
    """the MEM tier's route: pieces at odd arena offsets that start
    mid-row and mid-tile, strided rows, then whole and sharded loads"""
    rng = np.random.default_rng(64)
    w = random_weights(rng, src, (9, 96), BLOCK)
    v = w[:, 24:90]                           # dense (9, 66)
    s = ref_scales(v, BLOCK)
    q = ref_quant(v, s, BLOCK)
    sc = s.contiguous()
    ss = w.element_size()
    geom = (9, 66, 4, 16)
    arena.fill(0, 8192, SENTINEL)
    # whole rows from row 1, and the tail of row 0 from element 24
    arena.store_ptr([
        (v[1].data_ptr(), 4099, 8, 66, 96 * ss, D[src], D["F8_E4M3"],
         sc.data_ptr(), 66, 66) + geom,
        (v[0, 24:].data_ptr(), 2051, 1, 42, 0, D[src], D["F8_E4M3"],
         sc.data_ptr(), 24, 42) + geom])
    got = arena.read_bytes(4099 - 16, 8 * 66 + 32)
    assert got[16:-16] == raw_bytes(q[1:])
    assert got[:16] == got[-16:] == bytes([SENTINEL]) * 16
    got = arena.read_bytes(2051 - 16, 42 + 32)
    assert got[16:-16] == raw_bytes(q[0, 24:])
    assert got[:16] == got[-16:] == bytes([SENTINEL]) * 16
    # load: the whole tensor, a column shard that cuts tiles, a piece
    arena.write(1027, raw_bytes(q))
    for dst in SOURCES:
        full = ref_dequant(q, s, BLOCK, TORCH[dst])
        out = torch.zeros((9, 66), dtype=TORCH[dst])
        arena.convert_ptr([(1027, out.data_ptr(), 1, 594, 594, D["F8_E4M3"],
                            D[dst], sc.data_ptr(), 0, 594) + geom])
        assert_bits_equal(out, full, 0)
        out = torch.zeros((9, 33), dtype=TORCH[dst])
        arena.convert_ptr([(1027 + 33, out.data_ptr(), 9, 33, 66,
                            D["F8_E4M3"], D[dst], sc.data_ptr(), 33, 66)
                           + geom])
        assert_bits_equal(out, full[:, 33:].contiguous(), 0)
        out = torch.zeros(100, dtype=TORCH[dst])
        arena.convert_ptr([(1027 + 41, out.data_ptr(), 1, 100, 100,
                            D["F8_E4M3"], D[dst], sc.data_ptr(), 41, 100)
                           + geom])
        assert_bits_equal(out, full.reshape(-1)[41:141], 0)


# ------------------------------------------------------------------- save

def test_save_mem_tier(fsx, model):
    """the host-arena path: file bytes equal the expected file"""
    smc, sf = fsx
    blob, start, stored, order = expected_block_file(model, BLOCK,
                                                     {"format": "pt"})
    path = "/blk/mem.safetensors"
    st = save_file(sf, model, path, metadata={"format": "pt"},
                   storage_tier="MEM", block_size=4096, quantize="block",
                   quantize_block=BLOCK)
    assert st.length == len(blob) and len(blob) > 3 * 4096
    check_file(smc, sf, path, blob)
    got = sf.read_file(path)
    (n,) = struct.unpack("<Q", got[:8])
    doc = json.loads(got[8:8 + n])
    assert doc["__metadata__"] == {"format": "pt", META_KEY: "4,16"}
    for name in ("a", "b", "h", "cols"):
        shape = list(model[name].shape)
        assert doc[name]["dtype"] == "F8_E4M3" and doc[name]["shape"] == shape
        assert doc[name + "_scale_inv"]["dtype"] == "F32"
        assert doc[name + "_scale_inv"]["shape"] == \
            list(scale_shape(shape, BLOCK))
        assert name + "_scale" not in doc
    for name in ("bias", "ids"):                  # not selected: as ever
        assert doc[name]["dtype"] in ("F32", "I64")
        assert name + "_scale_inv" not in doc
    assert [k for k in doc if k != "__metadata__"] == order


def test_save_real_block_and_metadata(fsx):
    smc, sf = fsx
    rng = np.random.default_rng(65)
    tens = {"w": random_weights(rng, "BF16", (130, 200), (128, 128))}
    blob = expected_block_file(tens)[0]
    save_file(sf, tens, "/blk/default.safetensors", storage_tier="MEM",
              quantize="block", quantize_block=(128, 128))
    check_file(smc, sf, "/blk/default.safetensors", blob)
    with CurvineSafetensors(sf, "/blk/default.safetensors") as f:
        assert f.metadata() == {META_KEY: "128,128"}
        assert f.info("w_scale_inv").shape == (2, 2)
    # the caller's own equal value is kept where it stands
    meta = {META_KEY: "128,128", "format": "pt"}
    save_file(sf, tens, "/blk/meta.safetensors", storage_tier="MEM",
              quantize="block", quantize_block=[128, 128], metadata=meta)
    check_file(smc, sf, "/blk/meta.safetensors",
               expected_block_file(tens, metadata=meta)[0])
    assert meta == {META_KEY: "128,128", "format": "pt"}


def test_save_cut_mid_tile_equals_uncut(fsx, model):
    """block_size 4112: tensors are cut mid-row and mid-tile between two
    file blocks"""
    smc, sf = fsx
    blob, start, _, _ = expected_block_file(model, BLOCK)
    assert start % 64 == 0 and len(blob) > 3 * 4112
    save_file(sf, model, "/blk/cut.safetensors", storage_tier="MEM",
              block_size=4112, quantize="block", quantize_block=BLOCK)
    check_file(smc, sf, "/blk/cut.safetensors", blob)


@pytest.mark.parametrize("how", ["file_tier", "replicas"])
def test_save_byte_path_identical(fsx, model, how, monkeypatch):
    smc, sf = fsx
    calls = []
    orig = native.Arena.store_ptr
    monkeypatch.setattr(native.Arena, "store_ptr",
                        lambda self, segs: (calls.append(segs),
                                            orig(self, segs))[1])
    kw = {"storage_tier": "SSD"} if how == "file_tier" else \
        {"storage_tier": "MEM", "replicas": 2}
    path = f"/blk/{how}.safetensors"
    save_file(sf, model, path, block_size=4112, quantize="block",
              quantize_block=BLOCK, **kw)
    assert calls == []                            # no typed store
    check_file(smc, sf, path, expected_block_file(model, BLOCK)[0])


def test_save_filter_and_views(fsx):
    smc, sf = fsx
    rng = np.random.default_rng(66)
    w = random_weights(rng, "BF16", (12, 6, 64), BLOCK)
    tens = {"t": random_weights(rng, "F32", (64, 9), BLOCK).t(),  # temporary
            "inner": w[:, :, 30:],      # rows of 34 inside rows of 64
            "rows": w[3:9],
            "keep": random_weights(rng, "F32", (4, 32), BLOCK)}

    def pick(name, t):
        return name != "keep"
    blob = expected_block_file(tens, BLOCK, selected=pick)[0]
    save_file(sf, tens, "/blk/filter.safetensors", storage_tier="MEM",
              block_size=512, quantize="block", quantize_block=BLOCK,
              quantize_filter=pick)
    check_file(smc, sf, "/blk/filter.safetensors", blob)


# ------------------------------------------------------------------- load

@pytest.mark.parametrize("src", SOURCES)
def test_round_trip(fsx, src):
    """save then load(dequantize=True) against the reference"""
    _, sf = fsx
    rng = np.random.default_rng(67)
    block = (16, 16)
    tens = {"w": random_weights(rng, src, (3, 20, 48), block),
            "e": peaked_weights(src, (10, 40), block)}
    path = f"/blk/rt-{src}.safetensors"
    save_file(sf, tens, path, storage_tier="MEM", block_size=1024,
              quantize="block", quantize_block=block)
    for dst in SOURCES:
        out = load_file(sf, path, device="cpu", dtype=TORCH[dst],
                        dequantize=True)
        assert set(out) == {"w", "e"}
        for name, t in tens.items():
            s = ref_scales(t, block)
            assert_bits_equal(out[name], ref_dequant(
                ref_quant(t, s, block), s, block, TORCH[dst]), 0)


@pytest.mark.parametrize("dst", SOURCES)
def test_load_dequantize(fsx, model, dst):
    _, sf = fsx
    dt = TORCH[dst]
    path = f"/blk/load-{dst}.safetensors"
    save_file(sf, model, path, storage_tier="MEM", block_size=4112,
              quantize="block", quantize_block=BLOCK)
    stored = expected_block_file(model, BLOCK)[2]

    def ref(name):
        return ref_dequant(stored[name], stored[name + "_scale_inv"], BLOCK,
                           dt)
    out = load_file(sf, path, device="cpu", dtype=dt, dequantize=True)
    assert set(out) == set(model)                 # no _scale_inv entries
    for name in ("a", "b", "h", "cols"):
        assert_bits_equal(out[name], ref(name), 0)
    assert_bits_equal(out["bias"], model["bias"].to(dt), 0)
    assert_bits_equal(out["ids"], model["ids"], 0)
    with CurvineSafetensors(sf, path) as f:
        # names asking for the scale
        got = f.load(device="cpu", names=["a", "a_scale_inv"],
                     dequantize=True)
        assert got["a"].dtype == torch.float32    # dtype None: F32
        assert_bits_equal(got["a"], ref_dequant(
            stored["a"], stored["a_scale_inv"], BLOCK, torch.float32), 0)
        assert_bits_equal(got["a_scale_inv"], stored["a_scale_inv"], 0)
        into = torch.zeros(model["h"].shape, dtype=dt)
        f.load_into("h", into, dequantize=True)
        assert_bits_equal(into, ref("h"), 0)
        full = ref("b")                           # (130, 72): parts cut tiles
        for r in range(2):
            t = f.get_tensor("b", device="cpu", dtype=dt, shard=(0, r, 2),
                             dequantize=True)
            assert_bits_equal(t, full[r * 65:(r + 1) * 65], 0)
            t = f.get_tensor("b", device="cpu", dtype=dt, shard=(-1, r, 2),
                             dequantize=True)
            assert_bits_equal(t, full[:, r * 36:(r + 1) * 36].contiguous(), 0)
        for dim, world in ((0, 3), (1, 4), (2, 3)):
            for r in range(world):
                t = f.get_tensor("h", device="cpu", dtype=dt,
                                 shard=(dim, r, world), dequantize=True)
                part = model["h"].shape[dim] // world
                assert_bits_equal(t, ref("h").narrow(dim, r * part, part)
                                  .contiguous(), 0)
        into = torch.zeros((10, 36), dtype=dt)
        f.load_into("a", into, shard=(1, 1, 2), dequantize=True)
        assert_bits_equal(into, ref("a")[:, 36:].contiguous(), 0)
        with pytest.raises(err.Unsupported):
            f.get_tensor("b", device="cpu", dtype=torch.float64,
                         dequantize=True)
        # without dequantize: raw fp8 and the F32 scales, as ever
        raw = f.load(device="cpu")
        assert set(raw) == set(stored)
        assert raw["a"].dtype == F8
        assert_bits_equal(raw["a_scale_inv"], stored["a_scale_inv"], 0)


def test_load_file_tier_slow_path(fsx, model):
    """the pread + host-convert route gives the same bits"""
    _, sf = fsx
    path = "/blk/ssd-load.safetensors"
    save_file(sf, model, path, storage_tier="SSD", block_size=4112,
              quantize="block", quantize_block=BLOCK)
    stored = expected_block_file(model, BLOCK)[2]
    out = load_file(sf, path, device="cpu", dtype=torch.bfloat16,
                    dequantize=True)
    for name in ("a", "b", "h", "cols"):
        assert_bits_equal(out[name], ref_dequant(
            stored[name], stored[name + "_scale_inv"], BLOCK,
            torch.bfloat16), 0)
    with CurvineSafetensors(sf, path) as f:
        t = f.get_tensor("b", device="cpu", shard=(1, 1, 2), dequantize=True)
        assert_bits_equal(t, ref_dequant(
            stored["b"], stored["b_scale_inv"], BLOCK,
            torch.float32)[:, 36:].contiguous(), 0)


def test_resave_round_trip(fsx, model):
    """a loaded block-scaled checkpoint saved back without `quantize`
    keeps its fp8 and F32 tensors byte for byte"""
    smc, sf = fsx
    blob = expected_block_file(model, BLOCK)[0]
    save_file(sf, model, "/blk/first.safetensors", storage_tier="MEM",
              quantize="block", quantize_block=BLOCK)
    with CurvineSafetensors(sf, "/blk/first.safetensors") as f:
        raw, meta = f.load(device="cpu"), f.metadata()
    save_file(sf, raw, "/blk/again.safetensors", storage_tier="MEM",
              block_size=4112, metadata=meta)
    check_file(smc, sf, "/blk/again.safetensors", blob)


def hand_written(tensors, metadata=None):
    """a safetensors file from (name, dtype, shape, raw bytes) with struct
    and json alone"""
    hdr, pos = {}, 0
    if metadata is not None:
        hdr["__metadata__"] = metadata
    for name, dt, shape, raw in tensors:
        hdr[name] = {"dtype": dt, "shape": list(shape),
                     "data_offsets": [pos, pos + len(raw)]}
        pos += len(raw)
    js = json.dumps(hdr).encode()
    return struct.pack("<Q", len(js)) + js + b"".join(t[3] for t in tensors)


@pytest.fixture(scope="module")
def foreign(fsx):
    """`weight` / `weight_scale_inv` as other writers name them, fp8 codes
    and scales chosen freely (not this project's scale rule)"""
    _, sf = fsx
    rng = np.random.default_rng(68)
    codes = rng.integers(0, 256, (130, 200), dtype=np.uint8)
    codes[codes == 0x7F] = 0x7E
    codes[codes == 0xFF] = 0xFE
    q = torch.from_numpy(codes).view(F8)
    s = torch.from_numpy(np.exp2(rng.integers(-9, 5, (2, 2)))
                         .astype(np.float32)) * 1.25
    s4 = torch.from_numpy(rng.uniform(0.001, 2.0, (33, 13))
                          .astype(np.float32))
    files = {
        "/blk/hf.safetensors": hand_written(
            [("model.layers.0.mlp.weight", "F8_E4M3", (130, 200),
              codes.tobytes()),
             ("model.layers.0.mlp.weight_scale_inv", "F32", (2, 2),
              raw_bytes(s))]),
        "/blk/hf-meta.safetensors": hand_written(
            [("weight", "F8_E4M3", (130, 200), codes.tobytes()),
             ("weight_scale_inv", "F32", (33, 13), raw_bytes(s4))],
            {META_KEY: "4,16"}),
        "/blk/both.safetensors": hand_written(
            [("weight", "F8_E4M3", (130, 200), codes.tobytes()),
             ("weight_scale", "F32", (1,), raw_bytes(torch.tensor([0.5]))),
             ("weight_scale_inv", "F32", (2, 2), raw_bytes(s))]),
    }
    for path, blob in files.items():
        sf.write_file(path, blob, storage_tier="MEM")
        assert sf.read_file(path) == blob
    return q, s, s4


def test_hand_written_file(fsx, foreign):
    _, sf = fsx
    q, s, _ = foreign
    name = "model.layers.0.mlp.weight"
    for dst in SOURCES:
        out = load_file(sf, "/blk/hf.safetensors", device="cpu",
                        dtype=TORCH[dst], dequantize=True)
        assert set(out) == {name}
        assert_bits_equal(out[name], ref_dequant(q, s, (128, 128),
                                                 TORCH[dst]), 0)
    raw = load_file(sf, "/blk/hf.safetensors", device="cpu")
    assert set(raw) == {name, name + "_scale_inv"} and raw[name].dtype == F8


def test_scale_block_sources(fsx, foreign):
    """the keyword, the metadata, the default"""
    _, sf = fsx
    q, s, s4 = foreign
    exp4 = ref_dequant(q, s4, (4, 16), torch.float32)
    with CurvineSafetensors(sf, "/blk/hf-meta.safetensors") as f:
        # metadata says 4,16
        assert_bits_equal(f.get_tensor("weight", device="cpu",
                                       dequantize=True), exp4, 0)
        assert set(f.load(device="cpu", dequantize=True)) == {"weight"}
        # the keyword overrides it: (128, 128) does not fit (33, 13) ->
        # the tensor loads unscaled and the scale is an ordinary tensor
        out = f.load(device="cpu", dequantize=True, scale_block=(128, 128))
        assert set(out) == {"weight", "weight_scale_inv"}
        assert_bits_equal(out["weight"], q, 0)
        assert_bits_equal(f.get_tensor("weight", device="cpu",
                                       dequantize=True, scale_block=[4, 16]),
                          exp4, 0)
        into = torch.zeros((130, 200))
        f.load_into("weight", into, dequantize=True, scale_block=(4, 16))
        assert_bits_equal(into, exp4, 0)
        for bad in ((0, 16), (4,), (4, 16, 1), (4.0, 16), "4,16", 128,
                    (True, 16), (-4, 16)):
            with pytest.raises(err.InvalidArgument):
                f.load(device="cpu", dequantize=True, scale_block=bad)
            with pytest.raises(err.InvalidArgument):
                f.load_into("weight", into, dequantize=True, scale_block=bad)
    # no metadata: the default (128, 128); the keyword can say otherwise
    with CurvineSafetensors(sf, "/blk/hf.safetensors") as f:
        name = "model.layers.0.mlp.weight"
        assert_bits_equal(
            f.get_tensor(name, device="cpu", dequantize=True),
            ref_dequant(q, s, (128, 128), torch.float32), 0)
        # (65, 100) gives the same (2, 2) scale shape with other tiles
        assert_bits_equal(
            f.get_tensor(name, device="cpu", dequantize=True,
                         scale_block=(65, 100)),
            ref_dequant(q, s, (65, 100), torch.float32), 0)
        out = load_file(sf, "/blk/hf.safetensors", device="cpu",
                        dequantize=True, scale_block=(64, 64))
        assert set(out) == {name, name + "_scale_inv"}     # (3, 4) != (2, 2)
        assert_bits_equal(out[name], q, 0)


def test_scale_wins_over_scale_inv(fsx, foreign):
    _, sf = fsx
    q, s, _ = foreign
    out = load_file(sf, "/blk/both.safetensors", device="cpu",
                    dequantize=True)
    assert set(out) == {"weight", "weight_scale_inv"}
    assert_bits_equal(out["weight"], q.float() * 0.5, 0)
    assert_bits_equal(out["weight_scale_inv"], s, 0)


def test_mismatched_scale_inv_loads_raw(fsx):
    _, sf = fsx
    q = torch.arange(64, dtype=torch.uint8).view(F8).reshape(2, 32)
    for i, s in enumerate((torch.ones((1, 2)), torch.ones((2,)),
                           torch.ones((1, 1), dtype=torch.float16))):
        path = f"/blk/wrong{i}.safetensors"
        save_file(sf, {"q": q, "q_scale_inv": s}, path, storage_tier="MEM")
        out = load_file(sf, path, device="cpu", dtype=torch.bfloat16,
                        dequantize=True)
        assert set(out) == {"q", "q_scale_inv"}
        assert_bits_equal(out["q"], q.to(torch.bfloat16), 0)
    # a vector has no two dimensions to tile
    save_file(sf, {"v": q.reshape(64), "v_scale_inv": torch.ones((1, 1))},
              "/blk/vec.safetensors", storage_tier="MEM")
    out = load_file(sf, "/blk/vec.safetensors", device="cpu", dequantize=True)
    assert set(out) == {"v", "v_scale_inv"} and out["v"].dtype == F8


# --------------------------------------------------------------- refusals

def test_refused_before_create(fsx):
    _, sf = fsx
    w = torch.ones((4, 64))

    def every(n, t):
        return True
    real = (128, 128)
    cases = [
        # the geometry of a written file is named, never assumed
        (dict(tensors={"w": w}, quantize="block"), err.InvalidArgument),
        (dict(tensors={"w": w, "w_scale_inv": torch.ones((1, 1))},
              quantize="block", quantize_block=real), err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="block", quantize_block=real,
              metadata={META_KEY: "64,64"}), err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="block", quantize_block=(4, 16),
              metadata={META_KEY: "128,128"}), err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="row", quantize_block=real),
         err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="mxfp8", quantize_block=real),
         err.InvalidArgument),
        (dict(tensors={"w": w}, quantize_block=real), err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="block", quantize_block=(0, 128)),
         err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="block", quantize_block=(128,)),
         err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="block", quantize_block=128),
         err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="block", quantize_block=(4.0, 16)),
         err.InvalidArgument),
        (dict(tensors={"w": torch.ones(64)}, quantize="block",
              quantize_block=real, quantize_filter=every),
         err.InvalidArgument),
        (dict(tensors={"w": w.double()}, quantize="block",
              quantize_block=real, quantize_filter=every), err.Unsupported),
        (dict(tensors={"w": w.to(torch.int32)}, quantize="block",
              quantize_block=real, quantize_filter=every), err.Unsupported),
        (dict(tensors={"w": w.to(F8)}, quantize="block",
              quantize_block=real, quantize_filter=every), err.Unsupported),
        # a given `w_scale` would win over the `_scale_inv` on load
        (dict(tensors={"w": w, "w_scale": torch.ones(1)}, quantize="block",
              quantize_block=real), err.InvalidArgument),
    ]
    for i, (kw, exc) in enumerate(cases):
        path = f"/blk/refused{i}.safetensors"
        tensors = kw.pop("tensors")
        with pytest.raises(exc):
            save_file(sf, tensors, path, storage_tier="MEM", **kw)
        assert not sf.exists(path), i
    # the same tensors with the geometry named are accepted
    save_file(sf, {"w": w}, "/blk/accepted.safetensors", storage_tier="MEM",
              quantize="block", quantize_block=real)
    with CurvineSafetensors(sf, "/blk/accepted.safetensors") as f:
        assert sorted(f.keys()) == ["w", "w_scale_inv"]
