"""MXFP8 / MXFP4 safetensors without a GPU: the host twins of the mx_cast
kernels on host memory, save_file(quantize="mxfp8" | "mxfp4") into the MEM
tier from cpu tensors and load(dequantize=True) back.  Every expected
value is the float64 reference of safetensors_mx_cases; comparisons are
bitwise."""
import json
import struct

import numpy as np
import pytest
import torch

from curvine_amd import errors as err
from curvine_amd import native
from curvine_amd.client.filesystem import SyncFs
from curvine_amd.sdk import CurvineSafetensors, load_file, save_file
from curvine_amd.sdk.safetensors_io import parse_header
from curvine_amd.testing import SyncMiniCluster
from curvine_amd.testing import test_conf as make_conf

from safetensors_cases import assert_bits_equal, raw_header
from safetensors_mx_cases import (SOURCES, STORED, TDT, count_nan,
                                  expected_mx_file, pack, per_element,
                                  random_weights, ref_dequant, ref_quant,
                                  ref_scales, widen)
from safetensors_save_cases import check_file

D = native.DTYPES
MiB = 1 << 20
SENTINEL = 0xAB
MODES = ("mxfp8", "mxfp4")


@pytest.fixture(scope="module")
def fsx(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("stmx"))
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
    rng = np.random.default_rng(51)
    w = random_weights(rng, "F32", (9, 96))
    return {"a": random_weights(rng, "F32", (5, 64)),
            "b": random_weights(rng, "BF16", (130, 256)),
            "h": random_weights(rng, "F16", (3, 4, 32)),
            "cols": w[:, 32:96],
            "bias": random_weights(rng, "F32", (67,)),
            "odd": random_weights(rng, "F32", (4, 33)),
            "ids": torch.arange(33, dtype=torch.int64)}


def host_scales(t, stored, rows=None, run=None, pitch=None):
    """mx_scales on the host for a contiguous or row-strided cpu tensor"""
    rows = 1 if rows is None else rows
    run = t.numel() if run is None else run
    out = torch.full((rows * run // 32 + 2,), SENTINEL, dtype=torch.uint8)
    src = {v: k for k, v in TDT.items()}[t.dtype]
    native.mx_scales(-1, [(t.data_ptr(), rows, run,
                           (pitch or run) * t.element_size(), D[src],
                           D[stored], out[1:].data_ptr())])
    assert out[0] == SENTINEL and out[-1] == SENTINEL
    return out[1:-1].numpy()


# ------------------------------------------------------------- the formats

def test_element_tables_against_torch():
    """the reference's own decode tables are torch's"""
    from safetensors_mx_cases import TABLE
    q = torch.arange(128, dtype=torch.uint8).view(torch.float8_e4m3fn)
    t = q.double().numpy()
    assert np.array_equal(t[:127], TABLE["F8_E4M3"][:127]) and np.isnan(t[127])
    assert list(TABLE["F4"]) == [0, 0.5, 1, 1.5, 2, 3, 4, 6]


@pytest.mark.parametrize("stored", ["F8_E4M3", "F4"])
def test_scale_rule(stored):
    emax = 8 if stored == "F8_E4M3" else 2
    big = float(np.finfo(np.float32).max)
    blocks = {
        "zeros": ([0.0, -0.0] * 16, 0),
        "nonfinite": ([float("nan"), float("inf"), float("-inf"), float("nan")]
                      * 8, 0),
        "subnormal": ([2.0 ** -140] + [0.0] * 31, 0),
        "largest": ([1.0] * 31 + [-big], 254 - emax),
        "448": ([448.0] + [1.0] * 31, 127 + 8 - emax),
        "480": ([1.0] * 5 + [-480.0] + [1.0] * 26, 127 + 8 - emax),
        "6": ([6.0] + [0.0] * 31, 127 + 2 - emax),
        "7": ([0.0] * 31 + [7.0], 127 + 2 - emax),
        "skips": ([float("inf"), 3.0, float("nan")] + [0.5] * 29,
                  127 + 1 - emax if emax == 2 else 120),
    }
    x = torch.tensor(sum((v for v, _ in blocks.values()), []),
                     dtype=torch.float32)
    got = host_scales(x, stored)
    exp = [max(s, 0) for _, s in blocks.values()]
    assert list(got) == exp
    assert np.array_equal(ref_scales(widen(x), stored), got)   # the reference
    assert 255 not in got


@pytest.mark.parametrize("src", SOURCES)
def test_scales_strided_view(src):
    """rows of 64 inside rows of 96: the gaps hold larger values"""
    rng = np.random.default_rng(52)
    w = random_weights(rng, src, (7, 96))
    w[:, 64:] = 30000.0
    v = w[:, :64]
    for stored in ("F8_E4M3", "F4"):
        got = host_scales(w, stored, 7, 64, 96)
        assert np.array_equal(got, ref_scales(widen(v), stored).reshape(-1))


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("stored", ["F8_E4M3", "F4"])
def test_convert_host_both_ways(src, stored):
    """mx_convert_host, pieces starting mid-block included, and the
    exactness of f32-subnormal sources and subnormal results"""
    rng = np.random.default_rng(53)
    x = random_weights(rng, src, (32 * 40,))
    if src == "F32":
        x[:32] = torch.from_numpy(
            rng.integers(1, 1 << 23, 32).astype(np.uint32).view(np.float32))
    x[40], x[41], x[42], x[43] = float("nan"), float("inf"), -0.0, \
        float("-inf")
    x64 = widen(x)
    s = ref_scales(x64, stored)
    se = per_element(s, x64.shape)
    codes = ref_quant(x64, se, stored)
    for e0, n in ((0, x.numel()), (8, 50), (16, 34), (40, 600)):
        raw = x[e0:e0 + n].contiguous().view(torch.uint8).numpy()
        got = native.mx_convert_host(raw, D[src], D[stored], n, s, e0)
        assert got == pack(codes[e0:e0 + n], stored), (e0, n)
    rs = rng.integers(0, 256, s.size).astype(np.uint8)     # any scale byte
    rs[:3] = (0, 254, 255)
    rse = per_element(rs, x64.shape)
    for dst in SOURCES:
        for e0, n in ((0, x.numel()), (16, 34), (40, 600)):
            got = native.mx_convert_host(
                pack(codes[e0:e0 + n], stored), D[stored], D[dst], n, rs, e0)
            exp = ref_dequant(codes[e0:e0 + n], rse[e0:e0 + n], stored,
                              TDT[dst])
            assert_bits_equal(
                torch.frombuffer(bytearray(got), dtype=TDT[dst]), exp,
                count_nan(codes[e0:e0 + n], rse[e0:e0 + n], stored))


def test_support_tables_and_old_codes(arena):
    assert native.DTYPE_ITEMSIZE["F8_E8M0"] == 1
    assert native.DTYPE_BITS["F4"] == 4 and "F4" not in native.DTYPE_ITEMSIZE
    assert native.mx_quantize_supported("BF16", "F4")
    assert native.mx_dequantize_supported("F8_E4M3", "F16")
    assert not native.mx_quantize_supported("F64", "F4")
    assert not native.mx_dequantize_supported("F4", "F64")
    assert not native.quantize_supported("F4")
    assert not native.convert_supported("F4", "F32")
    x = torch.ones(64)
    for code in (15, D["F8_E8M0"], D["F4"]):     # stay refused there
        with pytest.raises(ValueError):
            arena.store_ptr([(x.data_ptr(), 0, 1, 64, 256, D["F32"], code)])
        with pytest.raises(ValueError):
            arena.convert_ptr([(0, x.data_ptr(), 1, 64, 64, code, D["F32"])])


def test_native_rejects(arena):
    x = torch.ones(64)
    s = torch.zeros(8, dtype=torch.uint8)
    p, q = x.data_ptr(), s.data_ptr()
    arena.fill(0, 4096, SENTINEL)
    f32, f4, e4 = D["F32"], D["F4"], D["F8_E4M3"]
    for seg in [(p, 0, 1, 64, 256, D["I32"], e4, q, 0, 64, 32),
                (p, 0, 1, 64, 256, f32, D["F8_E5M2"], q, 0, 64, 32),
                (p, 0, 1, 64, 256, f32, e4, 0, 0, 64, 32),
                (p, 0, 1, 64, 256, f32, e4, q, 0, 64, 16),
                (0, 0, 1, 64, 256, f32, e4, q, 0, 64, 32),
                (p + 2, 0, 1, 32, 256, f32, e4, q, 0, 64, 32),
                (p, 4 * MiB - 8, 1, 64, 256, f32, e4, q, 0, 64, 32),
                (p, 0, 1, 63, 256, f32, f4, q, 0, 64, 32),
                (p, 0, 1, 32, 256, f32, f4, q, 1, 64, 32),
                (p, 0, 2, 32, 64, f32, e4, q, 0, 32, 32)]:   # rows overlap
        with pytest.raises(ValueError):
            arena.store_ptr([(p, 64, 1, 64, 256, f32, e4, q, 0, 64, 32), seg])
    assert arena.read_bytes(0, 4096) == bytes([SENTINEL]) * 4096
    for seg in [(0, p, 1, 64, 64, e4, D["F64"], q, 0, 64, 32),
                (0, p + 2, 1, 32, 32, e4, f32, q, 0, 64, 32),
                (4 * MiB - 8, p, 1, 64, 64, e4, f32, q, 0, 64, 32),
                (0, p, 1, 33, 33, f4, f32, q, 0, 64, 32)]:
        with pytest.raises(ValueError):
            arena.convert_ptr([seg])
    for seg in [(p, 1, 48, 256, f32, e4, q), (p, 1, 64, 256, D["U8"], e4, q),
                (p, 1, 64, 256, f32, D["F32"], q), (p, 1, 64, 256, f32, e4, 0)]:
        with pytest.raises(ValueError):
            native.mx_scales(-1, [seg])


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("mode", MODES)
def test_host_arena_store_and_load(arena, src, mode):
    """the MEM tier's route: pieces at odd arena offsets that start
    mid-block, strided rows, then the sharded load"""
    stored = STORED[mode]
    rng = np.random.default_rng(54)
    w = random_weights(rng, src, (6, 96))
    v = w[:, :64]
    x64 = widen(v)
    s = ref_scales(x64, stored)
    codes = ref_quant(x64, per_element(s, x64.shape), stored)
    sc = torch.from_numpy(s.copy())
    bpe = 2 if stored == "F4" else 1             # elements per byte
    ss = w.element_size()
    arena.fill(0, 8192, SENTINEL)
    # whole rows from row 1, and the tail of row 0 from element 24
    arena.store_ptr([
        (w[1].data_ptr(), 4099, 5, 64, 96 * ss, D[src], D[stored],
         sc.data_ptr(), 64, 64, 32),
        (w[0, 24:].data_ptr(), 2051, 1, 40, 0, D[src], D[stored],
         sc.data_ptr(), 24, 40, 32)])
    n = 5 * 64 // bpe
    got = arena.read_bytes(4099 - 16, n + 32)
    assert got[16:-16] == pack(codes[1:], stored)
    assert got[:16] == got[-16:] == bytes([SENTINEL]) * 16
    got = arena.read_bytes(2051 - 16, 40 // bpe + 32)
    assert got[16:-16] == pack(codes[0, 24:], stored)
    assert got[:16] == got[-16:] == bytes([SENTINEL]) * 16
    # load: the whole tensor, a column shard, a piece from element 40
    arena.write(1027, pack(codes, stored))
    for dst in SOURCES:
        full = ref_dequant(codes, per_element(s, codes.shape), stored,
                           TDT[dst])
        out = torch.zeros((6, 64), dtype=TDT[dst])
        arena.convert_ptr([(1027, out.data_ptr(), 1, 384, 384 // bpe,
                            D[stored], D[dst], sc.data_ptr(), 0, 384, 32)])
        assert_bits_equal(out, full, 0)
        out = torch.zeros((6, 32), dtype=TDT[dst])
        arena.convert_ptr([(1027 + 32 // bpe, out.data_ptr(), 6, 32,
                            64 // bpe, D[stored], D[dst], sc.data_ptr(), 32,
                            64, 32)])
        assert_bits_equal(out, full[:, 32:].contiguous(), 0)
        out = torch.zeros(100, dtype=TDT[dst])
        arena.convert_ptr([(1027 + 40 // bpe, out.data_ptr(), 1, 100,
                            100 // bpe, D[stored], D[dst], sc.data_ptr(), 40,
                            100, 32)])
        assert_bits_equal(out, full.reshape(-1)[40:140], 0)


# ------------------------------------------------------------------ header

def test_parse_header_mx_dtypes():
    def parse(doc, n_data):
        js = json.dumps(doc).encode()
        blob = raw_header(js, b"\0" * n_data)
        return parse_header(blob[:8], lambda o, n: blob[o:o + n], len(blob))
    infos, _, _ = parse({"w": {"dtype": "F4", "shape": [2, 16],
                               "data_offsets": [0, 16]},
                         "s": {"dtype": "F8_E8M0", "shape": [2, 1],
                               "data_offsets": [16, 18]}}, 18)
    assert infos["w"].shape == (2, 16) and infos["w"].nbytes == 16
    assert infos["s"].dtype == "F8_E8M0"
    for shape, nbytes in (([2, 15], 15), ([2, 16], 32), ([2, 16], 15), ([], 1)):
        with pytest.raises(err.InvalidArgument):
            parse({"w": {"dtype": "F4", "shape": shape,
                         "data_offsets": [0, nbytes]}}, 64)
    with pytest.raises(err.InvalidArgument):
        parse({"w": {"dtype": "F6", "shape": [4], "data_offsets": [0, 3]}}, 8)


# ------------------------------------------------------------------- save

@pytest.mark.parametrize("mode", MODES)
def test_save_mem_tier(fsx, model, mode):
    smc, sf = fsx
    blob, start, ent, order = expected_mx_file(model, mode, {"format": "pt"})
    path = f"/mx/{mode}.safetensors"
    st = save_file(sf, model, path, metadata={"format": "pt"},
                   storage_tier="MEM", block_size=8192, quantize=mode)
    assert st.length == len(blob) and len(blob) > 2 * 8192
    check_file(smc, sf, path, blob)
    got = sf.read_file(path)
    (n,) = struct.unpack("<Q", got[:8])
    doc = json.loads(got[8:8 + n])
    for name in ("a", "b", "h", "cols"):
        shape = list(model[name].shape)
        assert doc[name]["dtype"] == STORED[mode]
        assert doc[name]["shape"] == shape
        assert doc[name + "_scale"]["dtype"] == "F8_E8M0"
        assert doc[name + "_scale"]["shape"] == shape[:-1] + [shape[-1] // 32]
    for name in ("bias", "odd", "ids"):           # not selected: as ever
        assert doc[name]["dtype"] in ("F32", "I64")
        assert name + "_scale" not in doc
    assert [k for k in doc if k != "__metadata__"] == order
    if mode == "mxfp4":                            # half a byte sorts last
        assert order[-4:] == ["a", "b", "cols", "h"]


@pytest.mark.parametrize("mode", MODES)
def test_save_cut_mid_block_equals_uncut(fsx, model, mode):
    """block_size 4112: with the data section on a multiple of 64 the
    cuts land 16 elements into an MX block"""
    smc, sf = fsx
    blob, start, _, _ = expected_mx_file(model, mode)
    assert start % 64 == 0 and len(blob) > 4 * 4112
    path = f"/mx/cut-{mode}.safetensors"
    save_file(sf, model, path, storage_tier="MEM", block_size=4112,
              quantize=mode)
    check_file(smc, sf, path, blob)


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
    for mode in MODES:
        path = f"/mx/{how}-{mode}.safetensors"
        save_file(sf, model, path, block_size=4112, quantize=mode, **kw)
        assert calls == []                        # no typed store
        check_file(smc, sf, path, expected_mx_file(model, mode)[0])


def test_save_filter_and_views(fsx):
    smc, sf = fsx
    rng = np.random.default_rng(55)
    w = random_weights(rng, "BF16", (12, 6, 64))
    tens = {"t": random_weights(rng, "F32", (64, 9)).t(),   # temporary
            "inner": w[:, :, 32:],      # rows of 32 inside rows of 64
            "rows": w[3:9],
            "vec": random_weights(rng, "F16", (64,)),
            "keep": random_weights(rng, "F32", (4, 32))}

    def pick(name, t):
        return name != "keep"
    for mode in MODES:
        blob = expected_mx_file(tens, mode, select=pick)[0]
        path = f"/mx/filter-{mode}.safetensors"
        save_file(sf, tens, path, storage_tier="MEM", block_size=512,
                  quantize=mode, quantize_filter=pick)
        check_file(smc, sf, path, blob)


# ------------------------------------------------------------------- load

@pytest.mark.parametrize("dst", SOURCES)
@pytest.mark.parametrize("mode", MODES)
def test_load_dequantize(fsx, model, mode, dst):
    _, sf = fsx
    dt, stored = TDT[dst], STORED[mode]
    path = f"/mx/load-{mode}-{dst}.safetensors"
    save_file(sf, model, path, storage_tier="MEM", block_size=4112,
              quantize=mode)
    ent = expected_mx_file(model, mode)[2]

    def ref(name):
        codes = ent[name][3]
        return ref_dequant(codes, per_element(ent[name + "_scale"][3],
                                              codes.shape), stored, dt)
    out = load_file(sf, path, device="cpu", dtype=dt, dequantize=True)
    assert set(out) == set(model)                 # no _scale entries
    for name in ("a", "b", "h", "cols"):
        assert_bits_equal(out[name], ref(name), 0)
    assert_bits_equal(out["bias"], model["bias"].to(dt), 0)
    assert_bits_equal(out["ids"], model["ids"], 0)
    with CurvineSafetensors(sf, path) as f:
        got = f.load(device="cpu", names=["a", "a_scale"], dequantize=True)
        assert got["a"].dtype == torch.float32    # dtype None: F32
        assert got["a_scale"].dtype == torch.float8_e8m0fnu
        assert got["a_scale"].view(torch.uint8).numpy().tobytes() == \
            ent["a_scale"][2]
        into = torch.zeros(model["h"].shape, dtype=dt)
        f.load_into("h", into, dequantize=True)
        assert_bits_equal(into, ref("h"), 0)
        full = ref("b")
        for r in range(2):
            t = f.get_tensor("b", device="cpu", dtype=dt, shard=(0, r, 2),
                             dequantize=True)
            assert_bits_equal(t, full[r * 65:(r + 1) * 65], 0)
            t = f.get_tensor("b", device="cpu", dtype=dt, shard=(-1, r, 2),
                             dequantize=True)
            assert_bits_equal(t, full[:, r * 128:(r + 1) * 128].contiguous(),
                              0)
        t = f.get_tensor("h", device="cpu", dtype=dt, shard=(1, 3, 4),
                         dequantize=True)
        assert_bits_equal(t, ref("h")[:, 3:4].contiguous(), 0)
        with pytest.raises(err.Unsupported):      # parts of 16 cut blocks
            f.get_tensor("h", device="cpu", shard=(2, 0, 2), dequantize=True)
        with pytest.raises(err.Unsupported):
            f.get_tensor("b", device="cpu", dtype=torch.float64,
                         dequantize=True)


@pytest.mark.parametrize("mode", MODES)
def test_raw_load_and_resave_round_trip(fsx, model, mode):
    smc, sf = fsx
    blob, _, ent, _ = expected_mx_file(model, mode)
    path = f"/mx/raw-{mode}.safetensors"
    save_file(sf, model, path, storage_tier="MEM", quantize=mode)
    raw = load_file(sf, path, device="cpu")
    assert set(raw) == set(ent)
    el = torch.float8_e4m3fn if mode == "mxfp8" else torch.float4_e2m1fn_x2
    for name in ("a", "b", "h", "cols"):
        shape = list(model[name].shape)
        assert raw[name + "_scale"].dtype == torch.float8_e8m0fnu
        assert raw[name].dtype == el
        if mode == "mxfp4":
            shape[-1] //= 2
        assert list(raw[name].shape) == shape
        assert raw[name].view(torch.uint8).numpy().tobytes() == ent[name][2]
    save_file(sf, raw, f"/mx/resaved-{mode}.safetensors", storage_tier="MEM",
              block_size=4112)
    check_file(smc, sf, f"/mx/resaved-{mode}.safetensors", blob)
    with CurvineSafetensors(sf, path) as f:
        t = f.get_tensor("b", device="cpu", shard=(1, 1, 2))
        cols = 128 if mode == "mxfp8" else 64
        assert t.view(torch.uint8).numpy().tobytes() == \
            raw["b"].view(torch.uint8)[:, cols:].contiguous().numpy().tobytes()
    if mode == "mxfp4":
        # a last-dimension shard of raw F4 needs an even part
        save_file(sf, {"w": raw["a"].view(torch.uint8)[:, :3].contiguous()
                       .view(torch.float4_e2m1fn_x2)},
                  "/mx/six.safetensors", storage_tier="MEM")
        with CurvineSafetensors(sf, "/mx/six.safetensors") as f:
            assert f.info("w").shape == (5, 6) and f.info("w").dtype == "F4"
            assert f.get_tensor("w", device="cpu", shard=(1, 0, 3)).shape == \
                (5, 1)
            with pytest.raises(err.Unsupported):
                f.get_tensor("w", device="cpu", shard=(1, 0, 2))


def test_scale_of_another_shape_is_no_mx_scale(fsx):
    _, sf = fsx
    q = torch.arange(64, dtype=torch.uint8).view(torch.float8_e4m3fn) \
        .reshape(2, 32)
    s = torch.full((1, 2), 127, dtype=torch.uint8).view(torch.float8_e8m0fnu)
    save_file(sf, {"q": q, "q_scale": s}, "/mx/wrong.safetensors",
              storage_tier="MEM")
    out = load_file(sf, "/mx/wrong.safetensors", device="cpu",
                    dtype=torch.bfloat16, dequantize=True)
    assert set(out) == {"q", "q_scale"}
    assert_bits_equal(out["q"], q.to(torch.bfloat16), 0)


# --------------------------------------------------------------- refusals

def test_refused_before_create(fsx):
    _, sf = fsx
    w = torch.ones((4, 64))

    def every(n, t):
        return True
    cases = [
        (dict(tensors={"w": w}, quantize="block"), err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="mxfp6"), err.InvalidArgument),
        (dict(tensors={"w": w, "w_scale": torch.ones(1)}, quantize="mxfp8"),
         err.InvalidArgument),
        (dict(tensors={"w": torch.ones((4, 48))}, quantize="mxfp4",
              quantize_filter=every), err.InvalidArgument),
        (dict(tensors={"w": torch.tensor(1.0)}, quantize="mxfp8",
              quantize_filter=every), err.InvalidArgument),
        (dict(tensors={"w": w.double()}, quantize="mxfp8",
              quantize_filter=every), err.Unsupported),
        (dict(tensors={"w": w.to(torch.int32)}, quantize="mxfp4",
              quantize_filter=every), err.Unsupported),
        (dict(tensors={"w": w.to(torch.float8_e4m3fn)}, quantize="mxfp8",
              quantize_filter=every), err.Unsupported),
        (dict(tensors={"w": w}, dtype=torch.float4_e2m1fn_x2),
         err.Unsupported),
    ]
    for i, (kw, exc) in enumerate(cases):
        path = f"/mx/refused{i}.safetensors"
        tensors = kw.pop("tensors")
        with pytest.raises(exc):
            save_file(sf, tensors, path, storage_tier="MEM", **kw)
        assert not sf.exists(path), i
    # not a multiple of 32 and not forced: saved unquantised
    save_file(sf, {"w": torch.ones((4, 48))}, "/mx/plain.safetensors",
              storage_tier="MEM", quantize="mxfp4")
    with CurvineSafetensors(sf, "/mx/plain.safetensors") as f:
        assert f.keys() == ["w"] and f.info("w").dtype == "F32"
