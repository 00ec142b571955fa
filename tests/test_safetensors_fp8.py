"""FP8 (E4M3) safetensors on the CPU: the saturating cast and the scale
rule through the host twins of the kernels (convert_host, absmax_scales on
device -1, store_ptr / convert_ptr of a host arena), then
save_file(quantize=...) of cpu tensors into the MEM tier, the byte path,
load(dequantize=True) and the refusals.  Every expected value is the torch
CPU reference of safetensors_fp8_cases; comparisons are bitwise."""
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

from safetensors_cases import ISZ, TORCH, assert_bits_equal, from_raw
from safetensors_fp8_cases import (F8, SOURCES, expected_fp8_file,
                                   flat_dequant, flat_quant, flat_scales,
                                   random_weights, ref_dequant, ref_quant,
                                   ref_scales)
from safetensors_save_cases import check_file, expected_file

D = native.DTYPES
MiB = 1 << 20
SENTINEL = 0xAB
ONE = np.ones(1, dtype=np.float32)


@pytest.fixture(scope="module")
def fsx(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("stfp8"))
    conf = make_conf(tmp)
    smc = SyncMiniCluster(conf=conf, tmp_dir=tmp, workers=2).start()
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
    rng = np.random.default_rng(31)
    w = random_weights(rng, "F32", (9, 80))
    return {"a": random_weights(rng, "F32", (5, 67)),
            "b": random_weights(rng, "BF16", (130, 256)),
            "h": random_weights(rng, "F16", (3, 4, 8)),
            "cols": w[:, 3:70],
            "bias": random_weights(rng, "F32", (67,)),
            "ids": torch.arange(33, dtype=torch.int64),
            "none": torch.empty((0, 4), dtype=torch.float32)}


def host_scales(t, every, n_groups, e0=0):
    """absmax_scales on the host for a contiguous or row-strided 2-D cpu
    tensor"""
    out = torch.full((n_groups,), 7.0, dtype=torch.float32)
    if t.ndim == 2 and t.stride(0) != t.shape[1]:
        rows, run, pitch = t.shape[0], t.shape[1], t.stride(0)
    else:
        rows, run, pitch = 1, t.numel(), t.numel()
    dt = {v: k for k, v in TORCH.items()}[t.dtype]
    native.absmax_scales(-1, [(t.data_ptr(), rows, run, pitch * ISZ[dt],
                               D[dt], out.data_ptr(), every, e0, n_groups)])
    return out


# ---------------------------------------------------------- the cast rule

def test_cast_rule_fixed_values():
    vals = [0.0, -0.0, 2.0 ** -10, 2.0 ** -10 * (1 + 2.0 ** -20),
            1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 447.9, 448.0, 464.0, 465.0,
            1e9, float("inf"), float("-inf"), float("nan")]
    x = torch.tensor(vals + [-v for v in vals], dtype=torch.float32)
    got = from_raw(native.convert_host(x.numpy(), D["F32"], D["F8_E4M3"],
                                       x.numel(), scales=ONE), "F8_E4M3")
    assert_bits_equal(got, x.clamp(-448, 448).to(F8), 2)
    b = got.view(torch.uint8).tolist()
    # 2^-10 ties to 0, just above it is the smallest subnormal, 1.5 and 2.5
    # units tie to even, >= 448 and inf saturate, NaN keeps its place
    assert b[:13] == [0, 0x80, 0, 1, 2, 2, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E,
                      0x7E, 0xFE]
    assert b[13] & 0x7F == 0x7F


def test_cast_rule_random_patterns():
    rng = np.random.default_rng(7)
    n = 1 << 20
    bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | \
        (rng.integers(110, 140, n).astype(np.uint32) << 23) | \
        rng.integers(0, 1 << 23, n).astype(np.uint32)
    x = torch.from_numpy(bits.view(np.float32))
    got = from_raw(native.convert_host(bits, D["F32"], D["F8_E4M3"], n,
                                       scales=ONE), "F8_E4M3")
    assert_bits_equal(got, x.clamp(-448, 448).to(F8), 0)


@pytest.mark.parametrize("src", SOURCES)
def test_convert_host_scaled_both_ways(src):
    rng = np.random.default_rng(8)
    x = random_weights(rng, src, (1000,))
    scales, idx = flat_scales(x, 67, 139)
    q = from_raw(native.convert_host(
        x.view(torch.uint8).numpy(), D[src], D["F8_E4M3"], 1000,
        scales=scales.numpy(), scale_every=67, scale_e0=139), "F8_E4M3")
    assert_bits_equal(q, flat_quant(x, scales, idx), 0)
    y = from_raw(native.convert_host(
        q.view(torch.uint8).numpy(), D["F8_E4M3"], D[src], 1000,
        scales=scales.numpy(), scale_every=67, scale_e0=139), src)
    assert_bits_equal(y, flat_dequant(q, scales, idx, TORCH[src]), 0)
    with pytest.raises(ValueError):          # groups pass the scales given
        native.convert_host(x.view(torch.uint8).numpy(), D[src],
                            D["F8_E4M3"], 1000, scales=scales.numpy()[:5],
                            scale_every=67, scale_e0=139)
    with pytest.raises(ValueError):          # no unscaled fp8 downcast
        native.convert_host(x.view(torch.uint8).numpy(), D[src],
                            D["F8_E4M3"], 1000)
    with pytest.raises(ValueError):          # a scale on a plain cast
        native.convert_host(x.view(torch.uint8).numpy(), D[src], D["F32"],
                            1000, scales=ONE)


def test_support_tables():
    assert [native.quantize_supported(s) for s in
            ("F32", "F16", "BF16", "F64", "F8_E4M3", "I8")] == \
        [True, True, True, False, False, False]
    assert [native.dequantize_supported(d) for d in
            ("F32", "F16", "BF16", "F64", "F8_E5M2")] == \
        [True, True, True, False, False]
    assert not native.convert_supported("F32", "F8_E4M3")   # as before


# --------------------------------------------------------- the scale rule

FLOOR = torch.tensor([2.0 ** -40]) / 448


@pytest.mark.parametrize("src", SOURCES)
def test_scale_rule(src):
    dt = TORCH[src]
    zero = torch.zeros(100, dtype=dt)
    zero[3] = -0.0
    assert_bits_equal(host_scales(zero, 0, 1), FLOOR, 0)
    bad = torch.tensor([float("inf"), float("nan"), float("-inf")] * 9,
                       dtype=dt)
    assert_bits_equal(host_scales(bad, 0, 1), FLOOR, 0)
    mixed = torch.tensor([float("inf"), 3.0, float("nan"), -5.0], dtype=dt)
    assert_bits_equal(host_scales(mixed, 0, 1), ref_scales(mixed, "tensor"), 0)
    # the maximum at the last element of a strided view, larger values in
    # the gaps of the storage
    w = torch.ones((6, 20), dtype=dt)
    w[:, 17:] = 30000.0
    v = w[:, 2:17]
    v[5, 14] = -9.0
    assert_bits_equal(host_scales(v, 0, 1), ref_scales(v, "tensor"), 0)
    assert_bits_equal(host_scales(v, 15, 6).reshape(6, 1),
                      ref_scales(v, "row"), 0)
    # an amax below the floor
    tiny = torch.tensor([2.0 ** -41, -(2.0 ** -60), 0.0], dtype=torch.float32)
    if src == "F32":
        assert_bits_equal(host_scales(tiny, 0, 1), FLOOR, 0)
    # groups counted from the tensor's start: a piece beginning mid-tensor
    rng = np.random.default_rng(9)
    x = random_weights(rng, src, (500,))
    exp, _ = flat_scales(x, 67, 139)
    got = host_scales(x, 67, exp.numel(), 139)
    assert_bits_equal(got, exp, 0)


def test_absmax_rejects():
    x = torch.ones(64, dtype=torch.float32)
    out = torch.full((4,), 7.0)
    p, o = x.data_ptr(), out.data_ptr()
    bad = [
        (p, 1, 64, 256, D["F8_E4M3"], o, 0, 0, 1),      # not a source dtype
        (p, 1, 64, 256, D["I32"], o, 0, 0, 1),
        (0, 1, 64, 256, D["F32"], o, 0, 0, 1),          # null source
        (p + 2, 1, 64, 256, D["F32"], o, 0, 0, 1),      # misaligned source
        (p, 1, 64, 256, D["F32"], 0, 0, 0, 1),          # null out
        (p, 1, 64, 256, D["F32"], o + 2, 0, 0, 1),      # misaligned out
        (p, 1, 64, 256, D["F32"], o, 0, 0, 0),          # no slots
        (p, 1, 64, 256, D["F32"], o, 16, 0, 3),         # 4 groups, 3 slots
        (p, 1, 64, 256, D["F32"], o, 16, 1, 4),         # e0 pushes a 5th
        (p, 1 << 62, 8, 32, D["F32"], o, 0, 0, 1),      # rows*run wraps
        (p, 3, 1, (1 << 64) - 1, D["F32"], o, 0, 0, 1),  # rows*pitch wraps
    ]
    good = (p, 1, 64, 256, D["F32"], o, 16, 0, 4)
    for seg in bad:
        with pytest.raises(ValueError):
            native.absmax_scales(-1, [good, seg])   # whole call refused
    assert (out == 7.0).all()
    native.absmax_scales(-1, [])
    native.absmax_scales(-1, [good, (p, 1, 32, 128, D["F32"], o, 16, 0, 2)])
    assert (out == 1.0 / 448).all()                 # shared slots: once


# ------------------------------------------------- host arena store / load

@pytest.mark.parametrize("src", SOURCES)
def test_host_arena_store_and_load(arena, src):
    rng = np.random.default_rng(10)
    ss = ISZ[src]
    x = random_weights(rng, src, (700,))
    e0 = 67 * 2 + 5
    scales, idx = flat_scales(x, 67, e0)
    exp_q = flat_quant(x, scales, idx)
    arena.fill(0, 64 << 10, SENTINEL)
    off = 4099
    arena.store_ptr([(x.data_ptr(), off, 1, 700, 700 * ss, D[src],
                      D["F8_E4M3"], scales.data_ptr(), 67, e0)])
    assert_bits_equal(from_raw(arena.read_bytes(off, 700), "F8_E4M3"),
                      exp_q, 0)
    assert arena.read_bytes(off - 16, 16) == bytes([SENTINEL]) * 16
    assert arena.read_bytes(off + 700, 16) == bytes([SENTINEL]) * 16
    out = torch.zeros(700, dtype=TORCH[src])
    arena.convert_ptr([(off, out.data_ptr(), 1, 700, 700, D["F8_E4M3"],
                        D[src], scales.data_ptr(), 67, e0)])
    assert_bits_equal(out, flat_dequant(exp_q, scales, idx, TORCH[src]), 0)
    # the unscaled upcast is what it was
    arena.convert_ptr([(off, out.data_ptr(), 1, 700, 700, D["F8_E4M3"],
                        D[src])])
    assert_bits_equal(out, exp_q.to(TORCH[src]), 0)
    p, s = x.data_ptr(), scales.data_ptr()
    for seg in [(p, 0, 1, 8, 8 * ss, D[src], D["F8_E4M3"], 0, 0, 0),
                (p, 0, 1, 8, 8 * ss, D[src], D["F8_E4M3"], s + 2, 0, 0),
                (p, 0, 1, 8, 8 * ss, D[src], D["F8_E5M2"], s, 0, 0),
                (p, 0, 1, 8, 8 * ss, D[src], D[src], s, 0, 0),
                (p, 0, 1, 8, 8 * ss, D[src], D["F8_E4M3"], s, 0),
                (p, 0, 1, 8, 8, D["F8_E4M3"], D["F32"], s, 0, 0)]:
        with pytest.raises((ValueError, TypeError)):
            arena.store_ptr([seg])
    for seg in [(0, out.data_ptr(), 1, 8, 8 * ss, D[src], D["F8_E4M3"],
                 s, 0, 0),
                (0, out.data_ptr(), 1, 8, 8, D["F8_E5M2"], D["F32"], s, 0, 0),
                (0, out.data_ptr(), 1, 8, 8, D["F8_E4M3"], D["F32"],
                 s + 1, 0, 0)]:
        with pytest.raises(ValueError):
            arena.convert_ptr([seg])


# ------------------------------------------------------------------- save

@pytest.mark.parametrize("mode", ["tensor", "row"])
def test_save_mem_tier(fsx, model, mode):
    smc, sf = fsx
    blob, start, stored, order = expected_fp8_file(model, mode,
                                                   {"format": "pt"})
    path = f"/q/{mode}.safetensors"
    st = save_file(sf, model, path, metadata={"format": "pt"},
                   storage_tier="MEM", block_size=8192, quantize=mode)
    assert st.length == len(blob) and len(blob) > 3 * 8192
    check_file(smc, sf, path, blob)
    got = sf.read_file(path)
    (n,) = struct.unpack("<Q", got[:8])
    doc = json.loads(got[8:8 + n])
    for name in ("a", "b", "h", "cols"):
        assert doc[name]["dtype"] == "F8_E4M3"
        assert doc[name]["shape"] == list(model[name].shape)
        rows = model[name].shape[0]
        assert doc[name + "_scale"]["dtype"] == "F32"
        assert doc[name + "_scale"]["shape"] == \
            ([1] if mode == "tensor" else [rows, 1])
    for name in ("bias", "ids", "none"):          # not selected: as ever
        assert doc[name]["dtype"] == {"bias": "F32", "ids": "I64",
                                      "none": "F32"}[name]
        assert name + "_scale" not in doc
    assert list(k for k in doc if k != "__metadata__") == order


@pytest.mark.parametrize("how", ["file_tier", "replicas"])
def test_save_byte_path_identical(fsx, model, how, monkeypatch):
    smc, sf = fsx
    calls = []
    orig = native.Arena.store_ptr
    monkeypatch.setattr(native.Arena, "store_ptr",
                        lambda self, segs: (calls.append(segs),
                                            orig(self, segs))[1])
    blob = expected_fp8_file(model, "row")[0]
    kw = {"storage_tier": "SSD"} if how == "file_tier" else \
        {"storage_tier": "MEM", "replicas": 2}
    path = f"/q/{how}.safetensors"
    save_file(sf, model, path, block_size=8192, quantize="row", **kw)
    assert calls == []                            # no typed store
    check_file(smc, sf, path, blob)


def test_save_filter_dtype_and_views(fsx):
    smc, sf = fsx
    rng = np.random.default_rng(12)
    w = random_weights(rng, "BF16", (12, 6, 10))
    tens = {"t": random_weights(rng, "F32", (20, 9)).t(),   # temporary
            "inner": w[:, :, 2:9],      # collapses to rows of 7: groups of 42
            "rows": w[3:9],
            "vec": random_weights(rng, "F16", (40,)),
            "keep": random_weights(rng, "F32", (4, 4))}

    def pick(name, t):
        return name != "keep"
    for mode in ("tensor", "row"):
        # "keep" is not selected and takes the dtype= cast as before
        stored = {}
        for k, t in tens.items():
            if pick(k, t):
                s = ref_scales(t, mode)
                stored[k], stored[k + "_scale"] = ref_quant(t, s), s
            else:
                stored[k] = t.to(torch.bfloat16)
        blob = expected_file(stored)[0]
        path = f"/q/filter-{mode}.safetensors"
        save_file(sf, tens, path, dtype=torch.bfloat16, storage_tier="MEM",
                  block_size=512, quantize=mode, quantize_filter=pick)
        check_file(smc, sf, path, blob)


# ------------------------------------------------------------------- load

@pytest.mark.parametrize("dst", SOURCES)
def test_load_dequantize_round_trip(fsx, model, dst):
    _, sf = fsx
    dt = TORCH[dst]
    for mode in ("tensor", "row"):
        path = f"/q/load-{mode}-{dst}.safetensors"
        save_file(sf, model, path, storage_tier="MEM", block_size=8192,
                  quantize=mode)
        stored = expected_fp8_file(model, mode)[2]
        out = load_file(sf, path, device="cpu", dtype=dt, dequantize=True)
        assert set(out) == set(model)             # no _scale entries
        for name in ("a", "b", "h", "cols"):
            assert_bits_equal(out[name], ref_dequant(
                stored[name], stored[name + "_scale"], dt), 0)
        assert_bits_equal(out["bias"], model["bias"].to(dt), 0)
        assert_bits_equal(out["ids"], model["ids"], 0)
        with CurvineSafetensors(sf, path) as f:
            # dtype None: F32; an explicit name list may ask for a scale
            got = f.load(device="cpu", names=["a", "a_scale"],
                         dequantize=True)
            assert_bits_equal(got["a"], ref_dequant(
                stored["a"], stored["a_scale"], torch.float32), 0)
            assert_bits_equal(got["a_scale"], stored["a_scale"], 0)
            # without dequantize, and for fp8 without a scale: as before
            plain = f.load(device="cpu")
            assert set(plain) == set(stored)
            assert_bits_equal(plain["b"], stored["b"], 0)
            assert_bits_equal(f.get_tensor("b", device="cpu", dtype=dt),
                              stored["b"].to(dt), 0)
            into = torch.zeros(model["h"].shape, dtype=dt)
            f.load_into("h", into, dequantize=True)
            assert_bits_equal(into, ref_dequant(
                stored["h"], stored["h_scale"], dt), 0)
            if mode == "row":
                full = ref_dequant(stored["b"], stored["b_scale"], dt)
                for r in range(2):
                    t = f.get_tensor("b", device="cpu", dtype=dt,
                                     shard=(0, r, 2), dequantize=True)
                    assert_bits_equal(t, full[r * 65:(r + 1) * 65], 0)
                    t = f.get_tensor("b", device="cpu", dtype=dt,
                                     shard=(1, r, 2), dequantize=True)
                    assert_bits_equal(
                        t, full[:, r * 128:(r + 1) * 128].contiguous(), 0)
                full = ref_dequant(stored["h"], stored["h_scale"], dt)
                t = f.get_tensor("h", device="cpu", dtype=dt,
                                 shard=(2, 1, 4), dequantize=True)
                assert_bits_equal(t, full[:, :, 2:4].contiguous(), 0)


def test_fp8_without_scale_loads_as_before(fsx):
    _, sf = fsx
    rng = np.random.default_rng(13)
    q = random_weights(rng, "F32", (6, 10), spread=False).to(F8)
    tens = {"q": q,                               # no scale at all
            "r": q.clone(), "r_scale": torch.ones(3),          # wrong numel
            "s": q.clone(), "s_scale": torch.ones(6).half()}   # not F32
    save_file(sf, tens, "/q/noscale.safetensors", storage_tier="MEM")
    out = load_file(sf, "/q/noscale.safetensors", device="cpu",
                    dtype=torch.bfloat16, dequantize=True)
    assert set(out) == set(tens)
    for name in ("q", "r", "s"):
        assert_bits_equal(out[name], q.to(torch.bfloat16), 0)
    out = load_file(sf, "/q/noscale.safetensors", device="cpu",
                    dequantize=True)
    assert out["q"].dtype == F8
    assert_bits_equal(out["q"], q, 0)


# --------------------------------------------------------------- refusals

def test_refused_before_create(fsx):
    _, sf = fsx
    w = torch.ones((4, 4))
    cases = [
        (dict(tensors={"w": w, "w_scale": torch.ones(1)}, quantize="tensor"),
         err.InvalidArgument),
        (dict(tensors={"w": w}, quantize="block"), err.InvalidArgument),
        (dict(tensors={"w": w}, quantize=True), err.InvalidArgument),
        (dict(tensors={"w": w.double()}, quantize="row",
              quantize_filter=lambda n, t: True), err.Unsupported),
        (dict(tensors={"w": w.to(torch.int32)}, quantize="tensor",
              quantize_filter=lambda n, t: True), err.Unsupported),
        (dict(tensors={"w": w.to(F8)}, quantize="tensor",
              quantize_filter=lambda n, t: True), err.Unsupported),
        # the plain dtype= downcast stays unsupported
        (dict(tensors={"w": w}, dtype=F8), err.Unsupported),
    ]
    for i, (kw, exc) in enumerate(cases):
        path = f"/q/refused{i}.safetensors"
        tensors = kw.pop("tensors")
        with pytest.raises(exc):
            save_file(sf, tensors, path, storage_tier="MEM", **kw)
        assert not sf.exists(path), i
    # a given "_scale" of a tensor that is not selected is no collision
    save_file(sf, {"b": torch.ones(4), "b_scale": torch.ones(1)},
              "/q/nocollision.safetensors", storage_tier="MEM",
              quantize="tensor")
    with CurvineSafetensors(sf, "/q/nocollision.safetensors") as f:
        assert f.info("b").dtype == "F32"
