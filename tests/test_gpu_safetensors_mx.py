"""mx_scales_kernel, mx_store_kernel and mx_load_kernel (csrc/mx_cast.hip)
on the MI355X, then save_file(quantize="mxfp8" | "mxfp4") and
load(dequantize=True) through the HBM tier.  Every expected value is the
float64 reference of safetensors_mx_cases; comparisons are bitwise, and
sentinel bytes stay on both sides of every destination."""
import numpy as np
import pytest
import torch

from curvine_amd import native
from curvine_amd.testing import test_conf as make_conf

from safetensors_cases import assert_bits_equal
from safetensors_mx_cases import (SOURCES, STORED, TABLE, TDT, count_nan,
                                  expected_mx_file, pack, per_element,
                                  random_weights, ref_dequant, ref_quant,
                                  ref_scales, widen)
from safetensors_save_cases import check_file

pytestmark = pytest.mark.gpu

D = native.DTYPES
MiB = 1 << 20
SENTINEL = 0xAB
FORMATS = ("F8_E4M3", "F4")
NP16 = {"F16": torch.float16, "BF16": torch.bfloat16}


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
    return {v: k for k, v in TDT.items()}[t.dtype]


def gpu_scales(dev, rows, run, pitch, stored):
    """E8M0 bytes of rows x run elements, sentinels checked on both sides"""
    n = rows * run // 32
    out = torch.full((n + 32,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    native.mx_scales(0, [(dev.data_ptr(), rows, run,
                          pitch * dev.element_size(), D[src_name(dev)],
                          D[stored], out.data_ptr() + 16)])
    got = out.cpu().numpy()
    assert (got[:16] == SENTINEL).all() and (got[-16:] == SENTINEL).all()
    return got[16:-16]


# ------------------------------------------------------------------ scales

@pytest.mark.parametrize("src", SOURCES)
def test_scales_maximum_at_every_position(src):
    """block i has its maximum at element i: every lane of the four that
    share a block, the lane boundaries 7/8, 15/16, 23/24 and the block
    edge 31/32"""
    x = torch.full((32, 32), 2.0 ** -12, dtype=TDT[src])
    for i in range(32):
        x[i, i] = -(2.0 ** (i // 2 - 6)) * 1.5
    for elem_off in (0, 1):          # vector loads; a source 1 element in
        dev = on_gpu(x, elem_off)
        for stored in FORMATS:
            got = gpu_scales(dev, 1, 1024, 1024, stored)
            assert np.array_equal(got, ref_scales(widen(x), stored)
                                  .reshape(-1)), (elem_off, stored)
            assert len(set(got)) >= 10


@pytest.mark.parametrize("src", SOURCES)
def test_scales_tiles_and_strided_rows(src):
    rng = np.random.default_rng(61)
    n = 2 * tile_elems() + 32
    x = random_weights(rng, src, (n,))
    x[5], x[77] = float("nan"), float("inf")
    for stored in FORMATS:
        assert np.array_equal(gpu_scales(on_gpu(x), 1, n, n, stored),
                              ref_scales(widen(x), stored))
    w = random_weights(rng, src, (7, 96))
    w[:, 64:] = 30000.0               # the gaps hold larger values
    dev = on_gpu(w, 1)
    for stored in FORMATS:
        got = gpu_scales(dev, 7, 64, 96, stored)
        assert np.array_equal(got, ref_scales(widen(w[:, :64]), stored)
                              .reshape(-1))


def test_scales_special_blocks_and_rejects():
    big = float(np.finfo(np.float32).max)
    x = torch.tensor([0.0, -0.0] * 16 + [float("nan"), float("inf")] * 16 +
                     [2.0 ** -140] + [0.0] * 31 + [1.0] * 31 + [-big] +
                     [448.0] + [1.0] * 31 + [1.0] * 5 + [-480.0] + [1.0] * 26
                     + [6.0] + [0.0] * 31 + [0.0] * 31 + [7.0],
                     dtype=torch.float32)
    dev = on_gpu(x)
    assert list(gpu_scales(dev, 1, 256, 256, "F8_E4M3")) == \
        [0, 0, 0, 246, 127, 127, 121, 121]
    assert list(gpu_scales(dev, 1, 256, 256, "F4")) == \
        [0, 0, 0, 252, 133, 133, 127, 127]
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    host, hout = torch.ones(64), torch.zeros(8, dtype=torch.uint8)
    torch.cuda.synchronize()
    p, o, f32, e4 = dev.data_ptr(), out.data_ptr(), D["F32"], D["F8_E4M3"]
    for seg in [(p, 1, 48, 256, f32, e4, o), (p, 1, 64, 256, D["I32"], e4, o),
                (p, 1, 64, 256, f32, D["F8_E5M2"], o), (0, 1, 64, 256, f32, e4, o),
                (p + 2, 1, 64, 256, f32, e4, o), (p, 1, 64, 256, f32, e4, 0),
                (p, 1, 1 << 28, 1 << 30, f32, e4, o),          # past alloc
                (host.data_ptr(), 1, 64, 256, f32, e4, o),
                (p, 1, 64, 256, f32, e4, hout.data_ptr())]:
        with pytest.raises(ValueError):
            native.mx_scales(0, [(p, 1, 64, 256, f32, e4, o), seg])
    assert (out.cpu() == SENTINEL).all()           # refused before launch


# ------------------------------------------------------------------- store

def store_and_check(arena, dev, x64, s, stored, pieces):
    """pieces: [(e0, n, dst_off)] of the flat tensor x64 whose E8M0 bytes
    are s; one call, then every piece and the bytes between them"""
    codes = ref_quant(x64, per_element(s, x64.shape), stored)
    dscale = torch.from_numpy(s.copy()).to("cuda:0")
    bpe = 2 if stored == "F4" else 1
    ss = dev.element_size()
    top = max(off + n // bpe for _, n, off in pieces) + 64
    arena.fill(0, top, SENTINEL)
    torch.cuda.synchronize()
    arena.store_ptr([(dev.data_ptr() + e0 * ss, off, 1, n, n * ss,
                      D[src_name(dev)], D[stored], dscale.data_ptr(), e0, n,
                      32) for e0, n, off in pieces])
    got = arena.read_bytes(0, top)
    prev = 0
    for e0, n, off in sorted(pieces, key=lambda p: p[2]):
        assert got[prev:off] == bytes([SENTINEL]) * (off - prev), (e0, n, off)
        assert off - prev >= 16
        exp = pack(codes[e0:e0 + n], stored)
        if got[off:off + len(exp)] != exp:
            g = np.frombuffer(got[off:off + len(exp)], dtype=np.uint8)
            bad = np.nonzero(g != np.frombuffer(exp, dtype=np.uint8))[0]
            raise AssertionError(
                f"piece e0={e0} n={n} at {off}: {bad.size} bytes differ, "
                f"first at {bad[0]}: got {g[bad[0]]:#x} expected "
                f"{exp[bad[0]]:#x}")
        prev = off + len(exp)
    assert got[prev:] == bytes([SENTINEL]) * (top - prev)


ANCHORS = {"F16": (1.0, 16384.0, 2.0 ** -14),
           "BF16": (1.0, 2.0 ** 60, 2.0 ** -60)}


@pytest.mark.parametrize("src", ["F16", "BF16"])
@pytest.mark.parametrize("stored", FORMATS)
@pytest.mark.parametrize("anchor", [0, 1, 2])
def test_store_every_16_bit_pattern(arena, src, stored, anchor):
    """all 65 536 patterns, one per block as element 0, beside an anchor
    that sets the scale: 1.0; a large one that puts the patterns in the
    subnormal range of the element format and below; a tiny one under
    which the pattern itself is the maximum and the upper ones saturate"""
    a = ANCHORS[src][anchor]
    raw = np.zeros((65536, 32), dtype=np.uint16)
    raw[:, 0] = np.arange(65536, dtype=np.uint16)
    x = torch.from_numpy(raw.view(np.int16)).view(NP16[src])
    x[:, 1] = a
    x[:, 2] = -a / 3
    x64 = widen(x).reshape(-1)
    s = ref_scales(x64, stored)
    store_and_check(arena, on_gpu(x), x64, s, stored, [(0, x64.size, 4096)])


@pytest.mark.parametrize("stored", FORMATS)
def test_store_f32_ties(arena, stored):
    """exact ties of the element grid and their f32 neighbours under scale
    2**0, both signs: the tie to zero, every midpoint, the last tie before
    saturation and the values around the maximum"""
    t = TABLE[stored][:127] if stored == "F8_E4M3" else TABLE[stored]
    top = t[-1]
    mids = np.concatenate([(t[:-1] + t[1:]) / 2, t,
                           [top + (top - t[-2]) / 2, top * 1.25, top * 64]])
    mids = mids.astype(np.float32)
    vals = np.concatenate([np.nextafter(mids, np.float32(0)), mids,
                           np.nextafter(mids, np.float32(np.inf))])
    vals = np.concatenate([vals, -vals,
                           np.array([np.inf, -np.inf, np.nan],
                                    dtype=np.float32)])
    # an anchor in every block: the largest finite element format value's
    # binade, so every block's scale byte is 127 whatever else it holds
    anchor = np.float32(256.0 if stored == "F8_E4M3" else 4.0)
    vals = vals[np.abs(np.nan_to_num(vals, posinf=0, neginf=0))
                < 2 * anchor]
    pad = -vals.size % 31
    vals = np.concatenate([vals, np.zeros(pad, dtype=np.float32)])
    x = np.concatenate([vals.reshape(-1, 31),
                        np.full((vals.size // 31, 1), anchor,
                                dtype=np.float32)], axis=1)
    xt = torch.from_numpy(x.copy())
    x64 = widen(xt).reshape(-1)
    s = ref_scales(x64, stored)
    assert (s == 127).all()
    store_and_check(arena, on_gpu(xt), x64, s, stored, [(0, x64.size, 4099)])


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("stored", FORMATS)
def test_store_offsets_and_mid_block_pieces(arena, src, stored):
    """destination offsets 0..7 x pieces that begin 8, 16 and 40 elements
    into the tensor with lengths that are no multiple of 32, a source one
    element into its storage, and more than two tiles"""
    rng = np.random.default_rng(62)
    n = 2 * tile_elems() + 32
    x = random_weights(rng, src, (n,))
    x[9], x[41] = float("nan"), float("-inf")
    x64 = widen(x)
    s = ref_scales(x64, stored)
    pieces, off = [], 4096
    for e0, cnt in ((0, n), (8, 30), (16, 50), (40, 2 * 1000 + 6),
                    (8, tile_elems() + 10), (0, 2), (40, 8), (16, 14)):
        for d in range(8):
            pieces.append((e0, cnt, off + d))
            off += (cnt + 127) // 64 * 64
    for elem_off in (0, 1):
        store_and_check(arena, on_gpu(x, elem_off), x64, s, stored, pieces)


def test_store_strided_rows_and_rejects(arena):
    rng = np.random.default_rng(63)
    w = random_weights(rng, "BF16", (9, 96))
    v = w[:, :64]
    x64 = widen(v)
    dev = on_gpu(w, 1)
    for stored in FORMATS:
        s = ref_scales(x64, stored)
        codes = ref_quant(x64, per_element(s, x64.shape), stored)
        dscale = torch.from_numpy(s.copy()).to("cuda:0")
        arena.fill(0, 8192, SENTINEL)
        torch.cuda.synchronize()
        # rows 1.. of the view: the piece begins 64 elements in
        arena.store_ptr([(dev.data_ptr() + 96 * 2, 4101, 8, 64, 96 * 2,
                          D["BF16"], D[stored], dscale.data_ptr(), 64, 64,
                          32)])
        exp = pack(codes[1:], stored)
        got = arena.read_bytes(4101 - 16, len(exp) + 32)
        assert got[16:-16] == exp
        assert got[:16] == got[-16:] == bytes([SENTINEL]) * 16
    arena.fill(0, 8192, SENTINEL)
    host = torch.ones(64)
    hs = torch.zeros(8, dtype=torch.uint8)
    torch.cuda.synchronize()
    p, q, bf, e4 = dev.data_ptr(), dscale.data_ptr(), D["BF16"], D["F8_E4M3"]
    for seg in [(p, 0, 1, 64, 128, bf, e4, 0, 0, 64, 32),
                (p, 0, 1, 64, 128, bf, D["F8_E5M2"], q, 0, 64, 32),
                (p, 0, 1, 64, 128, D["U8"], e4, q, 0, 64, 32),
                (p, 0, 1, 64, 128, bf, e4, q, 0, 64, 64),
                (p + 1, 0, 1, 64, 128, bf, e4, q, 0, 64, 32),
                (p, 16 * MiB - 8, 1, 64, 128, bf, e4, q, 0, 64, 32),
                (p, 0, 1, 63, 128, bf, D["F4"], q, 0, 64, 32),
                (p, 0, 1, 64, 128, bf, e4, q, 1 << 40, 64, 32),  # past scales
                (host.data_ptr(), 0, 1, 64, 128, D["F32"], e4, q, 0, 64, 32),
                (p, 0, 1, 64, 128, bf, e4, hs.data_ptr(), 0, 64, 32)]:
        with pytest.raises(ValueError):
            arena.store_ptr([(p, 64, 1, 64, 128, bf, e4, q, 0, 64, 32), seg])
    assert arena.read_bytes(0, 8192) == bytes([SENTINEL]) * 8192


# -------------------------------------------------------------------- load

def load_and_check(arena, off, rows, run, pitch_b, stored, dst, dscale, e0,
                   spitch, exp, n_nan, dst_off=1):
    n = rows * run
    out = torch.zeros(n + 16, dtype=TDT[dst], device="cuda:0")
    out.view(torch.uint8).fill_(SENTINEL)
    torch.cuda.synchronize()
    arena.convert_ptr([(off, out.data_ptr() + dst_off * out.element_size(),
                        rows, run, pitch_b, D[stored], D[dst],
                        dscale.data_ptr(), e0, spitch, 32)])
    assert_bits_equal(out[dst_off:dst_off + n], exp.reshape(-1), n_nan)
    side = out.view(torch.uint8).cpu()
    isz = out.element_size()
    assert (side[:dst_off * isz] == SENTINEL).all()
    assert (side[(dst_off + n) * isz:] == SENTINEL).all()


@pytest.mark.parametrize("dst", SOURCES)
@pytest.mark.parametrize("stored", FORMATS)
def test_load_every_code_and_scale(arena, stored, dst):
    """every element code under every scale byte (65 536 and 4 096 pairs;
    E2M1 blocks hold the 16 codes twice), from arena offsets 0..3"""
    n_codes = 256 if stored == "F8_E4M3" else 16
    per = max(n_codes, 32)
    codes = np.tile(np.arange(n_codes, dtype=np.uint8), 256 * per // n_codes)
    s = np.repeat(np.arange(256, dtype=np.uint8), per // 32)
    se = per_element(s, codes.shape)
    exp = ref_dequant(codes, se, stored, TDT[dst])
    nan = count_nan(codes, se, stored)
    dscale = torch.from_numpy(s.copy()).to("cuda:0")
    raw = pack(codes, stored)
    for k in range(4):
        arena.write(4096 + k, raw)
        load_and_check(arena, 4096 + k, 1, codes.size, len(raw), stored, dst,
                       dscale, 0, codes.size, exp, nan, dst_off=1 + k)


@pytest.mark.parametrize("dst", SOURCES)
@pytest.mark.parametrize("stored", FORMATS)
def test_load_shards_tiles_and_pieces(arena, stored, dst):
    rng = np.random.default_rng(64)
    bpe = 2 if stored == "F4" else 1
    n_codes = 256 if stored == "F8_E4M3" else 16
    rows, k = 2 * tile_elems() // 128 + 1, 128
    n = rows * k                                  # two tiles and a row
    codes = rng.integers(0, n_codes, n).astype(np.uint8)
    if stored == "F8_E4M3":
        codes[(codes & 0x7F) == 0x7F] = 0x7E
    s = rng.integers(90, 150, n // 32).astype(np.uint8)
    full = ref_dequant(codes, per_element(s, codes.shape), stored,
                       TDT[dst]).reshape(rows, k)
    dscale = torch.from_numpy(s.copy()).to("cuda:0")
    arena.write(8195, pack(codes, stored))
    load_and_check(arena, 8195, 1, n, n // bpe, stored, dst, dscale, 0, n,
                   full, 0)
    # last-dimension shard 1 of 2, dim-0 shard 1 of 3 (whole rows)
    load_and_check(arena, 8195 + 64 // bpe, rows, 64, k // bpe, stored, dst,
                   dscale, 64, k, full[:, 64:].contiguous(), 0, dst_off=0)
    r0, cnt = rows // 3, rows // 3
    load_and_check(arena, 8195 + r0 * k // bpe, 1, cnt * k, cnt * k // bpe,
                   stored, dst, dscale, r0 * k, cnt * k, full[r0:r0 + cnt], 0,
                   dst_off=3)
    # pieces as a file cut leaves them: mid-block starts, odd lengths
    for e0, cnt in ((8, 30), (16, 50), (40, 2006), (24, 2)):
        load_and_check(arena, 8195 + e0 // bpe, 1, cnt, cnt // bpe, stored,
                       dst, dscale, e0, cnt, full.reshape(-1)[e0:e0 + cnt], 0,
                       dst_off=5)


def test_load_rejects(arena):
    out = torch.zeros(128, device="cuda:0")
    sc = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    host = torch.zeros(128)
    torch.cuda.synchronize()
    p, q, f32, e4, f4 = out.data_ptr(), sc.data_ptr(), D["F32"], \
        D["F8_E4M3"], D["F4"]
    for seg in [(0, p, 1, 64, 64, e4, D["F64"], q, 0, 64, 32),
                (0, p, 1, 64, 64, D["F8_E5M2"], f32, q, 0, 64, 32),
                (0, p + 2, 1, 64, 64, e4, f32, q, 0, 64, 32),
                (0, 0, 1, 64, 64, e4, f32, q, 0, 64, 32),
                (0, p, 1, 64, 64, e4, f32, 0, 0, 64, 32),
                (16 * MiB - 8, p, 1, 64, 64, e4, f32, q, 0, 64, 32),
                (0, p, 1, 33, 33, f4, f32, q, 0, 64, 32),
                (0, p, 1, 1 << 20, 1 << 20, e4, f32, q, 0, 64, 32),  # past dst
                (0, p, 1, 64, 64, e4, f32, q, 1 << 40, 64, 32),
                (0, host.data_ptr(), 1, 64, 64, e4, f32, q, 0, 64, 32)]:
        with pytest.raises(ValueError):
            arena.convert_ptr([(0, p, 1, 64, 64, e4, f32, q, 0, 64, 32), seg])


# -------------------------------------------------------------- end to end

def test_end_to_end_hbm(tmp_path, monkeypatch):
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors, save_file
    from curvine_amd.testing import SyncMiniCluster

    rng = np.random.default_rng(65)
    w = random_weights(rng, "F32", (9, 96))
    cpu = {"a": random_weights(rng, "F32", (5, 64)),
           "b": random_weights(rng, "BF16", (130, 256)),
           "h": random_weights(rng, "F16", (3, 4, 32)),
           "cols": w[:, 32:96],
           "odd": random_weights(rng, "F32", (4, 33)),
           "bias": random_weights(rng, "F32", (67,))}
    w_dev = w.to("cuda:0")
    dev = {k: v.to("cuda:0") for k, v in cpu.items() if k != "cols"}
    dev["cols"] = w_dev[:, 32:96]

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
        for mode in ("mxfp8", "mxfp4"):
            blob, _start, ent, order = expected_mx_file(cpu, mode)
            assert len(blob) > 4 * 4112
            del calls[:]
            for bs in (8192, 4112):
                path = f"/mx/dev-{mode}-{bs}.safetensors"
                save_file(sf, dev, path, storage_tier="HBM", block_size=bs,
                          quantize=mode)
                check_file(smc, sf, path, blob)
            # typed stores on the GPU, MX ones among them, some of which
            # begin inside a tensor and inside a block
            mx = [s for d, segs in calls for s in segs
                  if d == 0 and len(s) == 11]
            assert mx and any(s[8] % 32 for s in mx)
            n_gpu = sum(d == 0 for d, _ in calls)
            save_file(sf, cpu, f"/mx/cpu-{mode}.safetensors",
                      storage_tier="MEM", block_size=4112, quantize=mode)
            assert sum(d == 0 for d, _ in calls) == n_gpu
            check_file(smc, sf, f"/mx/cpu-{mode}.safetensors", blob)

            bf, stored = torch.bfloat16, STORED[mode]
            full = {k: ref_dequant(
                ent[k][3], per_element(ent[k + "_scale"][3], ent[k][3].shape),
                stored, bf) for k in ("a", "b", "h", "cols")}
            with CurvineSafetensors(
                    sf, f"/mx/dev-{mode}-4112.safetensors") as f:
                assert f.keys() == order
                out = f.load(device="cuda:0", dtype=bf, dequantize=True)
                assert set(out) == set(cpu)
                for k in full:
                    assert out[k].is_cuda
                    assert_bits_equal(out[k], full[k], 0)
                assert_bits_equal(out["bias"], cpu["bias"].to(bf), 0)
                out = f.load(device="cuda:0", dtype=bf, dequantize=True,
                             shard_plan={"b": (0, 1, 2), "h": (1, 2, 4)},
                             names=["b", "h"])
                assert_bits_equal(out["b"], full["b"][65:], 0)
                assert_bits_equal(out["h"], full["h"][:, 2:3].contiguous(), 0)
                t = f.get_tensor("b", device="cuda:0", shard=(1, 1, 2),
                                 dequantize=True)
                exp = ref_dequant(
                    ent["b"][3], per_element(ent["b_scale"][3], (130, 256)),
                    stored, torch.float32)
                assert_bits_equal(t, exp[:, 128:].contiguous(), 0)
                plain = f.load(device="cuda:0")   # raw elements + scales
                assert plain["b_scale"].dtype == torch.float8_e8m0fnu
                assert plain["b"].view(torch.uint8).cpu().numpy() \
                    .tobytes() == ent["b"][2]
        sf.shutdown()
    finally:
        smc.stop()
