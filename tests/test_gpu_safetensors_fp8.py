"""absmax_segments_kernel, the quantising store and the scaled load
(csrc/tensor_cast.hip) on the MI355X, then save_file(quantize="row") and
load(dequantize=True) through the HBM tier.  Shapes are the smallest at
which each path of the kernels can go wrong.  Every expected value is the
torch CPU reference of safetensors_fp8_cases; comparisons are bitwise."""
import numpy as np
import pytest
import torch

from curvine_amd import native
from curvine_amd.testing import test_conf as make_conf

from safetensors_cases import ISZ, TORCH, assert_bits_equal, from_raw
from safetensors_fp8_cases import (SOURCES, expected_fp8_file, flat_dequant,
                                   flat_quant, flat_scales, random_weights,
                                   ref_dequant)
from safetensors_save_cases import check_file

pytestmark = pytest.mark.gpu

D = native.DTYPES
MiB = 1 << 20
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(0, 16 * MiB)
    yield a
    a.close()


def tile_elems():
    return native.load().CAST_TILE


def on_gpu(t, elem_off=0):
    """a cuda copy of the 1-D cpu tensor `t` that begins `elem_off`
    elements into its storage"""
    buf = torch.zeros(t.numel() + elem_off + 8, dtype=t.dtype,
                      device="cuda:0")
    buf[elem_off:elem_off + t.numel()] = t.to("cuda:0")
    torch.cuda.synchronize()
    return buf[elem_off:elem_off + t.numel()]


def region(arena, lo, n):
    return np.frombuffer(arena.read_bytes(lo, n), dtype=np.uint8)


def gpu_scales(dev, rows, run, pitch, src, every, n_groups, e0=0):
    out = torch.full((n_groups,), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    native.absmax_scales(0, [(dev.data_ptr(), rows, run, pitch * ISZ[src],
                              D[src], out.data_ptr(), every, e0, n_groups)])
    return out


# ------------------------------------------------------------------ absmax

@pytest.mark.parametrize("src", SOURCES)
def test_absmax_one_group_many_workgroups(src):
    """CAST_TILE*2 + 3 elements in one group: three workgroups meet in one
    slot; then the maximum at the first and last element and on both sides
    of the lane 63/64 and lane 255/256 boundaries of a unit."""
    rng = np.random.default_rng(41)
    n = tile_elems() * 2 + 3
    k = 16 // ISZ[src]                  # elements per 16-byte unit
    x = random_weights(rng, src, (n,), spread=False)
    for elem_off in (0, 1):             # 16-byte aligned, and a head
        dev = on_gpu(x, elem_off)
        assert_bits_equal(gpu_scales(dev, 1, n, n, src, 0, 1),
                          flat_scales(x, 0)[0], 0)
    dev = on_gpu(x)
    for pos in (0, n - 1, 63 * k + k - 1, 64 * k, 255 * k + k - 1, 256 * k,
                tile_elems() - 1, tile_elems()):
        y = x.clone()
        y[pos] = -300.0
        dev.copy_(y)
        torch.cuda.synchronize()
        got = gpu_scales(dev, 1, n, n, src, 0, 1)
        assert_bits_equal(got, flat_scales(y, 0)[0], 0)
        assert got.item() == (torch.tensor(300.0) / 448).item(), pos


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("rows,run", [(5, 67), (3, 8), (300, 64)])
def test_absmax_groups_inside_a_tile(src, rows, run):
    """row groups: several per tile with short-ish runs, the short-run
    branch, and rows crossing a tile boundary; contiguous, so the layout
    is one run while the groups follow the rows"""
    rng = np.random.default_rng(42)
    x = random_weights(rng, src, (rows, run))
    exp = flat_scales(x.reshape(-1), run)[0]
    dev = on_gpu(x.reshape(-1), 1)
    got = gpu_scales(dev, 1, rows * run, rows * run, src, run, rows)
    assert_bits_equal(got, exp, 0)
    got = gpu_scales(dev, rows, run, run, src, run, rows)    # as rows
    assert_bits_equal(got, exp, 0)


@pytest.mark.parametrize("src", SOURCES)
def test_absmax_strided_view_and_offsets(src):
    """rows=4, run=300, pitch=307: the gaps hold huge values that must not
    be seen; the source starts one element into its storage; a piece that
    begins mid-tensor (scale_e0) writes the slots of its own groups."""
    rng = np.random.default_rng(43)
    w = random_weights(rng, src, (4, 307), spread=False)
    w[:, 300:] = 60000.0
    v = w[:, :300]
    v[3, 299] = 17.0                      # the view's last element
    dev = on_gpu(w.reshape(-1), 1)
    exp_row = flat_scales(v.reshape(-1), 300)[0]
    assert_bits_equal(gpu_scales(dev, 4, 300, 307, src, 300, 4), exp_row, 0)
    assert_bits_equal(gpu_scales(dev, 4, 300, 307, src, 0, 1),
                      flat_scales(v.reshape(-1), 0)[0], 0)
    x = random_weights(rng, src, (500,))
    exp, _ = flat_scales(x, 67, 139)
    got = gpu_scales(on_gpu(x, 1), 1, 500, 500, src, 67, exp.numel(), 139)
    assert_bits_equal(got, exp, 0)


def test_absmax_special_groups_and_rejects():
    floor = torch.tensor([2.0 ** -40]) / 448
    for vals in ([0.0, -0.0] * 40, [float("inf"), float("nan")] * 40,
                 [2.0 ** -41, 0.0] * 40):
        x = torch.tensor(vals, dtype=torch.float32)
        assert_bits_equal(gpu_scales(on_gpu(x), 1, 80, 80, "F32", 0, 1),
                          floor, 0)
    x = on_gpu(torch.ones(64))
    out = torch.full((4,), 7.0, device="cuda:0")
    host = torch.ones(64)
    torch.cuda.synchronize()
    p, o = x.data_ptr(), out.data_ptr()
    for seg in [(p, 1, 64, 256, D["I32"], o, 0, 0, 1),
                (0, 1, 64, 256, D["F32"], o, 0, 0, 1),
                (p, 1, 64, 256, D["F32"], o + 2, 0, 0, 1),
                (p, 1, 64, 256, D["F32"], o, 16, 0, 3),
                (p, 1, 1 << 28, 1 << 30, D["F32"], o, 0, 0, 1),  # past alloc
                (host.data_ptr(), 1, 64, 256, D["F32"], o, 0, 0, 1),
                (p, 1, 64, 256, D["F32"], host.data_ptr(), 0, 0, 1)]:
        with pytest.raises(ValueError):
            native.absmax_scales(0, [(p, 1, 64, 256, D["F32"], o, 16, 0, 4),
                                     seg])
    assert (out.cpu() == 7.0).all()                # refused before launch


# -------------------------------------------------------- quantising store

COUNTS = [1, 3, 4, 15, 16, 17, 63, 64, 65, 1023]
OFFSETS = [4096, 4097, 4099, 4111]


@pytest.mark.parametrize("src", SOURCES)
def test_quantising_store_alignment(arena, src):
    """1-byte-aligned destinations x counts, source 0 and 1 elements into
    its storage (load modes 1 and 2 for 16-bit sources), all in one call
    with one scale; 16 sentinel bytes stay on each side."""
    rng = np.random.default_rng(44)
    ss = ISZ[src]
    counts = COUNTS + [tile_elems() + 5]
    x = random_weights(rng, src, (max(counts) + 1,))
    scales, _ = flat_scales(x, 0)
    exp = flat_quant(x, scales, torch.zeros(x.numel(), dtype=torch.int64))
    dev = on_gpu(x)
    dscale = scales.to("cuda:0")
    slot = (max(counts) + 15 + 31) // 16 * 16 + 32
    cases, segs = [], []
    for eoff in (0, 1):
        for off in OFFSETS:
            for n in counts:
                w0 = len(cases) * slot + off
                cases.append((eoff, n, w0))
                segs.append((dev.data_ptr() + eoff * ss, w0, 1, n, n * ss,
                             D[src], D["F8_E4M3"], dscale.data_ptr(), 0, 0))
    total = len(cases) * slot + 8192
    assert total <= 16 * MiB
    arena.fill(0, total, SENTINEL)
    torch.cuda.synchronize()
    arena.store_ptr(segs)
    got = region(arena, 0, total)
    prev = 0
    for eoff, n, w0 in cases:
        assert (got[prev:w0] == SENTINEL).all(), ("before", eoff, n, w0)
        assert w0 - prev >= 16
        assert_bits_equal(from_raw(got[w0:w0 + n].tobytes(), "F8_E4M3"),
                          exp[eoff:eoff + n], 0)
        prev = w0 + n
    assert (got[prev:prev + 16] == SENTINEL).all()


@pytest.mark.parametrize("src", SOURCES)
@pytest.mark.parametrize("every,rows,run,pitch", [
    (67, 1, 67 * 9, 67 * 9),       # collapsed: runs cut at group ends
    (67, 7, 67, 80),               # strided rows, one group per run
    (8, 1, 8 * 40, 8 * 40),        # short groups: element-wise branch
    (8, 40, 8, 11),                # short runs
    (300, 1, 300 * 120, 300 * 120),  # groups and tiles interleave
])
def test_quantising_store_row_scales(arena, src, every, rows, run, pitch):
    """row scales with the piece starting mid-tensor (scale_e0 = 67*2 + 5
    for groups of 67): the block-split case"""
    rng = np.random.default_rng(45)
    ss = ISZ[src]
    e0 = every * 2 + 5
    w = random_weights(rng, src, (rows, pitch))
    v = w[:, :run].reshape(-1)
    scales, idx = flat_scales(v, every, e0)
    exp = flat_quant(v, scales, idx)
    dev = on_gpu(w.reshape(-1), 1)
    dscale = scales.to("cuda:0")
    n = rows * run
    arena.fill(0, n + 8192, SENTINEL)
    torch.cuda.synchronize()
    arena.store_ptr([(dev.data_ptr(), 4099, rows, run, pitch * ss, D[src],
                      D["F8_E4M3"], dscale.data_ptr(), every, e0)])
    got = region(arena, 4099 - 16, n + 32)
    assert_bits_equal(from_raw(got[16:-16].tobytes(), "F8_E4M3"), exp, 0)
    assert (got[:16] == SENTINEL).all() and (got[-16:] == SENTINEL).all()


def test_special_values_and_rejects(arena):
    x = torch.tensor([0.0, -0.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 447.9, 448.0,
                      465.0, 1e9, float("inf"), float("-inf"), float("nan"),
                      -3.0] * 11, dtype=torch.float32)
    one = torch.ones(1)
    exp = flat_quant(x, one, torch.zeros(x.numel(), dtype=torch.int64))
    dev, dscale = on_gpu(x), one.to("cuda:0")
    arena.fill(0, 8192, SENTINEL)
    torch.cuda.synchronize()
    p, s = dev.data_ptr(), dscale.data_ptr()
    arena.store_ptr([(p, 4097, 1, x.numel(), 0, D["F32"], D["F8_E4M3"],
                      s, 0, 0)])
    assert_bits_equal(from_raw(region(arena, 4097, x.numel()).tobytes(),
                               "F8_E4M3"), exp, 11)
    arena.fill(0, 8192, SENTINEL)
    host = torch.ones(4)
    for seg in [(p, 0, 1, 8, 32, D["F32"], D["F8_E4M3"], 0, 0, 0),
                (p, 0, 1, 8, 32, D["F32"], D["F8_E4M3"], s + 2, 0, 0),
                (p, 0, 1, 8, 32, D["F32"], D["BF16"], s, 0, 0),
                (p, 0, 1, 8, 32, D["F32"], D["F8_E4M3"], host.data_ptr(),
                 0, 0)]:
        with pytest.raises(ValueError):
            arena.store_ptr([seg])
    assert (region(arena, 0, 8192) == SENTINEL).all()


# ------------------------------------------------------------- scaled load

@pytest.mark.parametrize("dst", SOURCES)
@pytest.mark.parametrize("off", [4096, 4099])
def test_scaled_load(arena, dst, off):
    rng = np.random.default_rng(46)
    n = tile_elems() + 67 * 3 + 5
    q = torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)) \
        .view(torch.float8_e4m3fn)
    nan = int(torch.isnan(q.float()).sum())
    arena.write(off, q.view(torch.uint8).numpy().tobytes())
    for every, e0 in ((0, 0), (67, 0), (67, 139), (8, 3)):
        n_groups = (e0 + n - 1) // every + 1 if every else 1
        scales = torch.from_numpy(np.exp2(
            rng.integers(-20, 6, n_groups)).astype(np.float32) * 1.37)
        idx = (torch.arange(n) + e0) // every if every else \
            torch.zeros(n, dtype=torch.int64)
        dscale = scales.to("cuda:0")
        out = torch.zeros(n + 8, dtype=TORCH[dst], device="cuda:0")
        torch.cuda.synchronize()
        arena.convert_ptr([(off, out.data_ptr() + ISZ[dst], 1, n, n,
                            D["F8_E4M3"], D[dst], dscale.data_ptr(),
                            every, e0)])
        assert_bits_equal(out[1:n + 1], flat_dequant(q, scales, idx,
                                                     TORCH[dst]), nan)
        assert (out[0] == 0).item() and (out[n + 1:] == 0).all().item()


# ----------------------------------------------------------- old interface

def test_seven_tuples_unchanged(arena):
    rng = np.random.default_rng(47)
    x = random_weights(rng, "F32", (1000,))
    dev = on_gpu(x, 1)
    arena.fill(0, 16384, SENTINEL)
    torch.cuda.synchronize()
    arena.store_ptr([(dev.data_ptr(), 4098, 1, 1000, 4000, D["F32"],
                      D["BF16"])])
    got = region(arena, 4098 - 16, 2000 + 32)
    assert_bits_equal(from_raw(got[16:-16].tobytes(), "BF16"),
                      x.to(torch.bfloat16), 0)
    assert (got[:16] == SENTINEL).all() and (got[-16:] == SENTINEL).all()
    out = torch.zeros(1000, dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    arena.convert_ptr([(4098, out.data_ptr(), 1, 1000, 2000, D["BF16"],
                        D["F16"])])
    assert_bits_equal(out, x.to(torch.bfloat16).to(torch.float16), 0)
    q = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn)
    arena.write(8195, q.view(torch.uint8).numpy().tobytes())
    out = torch.zeros(256, dtype=torch.bfloat16, device="cuda:0")
    torch.cuda.synchronize()
    arena.convert_ptr([(8195, out.data_ptr(), 1, 256, 256, D["F8_E4M3"],
                        D["BF16"])])                 # the unscaled upcast
    assert_bits_equal(out, q.to(torch.bfloat16), 2)


# -------------------------------------------------------------- end to end

def test_end_to_end_hbm(tmp_path, monkeypatch):
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors, save_file
    from curvine_amd.testing import SyncMiniCluster

    rng = np.random.default_rng(48)
    w = random_weights(rng, "F32", (9, 80))
    cpu = {"a": random_weights(rng, "F32", (5, 67)),
           "b": random_weights(rng, "BF16", (130, 256)),
           "cols": w[:, 3:70],
           "bias": random_weights(rng, "F32", (67,))}
    blob, _start, stored, order = expected_fp8_file(cpu, "row")
    block = 8192
    assert len(blob) > 4 * block            # "b" straddles several blocks
    w_dev = w.to("cuda:0")
    dev = {k: v.to("cuda:0") for k, v in cpu.items() if k != "cols"}
    dev["cols"] = w_dev[:, 3:70]

    conf = make_conf(str(tmp_path))
    smc = SyncMiniCluster(conf=conf, tmp_dir=str(tmp_path),
                          worker_dirs=[["[HBM:512MB:0]gpu0"]]).start()
    try:
        sf = SyncFs(smc.client_conf())
        calls = []
        orig = native.Arena.store_ptr

        def spy(self, segs):
            calls.append((self.device, list(segs)))
            return orig(self, segs)
        monkeypatch.setattr(native.Arena, "store_ptr", spy)
        save_file(sf, dev, "/q/dev.safetensors", storage_tier="HBM",
                  block_size=block, quantize="row")
        # fast blocks: typed stores on the GPU, quantising ones among
        # them, one of which begins inside "b" (the block-split case)
        assert calls and all(d == 0 for d, _ in calls)
        scaled = [s for _, segs in calls for s in segs if len(s) == 10]
        assert scaled and any(s[9] > 0 for s in scaled)
        n_calls = len(calls)
        save_file(sf, cpu, "/q/cpu.safetensors", storage_tier="HBM",
                  block_size=block, quantize="row")
        assert len(calls) == n_calls             # the byte path
        check_file(smc, sf, "/q/dev.safetensors", blob)
        check_file(smc, sf, "/q/cpu.safetensors", blob)

        bf = torch.bfloat16
        full = {k: ref_dequant(stored[k], stored[k + "_scale"], bf)
                for k in ("a", "b", "cols")}
        with CurvineSafetensors(sf, "/q/dev.safetensors") as f:
            assert f.keys() == order
            out = f.load(device="cuda:0", dtype=bf, dequantize=True)
            assert set(out) == set(cpu)
            for k in full:
                assert out[k].is_cuda
                assert_bits_equal(out[k], full[k], 0)
            assert_bits_equal(out["bias"], cpu["bias"].to(bf), 0)
            out = f.load(device="cuda:0", dtype=bf, dequantize=True,
                         shard_plan={"b": (0, 1, 2), "cols": (1, 0, 1),
                                     "a": (1, 0, 1)},
                         names=["a", "b", "cols"])
            assert_bits_equal(out["b"], full["b"][65:], 0)
            assert_bits_equal(out["cols"], full["cols"], 0)
            out = f.load(device="cuda:0", dtype=bf, dequantize=True,
                         shard_plan={"b": (1, 1, 2)}, names=["b"])
            assert_bits_equal(out["b"], full["b"][:, 128:].contiguous(), 0)
            plain = f.load(device="cuda:0")      # without: raw fp8 + scales
            assert_bits_equal(plain["b"], stored["b"], 0)
            assert_bits_equal(plain["b_scale"], stored["b_scale"], 0)
        sf.shutdown()
    finally:
        smc.stop()
