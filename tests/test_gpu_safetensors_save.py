"""store_segments_kernel (csrc/tensor_cast.hip) and safetensors save on the
MI355X.  Arena-level tests drive Arena.store_ptr from cuda tensors into a
sentinel-filled arena and read it back with read_bytes; every expected
value is torch's CPU result, compared bitwise (NaN inputs, which only the
conversion_sets() hold, must give NaN and are counted)."""
import numpy as np
import pytest
import torch

from curvine_amd import native
from curvine_amd.testing import test_conf as make_conf

from safetensors_cases import (ISZ, TORCH, assert_bits_equal,
                               conversion_sets, count_nan_inputs, expected,
                               from_raw)
from safetensors_save_cases import (check_file, expected_file, finite_raw,
                                    finite_tensor)

pytestmark = pytest.mark.gpu

D = native.DTYPES
MiB = 1 << 20
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(0, 64 * MiB)
    yield a
    a.close()


def tile_elems():
    return native.load().CAST_TILE


def on_gpu(raw: bytes, dt: str, elem_off: int = 0):
    """the elements of `raw` as a cuda tensor of `dt` that begins
    `elem_off` elements into its storage"""
    ss = ISZ[dt]
    buf = torch.zeros(len(raw) + elem_off * ss + 16, dtype=torch.uint8,
                      device="cuda:0")
    buf[elem_off * ss:elem_off * ss + len(raw)] = \
        torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda:0")
    t = buf[:len(raw) + elem_off * ss].view(TORCH[dt])[elem_off:]
    torch.cuda.synchronize()
    assert t.data_ptr() == buf.data_ptr() + elem_off * ss
    return t


def region(arena, lo, n):
    return np.frombuffer(arena.read_bytes(lo, n), dtype=np.uint8)


def check_written(got, src_cpu, src, dst):
    """one written range against torch on the CPU"""
    raw = src_cpu.contiguous().view(-1).view(torch.uint8).numpy().tobytes()
    if src == dst:
        assert got.tobytes() == raw
        return
    assert_bits_equal(from_raw(got.tobytes(), dst), expected(raw, src, dst),
                      count_nan_inputs(raw, src))


# ----------------------------------------------------------- numerics

@pytest.mark.parametrize(
    "idx", range(len(conversion_sets())),
    ids=[f"{s}-{d}-{len(r)}" for s, d, r in conversion_sets()])
def test_store_bitwise(arena, idx):
    s, d, raw = conversion_sets()[idx]
    ss, ds = ISZ[s], ISZ[d]
    n = len(raw) // ss
    exp, nan = expected(raw, s, d), count_nan_inputs(raw, s)
    arena.fill(0, 16 * MiB, SENTINEL)
    src = on_gpu(raw, s)
    arena.store_ptr([(src.data_ptr(), 4096, 1, n, n * ss, D[s], D[d])])
    got = region(arena, 4096 - 16, n * ds + 32)
    assert_bits_equal(from_raw(got[16:-16].tobytes(), d), exp, nan)
    assert (got[:16] == SENTINEL).all() and (got[-16:] == SENTINEL).all()
    # a view 3 elements into its storage, to a destination that is aligned
    # to its itemsize and to nothing more
    view = on_gpu(raw, s, 3)
    off = 8 * MiB + ds
    assert off % 16 and off % ds == 0
    arena.store_ptr([(view.data_ptr(), off, 1, n, n * ss, D[s], D[d])])
    got = region(arena, off - 16 - ds, n * ds + 32 + ds)
    assert_bits_equal(from_raw(got[16 + ds:-16].tobytes(), d), exp, nan)
    assert (got[:16 + ds] == SENTINEL).all() and (got[-16:] == SENTINEL).all()


# ---------------------------------------------------- alignment sweep

COUNTS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 4097]


@pytest.mark.parametrize("src,dst", [("F32", "BF16"), ("BF16", "F16"),
                                     ("BF16", "F32"), ("I8", "I8")])
def test_alignment_sweep(arena, src, dst):
    """source element offset 0..15 x counts x destination 0..3 elements
    past a 16-byte boundary, all 640 segments in one call; the sentinel
    stays on both sides of every written range."""
    rng = np.random.default_rng(5)
    ss, ds = ISZ[src], ISZ[dst]
    raw = finite_raw(rng, src, 4097 + 16)
    cpu = from_raw(raw, src)
    dev = on_gpu(raw, src)
    slot = ((4097 + 3) * ds + 15) // 16 * 16 + 32    # 16 B guard each side
    cases, segs = [], []
    for mis in range(16):
        for n in COUNTS:
            for doff in range(4):
                w0 = len(cases) * slot + 16 + doff * ds
                cases.append((mis, n, doff, w0))
                segs.append((dev.data_ptr() + mis * ss, w0, 1, n, n * ss,
                             D[src], D[dst]))
    total = len(cases) * slot
    assert total <= 32 * MiB
    arena.fill(0, total, SENTINEL)
    arena.store_ptr(segs)
    got = region(arena, 0, total)
    for i, (mis, n, doff, w0) in enumerate(cases):
        w1 = w0 + n * ds
        check_written(got[w0:w1], cpu[mis:mis + n], src, dst)
        assert (got[i * slot:w0] == SENTINEL).all(), ("before", mis, n, doff)
        assert (got[w1:(i + 1) * slot] == SENTINEL).all(), \
            ("after", mis, n, doff)


# --------------------------------------------------------- tile edges

@pytest.mark.parametrize("src,dst", [("F32", "BF16"), ("BF16", "F32"),
                                     ("I8", "I8"), ("I64", "I64")])
def test_tile_edges(arena, src, dst):
    rng = np.random.default_rng(6)
    ss, ds = ISZ[src], ISZ[dst]
    tile = tile_elems() if src != dst else 4 * tile_elems() // ss
    lens = [tile - 1, tile, tile + 1, 2 * tile + 1]
    raw = finite_raw(rng, src, max(lens) + 8)
    cpu = from_raw(raw, src)
    slot = ((max(lens) + 1) * ds + 15) // 16 * 16 + 32
    for elem_off in (1, 0):      # itemsize-aligned only, and 16 B aligned
        dev = on_gpu(raw, src, elem_off)
        arena.fill(0, len(lens) * slot, SENTINEL)
        segs = [(dev.data_ptr(), i * slot + 16 + ds, 1, n, n * ss,
                 D[src], D[dst]) for i, n in enumerate(lens)]
        arena.store_ptr(segs)
        got = region(arena, 0, len(lens) * slot)
        for i, n in enumerate(lens):
            w0 = i * slot + 16 + ds
            check_written(got[w0:w0 + n * ds], cpu[:n], src, dst)
            assert (got[i * slot:w0] == SENTINEL).all()
            assert (got[w0 + n * ds:(i + 1) * slot] == SENTINEL).all()


# ------------------------------------------------------------ strided

SHAPES = [(5, 4, 12), (4097, 3, 7), (9, 5000, 5003), (3, 64, 64),
          (700, 63, 65)]


@pytest.mark.parametrize("src,dst", [("F32", "BF16"), ("BF16", "F32"),
                                     ("I32", "I32")])
def test_strided(arena, src, dst):
    """rows of runs out of a wider tensor: short runs (element-wise path),
    runs that cross tiles, pitch == run, odd run lengths; the source
    begins one element into its storage."""
    rng = np.random.default_rng(8)
    ss, ds = ISZ[src], ISZ[dst]
    need = max((r - 1) * p + n for r, n, p in SHAPES)
    raw = finite_raw(rng, src, need)
    cpu = from_raw(raw, src)
    dev = on_gpu(raw, src, 1)
    starts, pos = [], 0
    for r, n, _p in SHAPES:
        starts.append(pos)
        pos += (r * n * ds + 15) // 16 * 16 + 32
    arena.fill(0, pos, SENTINEL)
    arena.store_ptr([(dev.data_ptr(), st + 16 + ds, r, n, p * ss,
                      D[src], D[dst])
                     for st, (r, n, p) in zip(starts, SHAPES)])
    got = region(arena, 0, pos)
    for i, (r, n, p) in enumerate(SHAPES):
        w0 = starts[i] + 16 + ds
        end = starts[i + 1] if i + 1 < len(SHAPES) else pos
        check_written(got[w0:w0 + r * n * ds],
                      cpu.as_strided((r, n), (p, 1)), src, dst)
        assert (got[starts[i]:w0] == SENTINEL).all()
        assert (got[w0 + r * n * ds:end] == SENTINEL).all()


# --------------------------------------------------------- mixed call

def test_mixed_big_and_many_small(arena):
    """one 4 Mi-element F32->BF16 segment in the middle of 300 segments of
    128 elements with mixed pairs and drifting destination alignment, in
    ONE call"""
    rng = np.random.default_rng(9)
    big_n = 4 << 20
    big_raw = finite_raw(rng, "F32", big_n)
    big = on_gpu(big_raw, "F32", 1)
    pairs = [("F32", "BF16"), ("BF16", "F32"), ("F16", "BF16"),
             ("F32", "F16"), ("F8_E5M2", "BF16"), ("I64", "I64"),
             ("BF16", "BF16"), ("F8_E4M3", "F32")]
    pos = 9 * MiB
    small, keep = [], []
    for i in range(300):
        s, d = pairs[i % len(pairs)]
        raw = finite_raw(rng, s, 128)
        t = on_gpu(raw, s, i % 7)
        keep.append(t)
        pos += 16 + (i % 5) * ISZ[d]              # drifting alignment
        pos += -pos % ISZ[d]
        small.append((s, d, pos, raw, t))
        pos += 128 * ISZ[d]
    arena.fill(0, pos + 64, SENTINEL)
    segs = [(t.data_ptr(), p, 1, 128, 128 * ISZ[s], D[s], D[d])
            for s, d, p, _r, t in small]
    segs.insert(150, (big.data_ptr(), 32, 1, big_n, big_n * 4,
                      D["F32"], D["BF16"]))
    arena.store_ptr(segs)
    got = region(arena, 0, pos + 64)
    assert_bits_equal(from_raw(got[32:32 + big_n * 2].tobytes(), "BF16"),
                      expected(big_raw, "F32", "BF16"), 0)
    assert (got[:32] == SENTINEL).all()
    prev = 32 + big_n * 2
    for s, d, p, raw, _t in small:
        assert (got[prev:p] == SENTINEL).all()
        check_written(got[p:p + 128 * ISZ[d]], from_raw(raw, s), s, d)
        prev = p + 128 * ISZ[d]
    assert (got[prev:] == SENTINEL).all()


# ------------------------------------------------------------ rejects

def test_binding_rejects_before_launch(arena):
    cap = 64 * MiB
    src = torch.full((64,), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p = src.data_ptr()
    arena.fill(0, 1 * MiB, SENTINEL)
    arena.fill(cap - MiB, MiB, SENTINEL)
    good = (p, 0, 1, 4, 16, D["F32"], D["F32"])
    bad = [
        (p, cap, 1, 1, 4, D["F32"], D["F32"]),              # past the arena
        (p, cap - 2, 1, 2, 8, D["F32"], D["BF16"]),         # last element
        (p, cap - 8, 3, 2, 16, D["F32"], D["BF16"]),        # last row
        (p, 0, 1 << 62, 2, 1 << 62, D["F32"], D["BF16"]),   # rows*pitch wraps
        (p, 0, 3, 1, (1 << 64) - 1, D["F32"], D["BF16"]),   # rows*pitch wraps
        (p, 0, 3, 1, 1 << 63, D["F32"], D["BF16"]),         # rows*pitch wraps
        (p, 8, (1 << 61) + 1, 1, 8, D["I64"], D["I64"]),    # size wraps
        (p, 0, 1, 1 << 62, 0, D["F32"], D["F32"]),          # run*ss wraps
        (p, 0, 1, 4, 16, 99, D["F32"]),                     # unknown code
        (p, 0, 1, 4, 16, D["F32"], 15),                     # unknown code
        (p, 0, 1, 4, 16, D["F32"], D["F8_E4M3"]),           # no fp8 downcast
        (p, 0, 1, 4, 16, D["I32"], D["F32"]),               # int -> float
        (0, 0, 1, 4, 16, D["F32"], D["F32"]),               # null source
        (p + 2, 0, 1, 4, 16, D["F32"], D["F32"]),           # misaligned src
        (p + 1, 0, 1, 4, 8, D["BF16"], D["F32"]),           # misaligned src
        (p, 2, 1, 4, 16, D["F32"], D["F32"]),               # misaligned dst
        (p, 1, 1, 4, 16, D["F32"], D["BF16"]),              # misaligned dst
    ]
    for seg in bad:
        with pytest.raises(ValueError):
            arena.store_ptr([seg])
        with pytest.raises(ValueError):
            arena.store_ptr([good, seg])    # whole call refused, no launch
    assert (region(arena, 0, MiB) == SENTINEL).all()
    assert (region(arena, cap - MiB, MiB) == SENTINEL).all()
    # zero-element segments are skipped: no launch, nothing written
    arena.store_ptr([(p, 0, 0, 4, 16, D["F32"], D["F32"]),
                     (0, 0, 4, 0, 16, D["F32"], D["F32"])])
    arena.store_ptr([])
    assert (region(arena, 0, 64) == SENTINEL).all()
    assert (src.cpu() == 7.0).all()


# --------------------------------------------------------- end to end

def test_end_to_end_hbm(tmp_path, monkeypatch):
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors, save_file
    from curvine_amd.testing import SyncMiniCluster

    rng = np.random.default_rng(12)
    w = finite_tensor(rng, "F32", (257, 1024))
    cpu = {"emb": finite_tensor(rng, "F32", (1200, 1030)),
           "proj": finite_tensor(rng, "BF16", (300, 1026)),
           "ids": finite_tensor(rng, "I64", (4099,)),
           "norm": finite_tensor(rng, "F32", (515,)),
           "cols": w[:, 100:613],
           "none": torch.empty((0, 4), dtype=torch.float32)}
    blob, start, stored, order = expected_file(
        cpu, {"format": "pt"}, torch.bfloat16)
    assert start % 64 == 0
    nblocks = -(-len(blob) // MiB)
    assert nblocks >= 4

    w_dev = w.to("cuda:0")
    dev = {k: v.to("cuda:0") for k, v in cpu.items() if k != "cols"}
    dev["cols"] = w_dev[:, 100:613]

    conf = make_conf(str(tmp_path))
    smc = SyncMiniCluster(conf=conf, tmp_dir=str(tmp_path),
                          worker_dirs=[["[HBM:512MB:0]gpu0"]]).start()
    calls = []
    orig = native.Arena.store_ptr

    def spy(self, segs):
        calls.append((self.device, list(segs)))
        return orig(self, segs)
    monkeypatch.setattr(native.Arena, "store_ptr", spy)
    try:
        sf = SyncFs(smc.client_conf())
        st = save_file(sf, dev, "/m/ckpt.safetensors",
                       metadata={"format": "pt"}, dtype=torch.bfloat16,
                       storage_tier="HBM", block_size=MiB)
        assert st.length == len(blob)
        assert 0 < len(calls) <= nblocks
        assert all(d == 0 for d, _ in calls)
        assert any(len(segs) > 1 for _, segs in calls)   # not per tensor
        lo = w_dev.data_ptr()
        cols = [s for _, segs in calls for s in segs
                if lo <= s[0] < lo + w_dev.numel() * 4]
        assert cols and any(s[2] > 1 for s in cols)
        # header, padding and data through the ordinary byte read path,
        # and every block's publish-time CRC
        check_file(smc, sf, "/m/ckpt.safetensors", blob)
        with CurvineSafetensors(sf, "/m/ckpt.safetensors") as f:
            assert f.keys() == order
            out = f.load(device="cuda:0")
            assert f.reader.verify() == []
        for name in cpu:
            assert out[name].is_cuda
            assert_bits_equal(out[name], stored[name], 0)
        sf.shutdown()
    finally:
        smc.stop()
