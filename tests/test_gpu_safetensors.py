"""convert_segments_kernel (csrc/tensor_cast.hip) and the safetensors
loader on the MI355X.  Arena-level tests drive Arena.convert_ptr directly
into cuda tensors; every expected value is torch's CPU result, compared
bitwise (NaN inputs must give NaN and are counted)."""
import numpy as np
import pytest
import torch

from curvine_amd import native
from curvine_amd.testing import test_conf as make_conf

from safetensors_cases import (ISZ, TORCH, assert_bits_equal, build_file,
                               conversion_sets, count_nan_inputs, expected,
                               from_raw)

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


def finite_raw(rng, dt, n):
    """random bit patterns with the top exponent bit cleared: no NaN/inf,
    so a comparison can be plain bytes"""
    if dt == "F32":
        return (rng.integers(0, 2 ** 32, n, dtype=np.uint32)
                & np.uint32(0xBFFFFFFF)).tobytes()
    if dt in ("BF16", "F16"):
        return (rng.integers(0, 65536, n, dtype=np.uint16)
                & np.uint16(0xBFFF)).tobytes()
    raw = rng.integers(0, 256, n * ISZ[dt], dtype=np.uint8)
    if dt.startswith("F8"):
        raw &= np.uint8(0xBF)
    return raw.tobytes()


def convert(arena, src, dst, segs_shape, dst_elems):
    """segs_shape: [(src_off, dst_elem_off, rows, run, pitch)] into one
    sentinel-filled cuda buffer of dst_elems elements; returns its bytes
    on the CPU."""
    ds = ISZ[dst]
    buf = torch.full((dst_elems * ds,), SENTINEL, dtype=torch.uint8,
                     device="cuda:0")
    torch.cuda.synchronize()
    base = buf.data_ptr()
    arena.convert_ptr([(so, base + de * ds, rows, run, pitch, D[src], D[dst])
                       for so, de, rows, run, pitch in segs_shape])
    return buf.cpu().numpy()


def check_segment(got_bytes, raw_at, src, dst, rows, run, pitch):
    """one written range against torch on the CPU; raw_at(off, n) reads the
    source bytes.  Misaligned reads reinterpret the source, so NaN inputs
    can appear: they are exempted and counted, as everywhere."""
    ss = ISZ[src]
    src_bytes = b"".join(raw_at(r * pitch, run * ss) for r in range(rows))
    got = from_raw(bytes(got_bytes), dst)
    assert_bits_equal(got, expected(src_bytes, src, dst),
                      count_nan_inputs(src_bytes, src))


# ----------------------------------------------------------- numerics

@pytest.mark.parametrize(
    "idx", range(len(conversion_sets())),
    ids=[f"{s}-{d}-{len(r)}" for s, d, r in conversion_sets()])
def test_conversion_bitwise(arena, idx):
    s, d, raw = conversion_sets()[idx]
    n = len(raw) // ISZ[s]
    arena.write(3, raw)                      # odd source offset
    out = torch.empty(n, dtype=TORCH[d], device="cuda:0")
    torch.cuda.synchronize()
    arena.convert_ptr([(3, out.data_ptr(), 1, n, n * ISZ[s], D[s], D[d])])
    assert_bits_equal(out, expected(raw, s, d), count_nan_inputs(raw, s))
    # and from a 16-byte aligned source (the vector-load tier)
    arena.write(4096, raw)
    out2 = torch.empty(n, dtype=TORCH[d], device="cuda:0")
    torch.cuda.synchronize()
    arena.convert_ptr([(4096, out2.data_ptr(), 1, n, n * ISZ[s], D[s], D[d])])
    assert_bits_equal(out2, expected(raw, s, d), count_nan_inputs(raw, s))


# ---------------------------------------------------- alignment sweep

COUNTS = [1, 2, 3, 7, 8, 9, 63, 64, 65, 4097]


@pytest.mark.parametrize("src,dst", [("F32", "BF16"), ("BF16", "F16"),
                                     ("I8", "I8")])
def test_alignment_sweep(arena, src, dst):
    """src_off % 16 in 0..15 x counts x destination element offset 0..3,
    all 640 segments in one call; the bytes around every written range
    keep their sentinel."""
    rng = np.random.default_rng(5)
    ss, ds = ISZ[src], ISZ[dst]
    raw = finite_raw(rng, src, 4097 + 16)
    arena.write(1024, raw + b"\0" * 16)
    slot = 4097 + 15                         # elements, room for offset+guard
    slot = (slot * ds + 15) // 16 * 16 // ds
    cases, segs = [], []
    for mis in range(16):
        for n in COUNTS:
            for doff in range(4):
                de = len(cases) * slot + doff
                cases.append((mis, n, doff, de))
                segs.append((1024 + mis, de, 1, n, n * ss))
    got = convert(arena, src, dst, segs, len(cases) * slot)
    src_np = np.frombuffer(raw + b"\0" * 16, dtype=np.uint8)
    for i, (mis, n, doff, de) in enumerate(cases):
        lo, hi = i * slot * ds, (i + 1) * slot * ds
        w0, w1 = de * ds, (de + n) * ds
        check_segment(got[w0:w1],
                      lambda o, k: src_np[mis + o:mis + o + k].tobytes(),
                      src, dst, 1, n, n * ss)
        assert (got[lo:w0] == SENTINEL).all(), ("before", mis, n, doff)
        assert (got[w1:hi] == SENTINEL).all(), ("after", mis, n, doff)


# --------------------------------------------------------- tile edges

@pytest.mark.parametrize("src,dst", [("F32", "BF16"), ("BF16", "F32"),
                                     ("F8_E4M3", "F16"), ("I8", "I8"),
                                     ("I64", "I64")])
def test_tile_edges(arena, src, dst):
    rng = np.random.default_rng(6)
    ss, ds = ISZ[src], ISZ[dst]
    tile = tile_elems() if src != dst else 4 * tile_elems() // ss
    lens = [tile - 1, tile, tile + 1, 2 * tile + 1]
    raw = finite_raw(rng, src, max(lens) + 8)
    for src_off in (7 * ss + 1, 256):        # odd, and 16-byte aligned
        arena.write(src_off, raw)
        slot = (max(lens) + 8) * ds // 16 * 16 // ds + 16 // ds
        segs = [(src_off, i * slot + 1, 1, n, n * ss)
                for i, n in enumerate(lens)]
        got = convert(arena, src, dst, segs, len(lens) * slot)
        for i, n in enumerate(lens):
            w0 = (i * slot + 1) * ds
            check_segment(got[w0:w0 + n * ds], lambda o, k: raw[o:o + k],
                          src, dst, 1, n, n * ss)
            assert (got[i * slot * ds:w0] == SENTINEL).all()
            assert (got[w0 + n * ds:(i + 1) * slot * ds] == SENTINEL).all()


# ------------------------------------------------------------ strided

@pytest.mark.parametrize("src,dst", [("F32", "BF16"), ("BF16", "F32"),
                                     ("I32", "I32"), ("U8", "U8")])
def test_strided(arena, src, dst):
    """(5 x 4 of pitch 12) from an odd offset, 4097 runs of 3 (many short
    runs), and long runs that cross tiles (9 x 5000 of pitch 5003)."""
    rng = np.random.default_rng(8)
    ss, ds = ISZ[src], ISZ[dst]
    shapes = [(5, 4, 12 * ss), (4097, 3, 7 * ss + 1), (9, 5000, 5003 * ss),
              (3, 64, 64 * ss), (700, 63, 65 * ss)]
    need = max((r - 1) * p + n * ss for r, n, p in shapes)
    raw = finite_raw(rng, src, need // ss + 2)
    src_off = 16 * 100 + 5
    arena.write(src_off, raw)
    slot_of = [(r * n * ds + 31) // 16 * 16 // ds for r, n, _ in shapes]
    starts = np.concatenate([[0], np.cumsum(slot_of)])
    segs = [(src_off, int(starts[i]) + 1, r, n, p)
            for i, (r, n, p) in enumerate(shapes)]
    got = convert(arena, src, dst, segs, int(starts[-1]))
    for i, (r, n, p) in enumerate(shapes):
        w0 = (int(starts[i]) + 1) * ds
        check_segment(got[w0:w0 + r * n * ds], lambda o, k: raw[o:o + k],
                      src, dst, r, n, p)
        assert (got[int(starts[i]) * ds:w0] == SENTINEL).all()
        assert (got[w0 + r * n * ds:int(starts[i + 1]) * ds]
                == SENTINEL).all()


# --------------------------------------------------------- mixed call

def test_mixed_big_and_many_small(arena):
    """one 4 Mi-element tensor and 300 tensors of 128 elements with mixed
    dtype pairs in ONE segment list"""
    rng = np.random.default_rng(9)
    big_n = 4 << 20
    big = rng.integers(0, 2 ** 32, big_n, dtype=np.uint32).tobytes()
    arena.write(1, big)                       # odd offset, 16 MiB
    pairs = [("F32", "BF16"), ("BF16", "F32"), ("F16", "BF16"),
             ("F32", "F16"), ("F8_E5M2", "BF16"), ("I64", "I64"),
             ("BF16", "BF16"), ("F8_E4M3", "F32")]
    pos = 17 * MiB
    small = []
    for i in range(300):
        s, d = pairs[i % len(pairs)]
        raw = rng.integers(0, 256, 128 * ISZ[s], dtype=np.uint8).tobytes()
        pos += i % 5                          # drifting alignment
        arena.write(pos, raw)
        small.append((s, d, pos, raw))
        pos += len(raw)
    big_out = torch.empty(big_n, dtype=torch.bfloat16, device="cuda:0")
    outs = [torch.empty(128, dtype=TORCH[d], device="cuda:0")
            for _s, d, _p, _r in small]
    torch.cuda.synchronize()
    segs = [(p, o.data_ptr(), 1, 128, 128 * ISZ[s], D[s], D[d])
            for (s, d, p, _r), o in zip(small, outs)]
    segs.insert(150, (1, big_out.data_ptr(), 1, big_n, big_n * 4,
                      D["F32"], D["BF16"]))
    arena.convert_ptr(segs)
    assert_bits_equal(big_out, expected(big, "F32", "BF16"),
                      count_nan_inputs(big, "F32"))
    for (s, d, _p, raw), o in zip(small, outs):
        if s == d:
            assert o.cpu().view(torch.uint8).numpy().tobytes() == raw
        else:
            assert_bits_equal(o, expected(raw, s, d),
                              count_nan_inputs(raw, s))


# ------------------------------------------------------------ rejects

def test_binding_rejects_before_launch(arena):
    cap = 64 * MiB
    dst = torch.full((64,), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p = dst.data_ptr()
    good = (0, p, 1, 4, 16, D["F32"], D["F32"])
    bad = [
        (cap, p, 1, 1, 4, D["F32"], D["F32"]),             # past the end
        (cap - 6, p, 1, 2, 8, D["F32"], D["BF16"]),        # last run
        (0, p, 3, 2, cap // 2, D["F32"], D["BF16"]),       # last row
        (0, p, 1 << 62, 2, 1 << 62, D["F32"], D["BF16"]),  # rows*pitch wraps
        (0, p, 3, 1, (1 << 64) - 1, D["F32"], D["BF16"]),  # rows*pitch wraps
        (0, p, 3, 1, 1 << 63, D["F32"], D["BF16"]),        # rows*pitch wraps
        (8, p, (1 << 61) + 1, 1, 8, D["I64"], D["I64"]),   # size wraps
        (0, p, 1, 4, 16, 99, D["F32"]),                    # unknown code
        (0, p, 1, 4, 16, D["F32"], 15),                    # unknown code
        (0, p, 1, 4, 16, D["F32"], D["F8_E4M3"]),          # no fp8 downcast
        (0, p, 1, 4, 16, D["I32"], D["F32"]),              # int -> float
    ]
    for seg in bad:
        with pytest.raises(ValueError):
            arena.convert_ptr([seg])
        with pytest.raises(ValueError):
            arena.convert_ptr([good, seg])   # whole call refused, no launch
    torch.cuda.synchronize()
    assert (dst.cpu() == 7.0).all()


# --------------------------------------------------------- end to end

def test_end_to_end_hbm(tmp_path, monkeypatch):
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors
    from curvine_amd.testing import SyncMiniCluster

    rng = np.random.default_rng(12)
    emb = rng.integers(0, 2 ** 32, (1200, 1030), dtype=np.uint32)  # 4.7 MiB
    emb &= np.uint32(0xBFFFFFFF)
    tens = [("norm", "F32", (515,), finite_raw(rng, "F32", 515)),
            ("emb", "F32", emb.shape, emb.tobytes()),
            ("proj", "BF16", (300, 1026), finite_raw(rng, "BF16", 300 * 1026)),
            ("ids", "I64", (4099,), finite_raw(rng, "I64", 4099))]
    blob, start = build_file(tens, metadata={"format": "pt"}, data_start=333)
    assert start % 2 == 1 and 5 * MiB < len(blob) < 7 * MiB

    conf = make_conf(str(tmp_path))
    smc = SyncMiniCluster(conf=conf, tmp_dir=str(tmp_path),
                          worker_dirs=[["[HBM:512MB:0]gpu0"]]).start()
    calls = []
    orig = native.Arena.convert_ptr

    def spy(self, segs):
        calls.append((self.device, len(segs)))
        return orig(self, segs)
    monkeypatch.setattr(native.Arena, "convert_ptr", spy)
    try:
        sf = SyncFs(smc.client_conf())
        sf.write_file("/m/model.safetensors", blob, storage_tier="HBM",
                      block_size=MiB)
        f = CurvineSafetensors(sf, "/m/model.safetensors")
        nblocks = len(f.reader.fb.blocks)
        assert nblocks >= 6
        # the only slow-list entries: elements straddling a block boundary
        reqs = [f._request(f.info(n), "BF16" if dt != "I64" else "I64",
                           None, 1 << 30) for n, dt, _s, _r in tens]
        _groups, slow = f.reader.resolve_convert(reqs, True)
        assert 0 < len(slow) < nblocks and all(s[1] == 1 for s in slow)

        out = f.load(device="cuda:0", dtype=torch.bfloat16)
        assert calls == [(0, calls[0][1])]      # ONE call, the HBM arena
        assert calls[0][1] >= len(tens)
        for name, dt, shape, raw in tens:
            assert out[name].is_cuda
            if dt == "I64":
                assert_bits_equal(out[name], from_raw(raw, dt, shape))
            else:
                assert_bits_equal(out[name],
                                  expected(raw, dt, "BF16", shape), 0)
        del calls[:]
        got = f.get_tensor("emb", "cuda:0", torch.bfloat16, shard=(1, 1, 2))
        assert len(calls) == 1 and calls[0][0] == 0
        exp = torch.chunk(from_raw(emb.tobytes(), "F32", emb.shape), 2, 1)[1] \
            .contiguous().to(torch.bfloat16)
        assert_bits_equal(got, exp, 0)
        got = f.get_tensor("proj", "cuda:0", shard=(-1, 0, 3))
        assert_bits_equal(got, torch.chunk(
            from_raw(tens[2][3], "BF16", (300, 1026)), 3, 1)[0].contiguous())
        f.close()
        sf.shutdown()
    finally:
        smc.stop()
