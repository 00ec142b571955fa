"""The exact ValueError text of every argument check of the typed load,
store and scale entry points, on a host arena and with device -1: one row
per check, reached through each entry point that can reach it, plus rows
that break two rules at once and pin which error wins.  Every list puts a
good segment in front of the bad one, and nothing may have been written
when the call is refused."""
import numpy as np
import pytest
import torch

from curvine_amd import native

D = native.DTYPES
F32, F16, BF16, F8, E5M2, F64, F4 = (D[k] for k in (
    "F32", "F16", "BF16", "F8_E4M3", "F8_E5M2", "F64", "F4"))
U = 2 ** 64 - 1
BIG = 2 ** 33
CAP = 4096
SENTINEL = 0xAB

# host memory the segments point at: 64 f32 sources, a 256-byte destination,
# 8 f32 scales and 8 E8M0 scale bytes
X = torch.ones(64)
DST = torch.full((256,), 7, dtype=torch.uint8)
S = torch.ones(8)
E = torch.full((8,), 127, dtype=torch.uint8)
P, DP, Q, EP = X.data_ptr(), DST.data_ptr(), S.data_ptr(), E.data_ptr()


@pytest.fixture(scope="module")
def arena():
    a = native.Arena(-1, CAP)
    a.fill(0, CAP, SENTINEL)
    yield a
    a.close()


# field names and a good segment per entry point
FAMILIES = {
    "convert7": ("a b rows run pitch sdt ddt", (0, DP, 1, 16, 64, F32, F16)),
    "convert10": ("a b rows run pitch sdt ddt sp every e0",
                  (0, DP, 1, 16, 16, F8, F32, Q, 4, 0)),
    "store7": ("a b rows run pitch sdt ddt", (P, 0, 1, 16, 64, F32, F16)),
    "store10": ("a b rows run pitch sdt ddt sp every e0",
                (P, 0, 1, 16, 64, F32, F8, Q, 4, 0)),
    "absmax": ("src rows run pitch sdt out every e0 n",
               (P, 1, 16, 64, F32, Q, 4, 0, 4)),
    "mxstore": ("a b rows run pitch sdt ddt sp e0 spitch blk",
                (P, 0, 1, 32, 128, F32, F8, EP, 0, 32, 32)),
    "mxconvert": ("a b rows run pitch sdt ddt sp e0 spitch blk",
                  (0, DP, 1, 32, 32, F8, F32, EP, 0, 32, 32)),
    "mxscales": ("src rows run pitch sdt ddt out",
                 (P, 1, 32, 128, F32, F8, EP)),
    "blockstore": ("a b rows run pitch sdt ddt sp e0 spitch M K bm bn",
                   (P, 0, 1, 64, 256, F32, F8, Q, 0, 64, 4, 16, 2, 8)),
    "blockconvert": ("a b rows run pitch sdt ddt sp e0 spitch M K bm bn",
                     (0, DP, 1, 64, 64, F8, F32, Q, 0, 64, 4, 16, 2, 8)),
    "blockabsmax": ("src rows run pitch sdt out e0 spitch M K bm bn n",
                    (P, 1, 64, 256, F32, Q, 0, 64, 4, 16, 2, 8, 4)),
}
WHO = {"convert7": "convert", "convert10": "convert", "store7": "store",
       "store10": "store", "absmax": "absmax", "mxstore": "mx store",
       "mxconvert": "mx convert", "mxscales": "mx scales",
       "blockstore": "block store", "blockconvert": "block convert",
       "blockabsmax": "block absmax"}


def seg(family, **kw):
    names, good = FAMILIES[family]
    names = names.split()
    assert set(kw) <= set(names), kw
    return tuple(kw.get(n, v) for n, v in zip(names, good))


def call(arena, family, segs, device=-1):
    if family.startswith(("convert", "mxconvert", "blockconvert")):
        arena.convert_ptr(segs)
    elif family.endswith(("store7", "store10", "mxstore", "blockstore")):
        arena.store_ptr(segs)
    elif family == "absmax":
        native.absmax_scales(device, segs)
    elif family == "mxscales":
        native.mx_scales(device, segs)
    else:
        native.block_absmax_scales(device, segs)


TWO33 = dict(rows=BIG, run=BIG)
# (family, changed fields, message after "<who>: ")
SEGMENT_ROWS = [
    # ---- typed load, 7- and 10-tuples
    ("convert7", dict(sdt=15), "unknown dtype code"),
    ("convert7", dict(ddt=99), "unknown dtype code"),
    ("convert7", TWO33, "segment size overflows"),
    ("convert10", dict(sdt=F32, ddt=F16), "scale_ptr on a dtype pair that takes none"),
    ("convert10", dict(sdt=F32, ddt=F8), "scale_ptr on a dtype pair that takes none"),
    ("convert10", dict(sp=Q + 1), "scale_ptr misaligned"),
    ("convert10", dict(e0=U), "scale range overflows"),
    ("convert10", dict(sp=U - 3, every=0), "scale range overflows"),
    ("convert7", dict(sdt=F64, ddt=F32), "unsupported dtype pair"),
    ("convert7", dict(sdt=F32, ddt=F8), "unsupported dtype pair"),
    ("convert10", dict(sdt=F32, ddt=F8, sp=0), "unsupported dtype pair"),
    ("convert7", dict(run=2 ** 62), "segment size overflows"),
    ("convert7", dict(b=U - 1), "segment size overflows"),
    ("convert7", dict(a=U), "segment range overflows"),
    ("convert7", dict(rows=2, pitch=U), "segment range overflows"),
    ("convert7", dict(a=CAP - 8), "arena range out of bounds"),
    ("convert7", dict(rows=2, pitch=CAP), "arena range out of bounds"),
    ("convert7", dict(b=0), "dst_ptr null or misaligned"),
    ("convert7", dict(b=DP + 1), "dst_ptr null or misaligned"),
    ("convert10", dict(b=DP + 2), "dst_ptr null or misaligned"),
    # two rules at once
    ("convert7", dict(sdt=15, a=CAP), "unknown dtype code"),
    ("convert7", dict(a=CAP, b=0), "arena range out of bounds"),
    ("convert10", dict(sp=Q + 1, a=CAP), "scale_ptr misaligned"),
    ("convert10", dict(sdt=F32, ddt=F16, sp=Q + 1),
     "scale_ptr on a dtype pair that takes none"),
    ("convert7", dict(sdt=F64, ddt=F32, a=CAP), "unsupported dtype pair"),
    ("convert7", dict(a=U, b=U - 1), "segment size overflows"),
    # ---- typed store, 7- and 10-tuples
    ("store7", dict(sdt=15), "unknown dtype code"),
    ("store7", dict(ddt=15), "unknown dtype code"),
    ("store7", TWO33, "segment size overflows"),
    ("store7", dict(ddt=F8), "unsupported dtype pair without a scale_ptr"),
    ("store10", dict(sdt=F8, ddt=F32), "scale_ptr on a dtype pair that takes none"),
    ("store10", dict(ddt=F16), "scale_ptr on a dtype pair that takes none"),
    ("store10", dict(sp=Q + 2), "scale_ptr misaligned"),
    ("store10", dict(e0=U), "scale range overflows"),
    ("store10", dict(sp=U - 3, every=0), "scale range overflows"),
    ("store7", dict(sdt=F64, ddt=F32), "unsupported dtype pair"),
    ("store7", dict(run=2 ** 62), "segment size overflows"),
    ("store7", dict(b=U - 1), "segment size overflows"),
    ("store7", dict(b=CAP - 8), "arena range out of bounds"),
    ("store7", dict(rows=0, b=CAP + 2), "arena range out of bounds"),
    ("store7", dict(a=U - 3), "source range overflows"),
    ("store7", dict(rows=2, pitch=U), "source range overflows"),
    ("store7", dict(a=0), "src_ptr null or misaligned"),
    ("store7", dict(a=P + 2), "src_ptr null or misaligned"),
    ("store7", dict(b=1), "dst_off misaligned"),
    ("store7", dict(sdt=15, b=CAP), "unknown dtype code"),
    ("store7", dict(a=0, b=CAP), "arena range out of bounds"),
    ("store7", dict(a=0, b=1), "src_ptr null or misaligned"),
    ("store10", dict(sp=Q + 2, a=0), "scale_ptr misaligned"),
    ("store7", dict(ddt=F8, b=CAP), "unsupported dtype pair without a scale_ptr"),
    # ---- group scales
    ("absmax", dict(sdt=F8), "source dtype is not F32/F16/BF16"),
    ("absmax", TWO33, "segment size overflows"),
    ("absmax", dict(e0=U), "segment size overflows"),
    ("absmax", dict(n=2 ** 62), "segment size overflows"),
    ("absmax", dict(out=U - 3), "segment size overflows"),
    ("absmax", dict(out=0), "out_ptr null, misaligned or empty"),
    ("absmax", dict(out=Q + 2), "out_ptr null, misaligned or empty"),
    ("absmax", dict(n=0), "out_ptr null, misaligned or empty"),
    ("absmax", dict(src=U - 3), "source range overflows"),
    ("absmax", dict(rows=2, pitch=U), "source range overflows"),
    ("absmax", dict(src=0), "src_ptr null or misaligned"),
    ("absmax", dict(src=P + 1), "src_ptr null or misaligned"),
    ("absmax", dict(n=2), "groups pass n_groups"),
    ("absmax", dict(every=0, e0=5, n=1, out=0), "out_ptr null, misaligned or empty"),
    ("absmax", dict(sdt=F8, out=0), "source dtype is not F32/F16/BF16"),
    ("absmax", dict(out=0, src=0), "out_ptr null, misaligned or empty"),
    ("absmax", dict(src=0, n=2), "src_ptr null or misaligned"),
    # ---- MX store
    ("mxstore", dict(blk=16), "block size is not 32"),
    ("mxstore", dict(sdt=F8), "not F32/F16/BF16 on the wide side"),
    ("mxstore", dict(ddt=E5M2), "stored dtype is not F8_E4M3 or F4"),
    ("mxstore", TWO33, "segment size overflows"),
    ("mxstore", dict(run=2 ** 62), "segment size overflows"),
    ("mxstore", dict(ddt=F4, run=31), "F4 piece splits a byte"),
    ("mxstore", dict(ddt=F4, e0=1), "F4 piece splits a byte"),
    ("mxstore", dict(ddt=F4, rows=2, run=16, pitch=64, spitch=17),
     "F4 piece splits a byte"),
    ("mxstore", dict(sp=0), "scale_ptr is null"),
    ("mxstore", dict(e0=U), "scale range overflows"),
    ("mxstore", dict(sp=U), "scale range overflows"),
    ("mxstore", dict(a=U - 3), "source range overflows"),
    ("mxstore", dict(rows=2, pitch=64), "rows overlap"),
    ("mxstore", dict(a=0), "src_ptr null or misaligned"),
    ("mxstore", dict(a=P + 2), "src_ptr null or misaligned"),
    ("mxstore", dict(b=CAP - 8), "arena range out of bounds"),
    ("mxstore", dict(b=U), "arena range out of bounds"),
    ("mxstore", dict(blk=16, sdt=F8), "block size is not 32"),
    ("mxstore", dict(sp=0, a=P + 2), "scale_ptr is null"),
    ("mxstore", dict(a=0, b=CAP), "src_ptr null or misaligned"),
    ("mxstore", dict(rows=2, pitch=64, a=0), "rows overlap"),
    # ---- MX load
    ("mxconvert", dict(blk=0), "block size is not 32"),
    ("mxconvert", dict(ddt=F64), "not F32/F16/BF16 on the wide side"),
    ("mxconvert", dict(sdt=F32), "stored dtype is not F8_E4M3 or F4"),
    ("mxconvert", TWO33, "segment size overflows"),
    ("mxconvert", dict(sdt=F4, run=31), "F4 piece splits a byte"),
    ("mxconvert", dict(sp=0), "scale_ptr is null"),
    ("mxconvert", dict(e0=U), "scale range overflows"),
    ("mxconvert", dict(a=U), "source range overflows"),
    ("mxconvert", dict(rows=2, pitch=16), "rows overlap"),
    ("mxconvert", dict(a=CAP - 8), "arena range out of bounds"),
    ("mxconvert", dict(b=0), "dst_ptr null, misaligned or overflowing"),
    ("mxconvert", dict(b=DP + 2), "dst_ptr null, misaligned or overflowing"),
    ("mxconvert", dict(b=U - 3), "dst_ptr null, misaligned or overflowing"),
    ("mxconvert", dict(a=CAP, b=0), "arena range out of bounds"),
    ("mxconvert", dict(sp=0, a=CAP), "scale_ptr is null"),
    # ---- MX scales
    ("mxscales", dict(sdt=F8), "not F32/F16/BF16 on the wide side"),
    ("mxscales", dict(ddt=E5M2), "stored dtype is not F8_E4M3 or F4"),
    ("mxscales", TWO33, "segment size overflows"),
    ("mxscales", dict(run=16), "not whole blocks of 32"),
    ("mxscales", dict(ddt=F4, run=48, pitch=192), "not whole blocks of 32"),
    ("mxscales", dict(ddt=F4, run=31), "F4 piece splits a byte"),
    ("mxscales", dict(out=0), "scale_ptr is null"),
    ("mxscales", dict(out=U), "scale range overflows"),
    ("mxscales", dict(src=U - 3), "source range overflows"),
    ("mxscales", dict(rows=2, pitch=64), "rows overlap"),
    ("mxscales", dict(src=0), "src_ptr null or misaligned"),
    ("mxscales", dict(src=P + 2), "src_ptr null or misaligned"),
    ("mxscales", dict(out=0, src=0), "scale_ptr is null"),
    ("mxscales", dict(run=16, out=0), "not whole blocks of 32"),
    # ---- block store
    ("blockstore", dict(sdt=F8), "not F32/F16/BF16 on the wide side"),
    ("blockstore", dict(ddt=F4), "stored dtype is not F8_E4M3"),
    ("blockstore", dict(M=0), "M, K, bm and bn must be positive"),
    ("blockstore", dict(bn=0), "M, K, bm and bn must be positive"),
    ("blockstore", TWO33, "segment size overflows"),
    ("blockstore", dict(run=2 ** 62), "segment size overflows"),
    ("blockstore", dict(sp=0), "scale_ptr null or misaligned"),
    ("blockstore", dict(sp=Q + 2), "scale_ptr null or misaligned"),
    ("blockstore", dict(rows=2, run=16, pitch=64, spitch=8),
     "rows overlap in the tensor"),
    ("blockstore", dict(e0=U), "scale range overflows"),
    ("blockstore", dict(sp=U - 3), "scale range overflows"),
    ("blockstore", dict(a=U - 3), "source range overflows"),
    ("blockstore", dict(rows=2, run=16, pitch=32, spitch=16),
     "rows overlap or pitch misaligned"),
    ("blockstore", dict(rows=2, run=16, pitch=66, spitch=16),
     "rows overlap or pitch misaligned"),
    ("blockstore", dict(a=0), "src_ptr null or misaligned"),
    ("blockstore", dict(a=P + 2), "src_ptr null or misaligned"),
    ("blockstore", dict(b=CAP - 8), "arena range out of bounds"),
    ("blockstore", dict(b=U), "arena range out of bounds"),
    ("blockstore", dict(sp=0, a=P + 2), "scale_ptr null or misaligned"),
    ("blockstore", dict(M=0, sdt=F8), "not F32/F16/BF16 on the wide side"),
    ("blockstore", dict(a=0, b=CAP), "src_ptr null or misaligned"),
    # ---- block load
    ("blockconvert", dict(ddt=F64), "not F32/F16/BF16 on the wide side"),
    ("blockconvert", dict(sdt=F32), "stored dtype is not F8_E4M3"),
    ("blockconvert", dict(K=0), "M, K, bm and bn must be positive"),
    ("blockconvert", TWO33, "segment size overflows"),
    ("blockconvert", dict(sp=Q + 1), "scale_ptr null or misaligned"),
    ("blockconvert", dict(rows=2, run=16, pitch=16, spitch=8),
     "rows overlap in the tensor"),
    ("blockconvert", dict(e0=U), "scale range overflows"),
    ("blockconvert", dict(a=U), "source range overflows"),
    ("blockconvert", dict(rows=2, run=16, pitch=8, spitch=16),
     "rows overlap or pitch misaligned"),
    ("blockconvert", dict(a=CAP - 8), "arena range out of bounds"),
    ("blockconvert", dict(b=0), "dst_ptr null, misaligned or overflowing"),
    ("blockconvert", dict(b=DP + 2), "dst_ptr null, misaligned or overflowing"),
    ("blockconvert", dict(b=U - 3), "dst_ptr null, misaligned or overflowing"),
    ("blockconvert", dict(a=CAP, b=0), "arena range out of bounds"),
    ("blockconvert", dict(sp=0, a=CAP), "scale_ptr null or misaligned"),
    # ---- block tile scales
    ("blockabsmax", dict(out=0), "out_ptr null, misaligned, empty or overflowing"),
    ("blockabsmax", dict(out=Q + 2), "out_ptr null, misaligned, empty or overflowing"),
    ("blockabsmax", dict(n=0), "out_ptr null, misaligned, empty or overflowing"),
    ("blockabsmax", dict(n=2 ** 62), "out_ptr null, misaligned, empty or overflowing"),
    ("blockabsmax", dict(out=U - 3), "out_ptr null, misaligned, empty or overflowing"),
    ("blockabsmax", dict(sdt=F8), "not F32/F16/BF16 on the wide side"),
    ("blockabsmax", dict(bm=0), "M, K, bm and bn must be positive"),
    ("blockabsmax", TWO33, "segment size overflows"),
    ("blockabsmax", dict(rows=2, run=16, pitch=64, spitch=8),
     "rows overlap in the tensor"),
    ("blockabsmax", dict(e0=U), "scale range overflows"),
    ("blockabsmax", dict(n=2), "tiles pass the scales given"),
    ("blockabsmax", dict(e0=64), "tiles pass the scales given"),
    ("blockabsmax", dict(src=U - 3), "source range overflows"),
    ("blockabsmax", dict(rows=2, run=16, pitch=32, spitch=16),
     "rows overlap or pitch misaligned"),
    ("blockabsmax", dict(src=0), "src_ptr null or misaligned"),
    ("blockabsmax", dict(out=0, sdt=F8), "out_ptr null, misaligned, empty or overflowing"),
    ("blockabsmax", dict(n=2, src=0), "tiles pass the scales given"),
]


def untouched(arena):
    assert arena.read_bytes(0, CAP) == bytes([SENTINEL]) * CAP
    assert torch.equal(DST, torch.full((256,), 7, dtype=torch.uint8))
    assert torch.equal(S, torch.ones(8))
    assert torch.equal(E, torch.full((8,), 127, dtype=torch.uint8))
    assert torch.equal(X, torch.ones(64))


@pytest.mark.parametrize(
    "family,changed,message", SEGMENT_ROWS,
    ids=[f"{i}-{r[0]}-{'-'.join(r[1])}" for i, r in enumerate(SEGMENT_ROWS)])
def test_segment_refused(arena, family, changed, message):
    with pytest.raises(ValueError) as ei:
        call(arena, family, [seg(family), seg(family, **changed)])
    assert str(ei.value) == f"{WHO[family]}: {message}"
    untouched(arena)


@pytest.mark.parametrize("fn,who", [(native.absmax_scales, "absmax"),
                                    (native.mx_scales, "mx scales"),
                                    (native.block_absmax_scales,
                                     "block absmax")])
def test_bad_device(arena, fn, who):
    family = {"absmax": "absmax", "mx scales": "mxscales",
              "block absmax": "blockabsmax"}[who]
    # the device is looked at first: before any segment, good or bad
    for segs in ([], [seg(family)], [seg(family, src=0)]):
        with pytest.raises(ValueError) as ei:
            fn(-2, segs)
        assert str(ei.value) == f"{who}: bad device"
    untouched(arena)


def test_empty_segments(arena):
    """The load leaves the range of a segment without elements alone, the
    store checks its destination all the same; segments without elements
    are accepted wherever their arguments are."""
    arena.convert_ptr([(10 ** 9, 0, 0, 16, 0, F32, F16)])
    arena.convert_ptr([seg("mxconvert", rows=0, a=10 ** 9, b=0, sp=0)])
    arena.convert_ptr([seg("blockconvert", run=0, a=10 ** 9, b=0, sp=0)])
    arena.store_ptr([seg("store7", rows=0, a=0, b=CAP)])
    arena.store_ptr([seg("mxstore", rows=0, a=0, b=10 ** 9, sp=0)])
    arena.store_ptr([seg("blockstore", run=0, a=0, b=10 ** 9, sp=0)])
    native.mx_scales(-1, [seg("mxscales", rows=0, src=0, out=0)])
    untouched(arena)


def f8(n):
    return bytes(n)


def f32(n):
    return np.ones(n, dtype=np.float32)


# (function, arguments, whole message)
HOST_ROWS = [
    (native.convert_host, (f32(16), 15, F16, 16), "convert: unknown dtype code"),
    (native.convert_host, (f32(16), F32, 15, 16), "convert: unknown dtype code"),
    (native.convert_host, (f32(16), F32, F8, 16),
     "convert: unsupported dtype pair without a scale_ptr"),
    (native.convert_host, (f32(16), F32, F16, 16, f32(4), 4, 0),
     "convert: scale_ptr on a dtype pair that takes none"),
    (native.convert_host, (f8(16), F8, F32, 16, f32(0), 4, 0),
     "convert: scales empty or misaligned"),
    (native.convert_host, (f8(16), F8, F32, 16, f32(1), 4, 0),
     "convert: scales shorter than the groups"),
    (native.convert_host, (f8(16), F8, F32, 16, f32(1), 4, U),
     "convert: scales shorter than the groups"),
    (native.convert_host, (f8(16), F8, F32, 16, f32(1), 0, U - 15),
     "convert: scale range overflows"),
    (native.convert_host, (f8(16), F8, F32, 2 ** 41),
     "convert: segment size overflows"),
    (native.convert_host, (f8(16), F8, F32, 2 ** 63),
     "convert: segment size overflows"),
    (native.convert_host, (np.ones(4), F64, F32, 4),
     "convert: unsupported dtype pair"),
    (native.convert_host, (f32(2), F32, F16, 16),
     "convert: arena range out of bounds"),
    # two rules: short scales and a pair that takes none; short source and
    # an unsupported pair
    (native.convert_host, (f32(16), F32, F16, 16, f32(1), 4, 0),
     "convert: scales shorter than the groups"),
    (native.convert_host, (np.ones(1), F64, F32, 4),
     "convert: unsupported dtype pair"),
    (native.mx_convert_host, (f32(32), F32, F32, 32, f8(1), 0),
     "mx convert: stored dtype is not F8_E4M3 or F4"),
    (native.mx_convert_host, (f8(32), F8, F8, 32, f8(1), 0),
     "mx convert: not F32/F16/BF16 on the wide side"),
    (native.mx_convert_host, (f8(32), F64, F32, 32, f8(1), 0),
     "mx convert: stored dtype is not F8_E4M3 or F4"),
    (native.mx_convert_host, (f32(31), F32, F4, 31, f8(1), 0),
     "mx convert: F4 piece splits a byte"),
    (native.mx_convert_host, (f8(16), F4, F32, 32, f8(1), 1),
     "mx convert: F4 piece splits a byte"),
    (native.mx_convert_host, (f32(32), F32, F8, 32, f8(1), U),
     "mx convert: scale range overflows"),
    (native.mx_convert_host, (f32(16), F32, F8, 32, f8(1), 0),
     "mx convert: source shorter than n"),
    (native.mx_convert_host, (f8(16), F8, F32, 32, f8(1), 0),
     "mx convert: arena range out of bounds"),
    (native.mx_convert_host, (f32(32), F32, F8, 32, f8(1), 16),
     "mx convert: scales shorter than the blocks"),
    (native.mx_convert_host, (f8(32), F8, BF16, 32, f8(1), 1),
     "mx convert: scales shorter than the blocks"),
    (native.mx_convert_host, (f32(16), F32, F8, 32, f8(0), 16),
     "mx convert: source shorter than n"),
    (native.block_convert_host, (f32(64), F32, F32, 64, f32(4), 0, 4, 16, 2, 8),
     "block convert: stored dtype is not F8_E4M3"),
    (native.block_convert_host, (f8(64), F8, F8, 64, f32(4), 0, 4, 16, 2, 8),
     "block convert: not F32/F16/BF16 on the wide side"),
    (native.block_convert_host, (f32(64), F32, F8, 64, f32(4), 0, 0, 16, 2, 8),
     "block convert: M, K, bm and bn must be positive"),
    (native.block_convert_host, (f32(64), F32, F8, 64, f32(4), U, 4, 16, 2, 8),
     "block convert: scale range overflows"),
    (native.block_convert_host, (f32(32), F32, F8, 64, f32(4), 0, 4, 16, 2, 8),
     "block convert: source shorter than n"),
    (native.block_convert_host, (f8(32), F8, F32, 64, f32(4), 0, 4, 16, 2, 8),
     "block convert: arena range out of bounds"),
    (native.block_convert_host, (f32(64), F32, F8, 64, f32(3), 0, 4, 16, 2, 8),
     "block convert: scales do not cover the tiles"),
    (native.block_convert_host,
     (f8(32), F8, F16, 32, f32(2), 32, 4, 16, 2, 8, 3),
     "block convert: scales do not cover the tiles"),
    (native.block_convert_host, (f32(32), F32, F8, 64, f32(1), 0, 4, 16, 2, 8),
     "block convert: source shorter than n"),
]


@pytest.mark.parametrize(
    "fn,args,message", HOST_ROWS,
    ids=[f"{i}-{r[0].__name__}" for i, r in enumerate(HOST_ROWS)])
def test_host_convert_refused(fn, args, message):
    with pytest.raises(ValueError) as ei:
        fn(*args)
    assert str(ei.value) == message
