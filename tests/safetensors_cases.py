"""Shared builders for the safetensors tests (CPU and GPU files): hand-made
files, the exhaustive / crafted conversion inputs, and the bitwise
comparison with its NaN accounting.  Expected values always come from
torch on the CPU."""
import json
import struct

import numpy as np
import torch

TORCH = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16,
         "F8_E4M3": torch.float8_e4m3fn, "F8_E5M2": torch.float8_e5m2,
         "F64": torch.float64, "I64": torch.int64, "I32": torch.int32,
         "I16": torch.int16, "I8": torch.int8, "U8": torch.uint8,
         "BOOL": torch.bool}
ISZ = {"F32": 4, "F16": 2, "BF16": 2, "F8_E4M3": 1, "F8_E5M2": 1, "F64": 8,
       "I64": 8, "I32": 4, "I16": 2, "I8": 1, "U8": 1, "BOOL": 1}
INT_VIEW = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def build_file(tensors, metadata=None, data_start=None):
    """tensors: [(name, dtype_name, shape, raw_bytes)] -> (file bytes,
    data_start).  `data_start` pads the JSON with spaces so the data
    section begins exactly there (odd offsets included)."""
    hdr, pos = {}, 0
    if metadata is not None:
        hdr["__metadata__"] = metadata
    for name, dt, shape, raw in tensors:
        hdr[name] = {"dtype": dt, "shape": list(shape),
                     "data_offsets": [pos, pos + len(raw)]}
        pos += len(raw)
    js = json.dumps(hdr, separators=(",", ":")).encode()
    if data_start is not None:
        assert data_start >= 8 + len(js)
        js += b" " * (data_start - 8 - len(js))
    blob = struct.pack("<Q", len(js)) + js + b"".join(t[3] for t in tensors)
    return blob, 8 + len(js)


def raw_header(js: bytes, data: bytes = b"", n=None) -> bytes:
    return struct.pack("<Q", len(js) if n is None else n) + js + data


def from_raw(raw: bytes, dt: str, shape=None):
    t = torch.frombuffer(bytearray(raw), dtype=TORCH[dt]) if raw else \
        torch.empty(0, dtype=TORCH[dt])
    return t if shape is None else t.reshape(shape)


def expected(raw: bytes, src: str, dst: str, shape=None):
    return from_raw(raw, src, shape).to(TORCH[dst])


def assert_bits_equal(got, exp, n_nan_inputs=None):
    """Bitwise equality through integer views; NaN (and only NaN) is
    exempt from the bit match but must still be NaN, and the number of
    exempted elements must equal the number of NaN inputs."""
    got = got.detach().cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape
    if exp.numel() == 0:
        return
    if exp.dtype == torch.bool:
        got, exp = got.view(torch.uint8), exp.view(torch.uint8)
    iv = INT_VIEW[exp.element_size()]
    gi, ei = got.contiguous().view(iv), exp.contiguous().view(iv)
    if exp.is_floating_point():
        nan = torch.isnan(exp.float() if exp.element_size() < 4 else exp)
        gnan = torch.isnan(got.float() if got.element_size() < 4 else got)
    else:
        nan = torch.zeros(exp.shape, dtype=torch.bool)
        gnan = nan
    assert bool(gnan[nan].all()), "a NaN input did not give a NaN"
    bad = (gi != ei) & ~nan
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(
            f"{int(bad.sum())} elements differ; first at {i}: got "
            f"{int(gi.flatten()[i]):#x} expected {int(ei.flatten()[i]):#x}")
    if n_nan_inputs is not None:
        assert int(nan.sum()) == n_nan_inputs, \
            f"{int(nan.sum())} NaN exemptions for {n_nan_inputs} NaN inputs"


def count_nan_inputs(raw: bytes, src: str) -> int:
    """NaN inputs counted from the bit patterns, independently of torch's
    conversions."""
    if src == "F32":
        u = np.frombuffer(raw, dtype=np.uint32)
        return int(((u & 0x7FFFFFFF) > 0x7F800000).sum())
    if src == "F16":
        u = np.frombuffer(raw, dtype=np.uint16)
        return int(((u & 0x7FFF) > 0x7C00).sum())
    if src == "BF16":
        u = np.frombuffer(raw, dtype=np.uint16)
        return int(((u & 0x7FFF) > 0x7F80).sum())
    if src == "F8_E4M3":
        u = np.frombuffer(raw, dtype=np.uint8)
        return int(((u & 0x7F) == 0x7F).sum())
    if src == "F8_E5M2":
        u = np.frombuffer(raw, dtype=np.uint8)
        return int(((u & 0x7F) > 0x7C).sum())
    return 0


ALL16 = np.arange(65536, dtype=np.uint16).tobytes()
ALL8 = np.arange(256, dtype=np.uint8).tobytes()


def f32_bf16_edges() -> bytes:
    """every 16-bit high half x low halves {0,7FFF,8000,8001,FFFF}:
    bf16 ties, subnormals, the overflow edge (327,680 values)."""
    hi = np.arange(65536, dtype=np.uint32) << 16
    lo = np.array([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)
    return (hi[:, None] | lo[None, :]).reshape(-1).tobytes()


def f32_f16_edges() -> bytes:
    """f32 pattern of every finite f16 x plus {0,0FFF,1000,1001,1FFF}: f16
    ties and the 65520 overflow edge; then inputs whose rounded result is
    an f16 subnormal (2^-25 .. 2^-14, dense around every step, both
    signs) and the underflow-to-zero edge."""
    h = np.arange(65536, dtype=np.uint16)
    fin = h[(h & 0x7C00) != 0x7C00]
    f = torch.frombuffer(bytearray(fin.tobytes()), dtype=torch.float16) \
        .float().view(torch.int32).numpy().astype(np.uint32)
    add = np.array([0, 0x0FFF, 0x1000, 0x1001, 0x1FFF], dtype=np.uint32)
    main = (f[:, None] + add[None, :]).reshape(-1)
    # f16 subnormal k*2^-24 and its half-way points (k+0.5)*2^-24, +-1 ulp
    k = np.arange(0, 2050, dtype=np.float64) / 2.0          # 0, .5, 1 ...
    centre = (k * 2.0 ** -24).astype(np.float32).view(np.uint32)
    sub = (centre[:, None] + np.array([-1, 0, 1], dtype=np.int64)[None, :]) \
        .reshape(-1)
    sub = sub[(sub >= 0) & (sub < 0x7F800000)].astype(np.uint32)
    sub = np.concatenate([sub, sub | np.uint32(0x80000000)])
    return np.concatenate([main, sub]).astype(np.uint32).tobytes()


# (src, dst, raw bytes) for every exhaustive / crafted set of the issue
def conversion_sets():
    sets = [("BF16", "F16", ALL16), ("BF16", "F32", ALL16),
            ("F16", "BF16", ALL16), ("F16", "F32", ALL16)]
    for s in ("F8_E4M3", "F8_E5M2"):
        for d in ("F32", "F16", "BF16"):
            sets.append((s, d, ALL8))
    e1, e2 = f32_bf16_edges(), f32_f16_edges()
    for d in ("BF16", "F16"):
        sets.append(("F32", d, e1))
        sets.append(("F32", d, e2))
    return sets
