"""Shared by the MX safetensors tests (CPU and GPU files): the reference for
the E8M0 scale rule, the single-rounding quantise and dequantise and the
expected file.  Everything here is numpy float64 (every product with a
power of two is exact there) and torch's CPU casts — never the code under
test.  Comparisons made with it are bitwise."""
import json
import struct

import numpy as np
import torch

STORED = {"mxfp8": "F8_E4M3", "mxfp4": "F4"}
EMAX = {"F8_E4M3": 8, "F4": 2}
MBITS = {"F8_E4M3": 3, "F4": 1}
EMIN = {"F8_E4M3": -6, "F4": 0}
FMAX = {"F8_E4M3": 448.0, "F4": 6.0}
BITS = {"F32": 32, "F16": 16, "BF16": 16, "F8_E4M3": 8, "F8_E8M0": 8,
        "F4": 4, "I64": 64, "U8": 8}
SOURCES = ("F32", "F16", "BF16")
TDT = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16}
BLOCK = 32


def _e4m3_table():
    out = np.zeros(128)
    for c in range(128):
        e, m = c >> 3, c & 7
        out[c] = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
    out[127] = np.nan
    return out


# magnitude of every non-negative code
TABLE = {"F8_E4M3": _e4m3_table(),
         "F4": np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=np.float64)}
SIGN = {"F8_E4M3": 0x80, "F4": 0x8}


def widen(t) -> np.ndarray:
    """a cpu F32/F16/BF16 tensor as float64, exactly"""
    return t.detach().double().numpy()


def ref_scales(x64, stored: str) -> np.ndarray:
    """E8M0 bytes of x64 (..., K): one per 32 consecutive elements of the
    last dimension, from the biased f32 exponent of the largest finite
    |x|."""
    a = np.abs(x64)
    a = np.where(np.isfinite(a), a, 0.0)
    amax = a.reshape(a.shape[:-1] + (a.shape[-1] // BLOCK, BLOCK)).max(-1)
    e = (amax.astype(np.float32).view(np.uint32) >> 23) & 0xFF
    return np.maximum(e.astype(np.int64) - EMAX[stored], 0).astype(np.uint8)


def per_element(scales, shape):
    """the scale byte of every element of a tensor of `shape`"""
    return np.repeat(scales, BLOCK, axis=-1).reshape(shape)


def ref_quant(x64, s, stored: str) -> np.ndarray:
    """element codes (one per uint8, unpacked) of x64 under the per-element
    scale bytes `s`: x * 2**(127-s) rounded once, ties to even, saturating"""
    mb, emin, top = MBITS[stored], EMIN[stored], FMAX[stored]
    x64 = np.asarray(x64, dtype=np.float64)
    v = np.abs(x64) * np.exp2(127.0 - s.astype(np.float64))
    nan, inf = np.isnan(x64), np.isinf(x64)
    fin = np.where(nan | inf, 0.0, v)
    _, ex = np.frexp(fin)                       # fin = m * 2**ex, m in [.5,1)
    q = np.exp2((np.maximum(ex - 1, emin) - mb).astype(np.float64))
    r = np.minimum(np.rint(fin / q) * q, top)
    r = np.where(inf, top, r)
    table = TABLE[stored][:127] if stored == "F8_E4M3" else TABLE[stored]
    code = np.searchsorted(table, r)
    assert (table[code] == r).all()
    if stored == "F8_E4M3":
        code = np.where(nan, 0x7F, code)
    else:
        code = np.where(nan | inf, 7, code)
    return (code | np.where(np.signbit(x64), SIGN[stored], 0)).astype(np.uint8)


def pack(codes, stored: str) -> bytes:
    """file bytes of unpacked codes: F4 two per byte, even element low"""
    c = np.ascontiguousarray(codes).reshape(-1)
    if stored == "F4":
        c = c[0::2] | (c[1::2] << 4)
    return c.astype(np.uint8).tobytes()


def unpack(raw, stored: str) -> np.ndarray:
    b = np.frombuffer(raw, dtype=np.uint8)
    if stored == "F4":
        return np.stack([b & 0xF, b >> 4], axis=-1).reshape(-1)
    return b.copy()


def ref_dequant(codes, s, stored: str, dtype):
    """value(code) * 2**(s-127) as an exact float64, cast once by torch on
    the CPU; s == 255 and the E4M3 NaN give NaN"""
    sign = SIGN[stored]
    mag = TABLE[stored][codes & (sign - 1)]
    val = np.where(codes & sign, -mag, mag)
    sc = np.exp2(np.where(s == 255, 0, s).astype(np.float64) - 127.0)
    y = np.where(s == 255, np.nan, val * sc)
    return torch.from_numpy(np.ascontiguousarray(y)).to(dtype)


def count_nan(codes, s, stored: str) -> int:
    nan = s == 255
    if stored == "F8_E4M3":
        nan = nan | ((codes & 0x7F) == 0x7F)
    return int(np.broadcast_to(nan, np.broadcast(codes, s).shape).sum())


def random_weights(rng, src: str, shape, spread=True):
    """finite values with block maxima spread over many binades"""
    x = rng.standard_normal(shape)
    if spread and len(shape):
        k = shape[-1]
        e = rng.integers(-12, 9, size=int(np.prod(shape)) // k * -(-k // BLOCK))
        x = x * np.repeat(np.exp2(e.astype(np.float64)), BLOCK) \
            .reshape(shape[:-1] + (-1,))[..., :k]
    return torch.from_numpy(x).to(TDT[src])


def raw_bytes(t) -> bytes:
    if t.numel() == 0:
        return b""
    return t.contiguous().view(-1).view(torch.uint8).numpy().tobytes()


def mx_default(name, t) -> bool:
    return t.is_floating_point() and t.element_size() in (2, 4) and \
        t.ndim >= 2 and t.numel() > 0 and t.shape[-1] % BLOCK == 0


def expected_mx_file(tensors, mode: str, metadata=None, select=mx_default,
                     names=None):
    """tensors: {name: cpu tensor}, `names` the safetensors dtype of the
    unselected ones.  Returns (file bytes, data_start, {name: (dtype,
    shape, raw bytes, codes or None)}, names in file order)."""
    stored = STORED[mode]
    names = names or {torch.float32: "F32", torch.float16: "F16",
                      torch.bfloat16: "BF16", torch.int64: "I64",
                      torch.uint8: "U8"}
    ent = {}
    for n, t in tensors.items():
        if select(n, t):
            x = widen(t)
            s = ref_scales(x, stored)
            codes = ref_quant(x, per_element(s, x.shape), stored)
            ent[n] = (stored, tuple(t.shape), pack(codes, stored), codes)
            ent[n + "_scale"] = ("F8_E8M0", s.shape, s.tobytes(), s)
        else:
            ent[n] = (names[t.dtype], tuple(t.shape), raw_bytes(t), None)
    order = sorted(ent, key=lambda n: (-BITS[ent[n][0]], n))
    hdr, pos = {}, 0
    if metadata is not None:
        hdr["__metadata__"] = metadata
    for n in order:
        dt, shape, raw, _ = ent[n]
        hdr[n] = {"dtype": dt, "shape": list(shape),
                  "data_offsets": [pos, pos + len(raw)]}
        pos += len(raw)
    js = json.dumps(hdr, separators=(",", ":")).encode()
    js += b" " * (-(8 + len(js)) % 64)
    blob = struct.pack("<Q", len(js)) + js + b"".join(ent[n][2] for n in order)
    return blob, 8 + len(js), ent, order
