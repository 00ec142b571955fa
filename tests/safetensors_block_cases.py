"""Shared by the block-scaled FP8 safetensors tests (CPU and GPU files): the
reference, all torch on the CPU and never the code under test.  For a
tensor w of shape (..., M, K) under bm x bn tiles,

    a = w.float().abs().nan_to_num(nan=0, posinf=0, neginf=0)
    s = amax of a over every tile (edge tiles: the elements that exist)
          .clamp(min=2**-40) / 448        shape (..., ceil(M/bm), ceil(K/bn))
    s_elem = s.repeat_interleave(bm, -2).repeat_interleave(bn, -1)
              trimmed to w's shape
    q = (w.float() / s_elem).clamp(-448, 448).to(torch.float8_e4m3fn)
    y = (q.float() * s_elem).to(dst)

and the expected file of save_file(quantize="block").  Comparisons made
with it are bitwise."""
import numpy as np
import torch

from safetensors_cases import TORCH
from safetensors_save_cases import expected_file

F8 = torch.float8_e4m3fn
SOURCES = ("F32", "F16", "BF16")
META_KEY = "weight_block_size"


def scale_shape(shape, block):
    bm, bn = block
    return tuple(shape[:-2]) + (-(-shape[-2] // bm), -(-shape[-1] // bn))


def ref_scales(w, block):
    """F32 tile scales of a cpu tensor (..., M, K)."""
    bm, bn = block
    m, k = w.shape[-2:]
    tm, tn = -(-m // bm), -(-k // bn)
    a = w.float().abs().nan_to_num(nan=0, posinf=0, neginf=0)
    # pad with zeros, which no amax notices (|x| >= 0)
    pad = torch.zeros(tuple(w.shape[:-2]) + (tm * bm, tn * bn))
    pad[..., :m, :k] = a
    amax = pad.reshape(tuple(w.shape[:-2]) + (tm, bm, tn, bn)) \
        .amax(dim=(-3, -1))
    return amax.clamp(min=2 ** -40) / 448


def per_element(s, shape, block):
    """the tile scale broadcast to the elements of a tensor of `shape`"""
    bm, bn = block
    return s.repeat_interleave(bm, -2).repeat_interleave(bn, -1)[
        ..., :shape[-2], :shape[-1]]


def ref_quant(w, s, block):
    return (w.float() / per_element(s, w.shape, block)) \
        .clamp(-448, 448).to(F8)


def ref_dequant(q, s, block, dst):
    return (q.float() * per_element(s, q.shape, block)).to(dst)


def default_selected(name, t):
    return t.dtype in (torch.float32, torch.float16, torch.bfloat16) and \
        t.ndim >= 2 and t.numel() > 0


def expected_block_file(tensors, block=(128, 128), metadata=None,
                        selected=default_selected):
    """What save_file(quantize="block", quantize_block=block) must write
    for {name: cpu tensor}: (file bytes, data_start, {name: stored cpu
    tensor}, names in order)."""
    stored = {}
    for name, t in tensors.items():
        if selected(name, t):
            s = ref_scales(t, block)
            stored[name] = ref_quant(t, s, block)
            stored[name + "_scale_inv"] = s
        else:
            stored[name] = t
    meta = dict(metadata or {})
    meta.setdefault(META_KEY, f"{block[0]},{block[1]}")
    return expected_file(stored, meta, None)


def random_weights(rng, dt, shape, block, spread=True):
    """finite values; every tile is scaled by its own power of two, many
    binades apart, so a scale taken from a neighbouring tile (or matrix)
    cannot go unnoticed"""
    v = torch.from_numpy(
        rng.standard_normal(int(np.prod(shape))).astype(np.float32)) \
        .reshape(shape)
    if spread:
        e = rng.integers(-10, 9, scale_shape(shape, block))
        v = v * per_element(torch.from_numpy(np.exp2(e).astype(np.float32)),
                            shape, block)
    return v.to(TORCH[dt])


def peaked_weights(dt, shape, block):
    """tile i holds small values and one maximum 2**(i % 24 - 12) * 1.5 at
    in-tile position i (row-major, taken modulo the tile's own extent), so
    across the tiles every lane of a unit and both sides of each unit and
    tile edge carry a maximum once"""
    bm, bn = block
    m, k = shape[-2:]
    w = torch.full(shape, 2.0 ** -16).reshape((-1, m, k))
    i = 0
    for b in range(w.shape[0]):
        for r0 in range(0, m, bm):
            for c0 in range(0, k, bn):
                h, wd = min(bm, m - r0), min(bn, k - c0)
                p = i % (h * wd)
                sign = -1.0 if i % 2 else 1.0
                w[b, r0 + p // wd, c0 + p % wd] = \
                    sign * 1.5 * 2.0 ** (i % 24 - 12)
                i += 1
    return w.reshape(shape).to(TORCH[dt])


def distinct_scales(w, block) -> int:
    return int(ref_scales(w, block).unique().numel())
