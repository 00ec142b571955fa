"""Shared by the FP8 safetensors tests (CPU and GPU files): the reference
expressions, all torch on the CPU and never the code under test,

    s = w.float().abs().nan_to_num(nan=0, posinf=0, neginf=0).amax(...)
         .clamp(min=2**-40) / 448
    q = (w.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn)
    y = (q.float() * s).to(dst)

the same for flat element ranges with a group size (the arena-level
tests), and the expected file of save_file(quantize=...)."""
import numpy as np
import torch

from safetensors_cases import TORCH
from safetensors_save_cases import expected_file

F8 = torch.float8_e4m3fn
SOURCES = ("F32", "F16", "BF16")


def ref_scales(w, mode):
    """F32 scales of a cpu tensor: shape [1] ("tensor") or [shape[0], 1]
    ("row")."""
    a = w.float().abs().nan_to_num(nan=0, posinf=0, neginf=0)
    if mode == "tensor":
        amax = a.amax().reshape(1)
    else:
        amax = a.reshape(w.shape[0], -1).amax(dim=1, keepdim=True)
    return amax.clamp(min=2 ** -40) / 448


def _per_element(w, s):
    return s if s.numel() == 1 else s.reshape([-1] + [1] * (w.ndim - 1))


def ref_quant(w, s):
    return (w.float() / _per_element(w, s)).clamp(-448, 448).to(F8)


def ref_dequant(q, s, dst):
    return (q.float() * _per_element(q, s)).to(dst)


def flat_scales(x, every, e0=0):
    """Scales of the groups of a flat cpu tensor whose element 0 is dense
    element e0 of its tensor: group (e0 + i) // every (every 0: one
    group).  Returns the scale array indexed by group from group 0 (groups
    before e0's hold the floor) and the group index of every element."""
    n = x.numel()
    idx = (torch.arange(n) + e0) // every if every else \
        torch.zeros(n, dtype=torch.int64)
    a = x.float().abs().nan_to_num(nan=0, posinf=0, neginf=0)
    amax = torch.zeros(int(idx.max()) + 1 if n else 1)
    amax.scatter_reduce_(0, idx, a, "amax")
    return amax.clamp(min=2 ** -40) / 448, idx


def flat_quant(x, scales, idx):
    return (x.float() / scales[idx]).clamp(-448, 448).to(F8)


def flat_dequant(q, scales, idx, dst):
    return (q.float() * scales[idx]).to(dst)


def default_selected(name, t):
    return t.dtype in (torch.float32, torch.float16, torch.bfloat16) and \
        t.ndim >= 2 and t.numel() > 0


def expected_fp8_file(tensors, mode, metadata=None, selected=default_selected):
    """What save_file(quantize=mode) must write for {name: cpu tensor}:
    (file bytes, data_start, {name: stored cpu tensor}, names in order)."""
    stored = {}
    for name, t in tensors.items():
        if selected(name, t):
            s = ref_scales(t, mode)
            stored[name] = ref_quant(t, s)
            stored[name + "_scale"] = s
        else:
            stored[name] = t
    return expected_file(stored, metadata, None)


def random_weights(rng, dt, shape, spread=True):
    """finite values whose rows differ in magnitude by many binades, so a
    wrong row's scale cannot go unnoticed"""
    n = int(np.prod(shape))
    v = rng.standard_normal(n).astype(np.float32)
    if spread:
        v *= np.exp2(rng.integers(-12, 8, n)).astype(np.float32)
    t = torch.from_numpy(v).reshape(shape)
    if spread and len(shape) >= 2:
        rows = np.exp2(rng.integers(-6, 6, shape[0])).astype(np.float32)
        t = t * torch.from_numpy(rows).reshape([-1] + [1] * (len(shape) - 1))
    return t.to(TORCH[dt])
