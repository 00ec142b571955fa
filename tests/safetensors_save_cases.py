"""Shared by the safetensors save tests (CPU and GPU files): the expected
file, built here from the documented layout with json/struct and torch's
CPU `.to()` — never from the code under test — plus the finite random
generator and the block-level checks."""
import json
import struct

import numpy as np
import torch

from curvine_amd import native

from safetensors_cases import ISZ, TORCH

NAME = {v: k for k, v in TORCH.items()}
FLOATING = ("F32", "F16", "BF16", "F8_E4M3", "F8_E5M2", "F64")


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


def finite_tensor(rng, dt, shape):
    n = int(np.prod(shape)) if len(shape) else 1
    if n == 0:
        return torch.empty(shape, dtype=TORCH[dt])
    return torch.frombuffer(bytearray(finite_raw(rng, dt, n)),
                            dtype=TORCH[dt]).reshape(shape)


def raw_bytes(t) -> bytes:
    if t.numel() == 0:
        return b""
    return t.contiguous().view(-1).view(torch.uint8).numpy().tobytes()


def stored_name(t, dtype):
    src = NAME[t.dtype]
    return NAME[dtype] if dtype is not None and src in FLOATING else src


def expected_file(tensors, metadata=None, dtype=None):
    """tensors: {name: cpu tensor}.  Returns (file bytes, data_start,
    {name: expected stored cpu tensor}, names in file order)."""
    stored = {n: t.contiguous().to(TORCH[stored_name(t, dtype)])
              for n, t in tensors.items()}
    order = sorted(stored, key=lambda n: (-stored[n].element_size(), n))
    hdr, pos = {}, 0
    if metadata is not None:
        hdr["__metadata__"] = metadata
    for n in order:
        nb = stored[n].numel() * stored[n].element_size()
        hdr[n] = {"dtype": NAME[stored[n].dtype],
                  "shape": list(stored[n].shape),
                  "data_offsets": [pos, pos + nb]}
        pos += nb
    js = json.dumps(hdr, separators=(",", ":")).encode()
    while (8 + len(js)) % 64:
        js += b" "
    blob = struct.pack("<Q", len(js)) + js + \
        b"".join(raw_bytes(stored[n]) for n in order)
    return blob, 8 + len(js), stored, order


def block_crcs(smc, sf, path):
    """[(length, stored crc32c)] of the file's blocks, from the workers'
    block stores."""
    fb = sf.call(sf.fs.client.open(path))
    out = []
    for lb in fb.blocks:
        crcs = set()
        for w in smc.mc.workers:
            c = w.store.block_crc(lb.block.block_id)
            if c is not None:
                crcs.add(c)
        assert len(crcs) == 1, (lb.block.block_id, crcs)
        out.append((lb.block.length, crcs.pop()))
    return out


def check_file(smc, sf, path, blob):
    """Whole file through the ordinary byte read path, and every block's
    publish-time CRC against native.crc32c of the expected bytes."""
    got = sf.read_file(path)
    assert len(got) == len(blob)
    assert got == blob
    pos = 0
    for length, crc in block_crcs(smc, sf, path):
        assert crc == native.crc32c(blob[pos:pos + length]), pos
        pos += length
    assert pos == len(blob)
