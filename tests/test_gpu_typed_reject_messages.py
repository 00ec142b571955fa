"""The device-range checks of the typed load, store and scale entry points
on the MI355X, by their exact ValueError text, once per entry point: a
host pointer where the kernel needs device memory, and a range that starts
inside a 128-element tensor and runs past its allocation.  Every call is
refused on the host before any launch, behind a good segment, and nothing
is written."""
import pytest
import torch

from curvine_amd import native

pytestmark = pytest.mark.gpu

D = native.DTYPES
F32, F8 = D["F32"], D["F8_E4M3"]
MiB = 1 << 20
CAP = 16 * MiB
SENTINEL = 0xAB
FAR = 1 << 30


@pytest.fixture(scope="module")
def mem():
    """(arena, x, s, e, hx, hs): a device arena, 128 f32 sources, 128 f32
    scales and 128 E8M0 bytes on the GPU, 128 f32 on the host twice"""
    a = native.Arena(0, CAP)
    a.fill(0, CAP, SENTINEL)
    x = torch.ones(128, device="cuda:0")
    s = torch.ones(128, device="cuda:0")
    e = torch.full((128,), 127, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    yield a, x, s, e, torch.ones(128), torch.ones(128)
    a.close()


def rows_for(mem):
    """(call, good segment, bad segment, message) for every entry point"""
    a, x, s, e, hx, hs = mem
    p, q, ep, hp, hq = (t.data_ptr() for t in (x, s, e, hx, hs))
    base = a.base_ptr()
    blk = (4, 16, 2, 8)            # M, K, bm, bn: 4 tiles per 64 elements
    dev = lambda fn: (lambda segs: fn(0, segs))
    rows = []

    def add(call, who, good, cases):
        for bad, message in cases:
            rows.append((call, good, bad, f"{who}: {message}"))

    add(a.convert_ptr, "convert", (0, p, 1, 16, 16, F8, F32, q, 4, 0), [
        ((0, p, 1, 16, 16, F8, F32, hq, 4, 0),
         "scale_ptr is not device-visible memory"),
        # 2 Mi elements from the arena's head land in its upper half: only
        # their 8 MiB of scales leave the tensor's allocation
        ((0, base + 8 * MiB, 1, 2 * MiB, 2 * MiB, F8, F32, q, 1, 0),
         "scales runs past its allocation")])
    add(a.store_ptr, "store", (p, 0, 1, 16, 64, F32, F8, q, 4, 0), [
        ((hp, 0, 1, 16, 64, F32, F32), "src_ptr is not device-visible memory"),
        ((p, 0, 2, 16, FAR, F32, F32), "source runs past its allocation"),
        ((p, 0, 1, 16, 64, F32, F8, hq, 4, 0),
         "scale_ptr is not device-visible memory"),
        ((base + 8 * MiB, 0, 1, 2 * MiB, 8 * MiB, F32, F8, q, 1, 0),
         "scales runs past its allocation"),
        # the source is looked at before the scales
        ((hp, 0, 1, 16, 64, F32, F8, hq, 4, 0),
         "src_ptr is not device-visible memory")])
    add(dev(native.absmax_scales), "absmax", (p, 1, 16, 64, F32, q, 4, 0, 4), [
        ((hp, 1, 16, 64, F32, q, 4, 0, 4),
         "src_ptr is not device-visible memory"),
        ((p, 2, 16, FAR, F32, q, 4, 0, 8), "source runs past its allocation"),
        ((p, 1, 16, 64, F32, hq, 4, 0, 4),
         "out_ptr is not device-visible memory"),
        ((p, 1, 16, 64, F32, q, 4, 0, FAR // 4),
         "scales runs past its allocation")])
    add(a.store_ptr, "mx store", (p, 0, 1, 32, 128, F32, F8, ep, 0, 32, 32), [
        ((hp, 0, 1, 32, 128, F32, F8, ep, 0, 32, 32),
         "src_ptr is not device-visible memory"),
        ((p, 0, 2, 32, FAR, F32, F8, ep, 0, 32, 32),
         "source runs past its allocation"),
        ((p, 0, 1, 32, 128, F32, F8, hq, 0, 32, 32),
         "scale_ptr is not device-visible memory"),
        ((p, 0, 2, 32, 128, F32, F8, ep, 0, 32 * FAR, 32),
         "scales runs past its allocation")])
    add(a.convert_ptr, "mx convert", (0, p, 1, 32, 32, F8, F32, ep, 0, 32, 32), [
        ((0, hp, 1, 32, 32, F8, F32, ep, 0, 32, 32),
         "dst_ptr is not device-visible memory"),
        ((0, p, 1, 8 * MiB, 8 * MiB, F8, F32, ep, 0, 8 * MiB, 32),
         "destination runs past its allocation"),
        ((0, p, 1, 32, 32, F8, F32, hq, 0, 32, 32),
         "scale_ptr is not device-visible memory"),
        ((0, p, 2, 32, 32, F8, F32, ep, 0, 32 * FAR, 32),
         "scales runs past its allocation")])
    # the scales of a whole tensor are 1/128 of its f32 bytes: the arena's
    # own memory is the source, and the scales start 64 bytes before its end
    add(dev(native.mx_scales), "mx scales", (p, 1, 32, 128, F32, F8, ep), [
        ((hp, 1, 32, 128, F32, F8, ep), "src_ptr is not device-visible memory"),
        ((p, 2, 32, FAR, F32, F8, ep), "source runs past its allocation"),
        ((p, 1, 32, 128, F32, F8, hq), "scale_ptr is not device-visible memory"),
        ((base, 1, CAP // 4, CAP, F32, F8, base + CAP - 64),
         "scales runs past its allocation")])
    add(a.store_ptr, "block store",
        (p, 0, 1, 64, 256, F32, F8, q, 0, 64) + blk, [
        ((hp, 0, 1, 64, 256, F32, F8, q, 0, 64) + blk,
         "src_ptr is not device-visible memory"),
        ((p, 0, 2, 64, FAR, F32, F8, q, 0, 64) + blk,
         "source runs past its allocation"),
        ((p, 0, 1, 64, 256, F32, F8, hq, 0, 64) + blk,
         "scale_ptr is not device-visible memory"),
        ((p, 0, 2, 64, 256, F32, F8, q, 0, 16 * FAR) + blk,
         "scales runs past its allocation")])
    add(a.convert_ptr, "block convert",
        (0, p, 1, 64, 64, F8, F32, q, 0, 64) + blk, [
        ((0, hp, 1, 64, 64, F8, F32, q, 0, 64) + blk,
         "dst_ptr is not device-visible memory"),
        ((0, p, 1, 8 * MiB, 8 * MiB, F8, F32, q, 0, 8 * MiB) + blk,
         "destination runs past its allocation"),
        ((0, p, 1, 64, 64, F8, F32, hq, 0, 64) + blk,
         "scale_ptr is not device-visible memory"),
        ((0, p, 2, 64, 64, F8, F32, q, 0, 16 * FAR) + blk,
         "scales runs past its allocation")])
    # the segment's own range check names the slots scale_ptr, the merged
    # one out_ptr: the first comes first
    add(dev(native.block_absmax_scales), "block absmax",
        (p, 1, 64, 256, F32, q, 0, 64) + blk + (4,), [
        ((hp, 1, 64, 256, F32, q, 0, 64) + blk + (4,),
         "src_ptr is not device-visible memory"),
        ((p, 2, 64, FAR, F32, q, 0, 64) + blk + (8,),
         "source runs past its allocation"),
        ((p, 1, 64, 256, F32, hq, 0, 64) + blk + (4,),
         "scale_ptr is not device-visible memory"),
        ((p, 1, 64, 256, F32, q, 0, 64) + blk + (FAR // 4,),
         "scales runs past its allocation")])
    return rows


def test_device_ranges_refused(mem):
    a, x, s, e, hx, hs = mem
    rows = rows_for(mem)
    assert len(rows) == 35
    for call, good, bad, message in rows:
        with pytest.raises(ValueError) as ei:
            call([good, bad])
        assert str(ei.value) == message, (bad, message)
    torch.cuda.synchronize()
    head = bytearray(MiB)
    a.read(0, head)
    assert head == bytes([SENTINEL]) * MiB
    assert torch.equal(x.cpu(), torch.ones(128))
    assert torch.equal(s.cpu(), torch.ones(128))
    assert torch.equal(e.cpu(), torch.full((128,), 127, dtype=torch.uint8))
    assert torch.equal(hx, torch.ones(128)) and torch.equal(hs, torch.ones(128))
