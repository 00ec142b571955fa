"""Shared cases for the array-sample tests (host arena and MI355X).

Nothing here imports project code.  The expected tensor is numpy's
`src[b, dy:dy+h, dx:dx+w, :]` (reversed along w when flipped)
`.astype(np.float32) * scale + bias` with float32 scale and bias, transposed
for NCHW, then `torch.from_numpy(...).to(dtype)` on the CPU.  The runners
take the arena, the dtype codes and the loader factory from the test module
that calls them, so the host and the GPU file run the same matrix.  Every
comparison is byte equality on whole buffers, guard bytes included."""
import io
import random

import numpy as np
import torch

DSTS = ["F32", "F16", "BF16"]
TORCH_DST = {"F32": torch.float32, "F16": torch.float16,
             "BF16": torch.bfloat16}
ITEM = {"F32": 4, "F16": 2, "BF16": 2}
LAYOUTS = ("NCHW", "NHWC")
SENTINEL = 0xAB
GUARD = 16

IMAGENET_MEAN = (0.485, 0.456, 0.406, 0.5)
IMAGENET_STD = (0.229, 0.224, 0.225, 0.25)


def norm(mean, std, C):
    """(scale, bias) as float32 arrays, by the loader's rule: Python floats,
    rounded once."""
    scale = np.array([1.0 / (255.0 * s) for s in std[:C]], np.float32)
    bias = np.array([-m / s for m, s in zip(mean[:C], std[:C])], np.float32)
    return scale, bias


def default_norm(C):
    return norm((0.0,) * 4, (1.0,) * 4, C)


def ref_sample(img, dy, dx, flip, crop, scale, bias, layout, dst):
    """img [H, W, C] uint8 -> (bytes of the dense output as uint8 array,
    the sample byte index every output element comes from)."""
    h, w = crop
    H, W, C = img.shape
    idx = np.arange(H * W * C, dtype=np.int64).reshape(H, W, C)
    x, e = img[dy:dy + h, dx:dx + w, :], idx[dy:dy + h, dx:dx + w, :]
    if flip:
        x, e = x[:, ::-1, :], e[:, ::-1, :]
    v = x.astype(np.float32) * scale + bias
    assert v.dtype == np.float32
    if layout == "NCHW":
        v, e = v.transpose(2, 0, 1), e.transpose(2, 0, 1)
    t = torch.from_numpy(np.ascontiguousarray(v)).to(TORCH_DST[dst])
    raw = t.contiguous().view(torch.uint8).numpy().reshape(-1)
    return raw, np.ascontiguousarray(e).reshape(-1)


def ref_batch(src, order, aug, crop, scale, bias, layout, dst):
    """The loader's tensor for samples src[order] under aug, as torch."""
    h, w = crop
    C = src.shape[3]
    out = []
    for i, (dy, dx, flip) in zip(order, aug):
        raw, _ = ref_sample(src[i], dy, dx, flip, crop, scale, bias, layout,
                            dst)
        t = torch.from_numpy(raw.copy()).view(TORCH_DST[dst])
        out.append(t.reshape((C, h, w) if layout == "NCHW" else (h, w, C)))
    return torch.stack(out)


# ------------------------------------------------------------ kernel runner

class Call:
    """One Arena.array_samples call on a sentinel-filled destination that
    starts `el_off` elements past a 16-byte boundary."""

    def __init__(self, arena, D, device, dst, shape, crop, rows, scale, bias,
                 layout="NCHW", el_off=1):
        self.arena, self.D, self.device, self.dst = arena, D, device, dst
        self.shape, self.crop, self.rows = tuple(shape), tuple(crop), rows
        self.scale, self.bias, self.layout = scale, bias, layout
        self.ds = ITEM[dst]
        self.batch = len(rows)
        self.out_el = shape[2] * crop[0] * crop[1]
        self.lead = GUARD + el_off * self.ds
        self.nbytes = self.lead + self.batch * self.out_el * self.ds + GUARD
        self.buf = torch.full((self.nbytes,), SENTINEL, dtype=torch.uint8,
                              device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.lead
        self.exp = np.full(self.nbytes, SENTINEL, np.uint8)
        self.pieces = []

    def place(self, off, img):
        self.arena.write(off, img.tobytes())

    def piece(self, off, row, e0, n, img):
        """Bytes e0 .. e0+n-1 of `img` (placed so that they sit at `off`)
        are a piece of sample `row`."""
        self.pieces.append((off, row, e0, n))
        dy, dx, flip = self.rows[row]
        raw, emap = ref_sample(img, dy, dx, flip, self.crop, self.scale,
                               self.bias, self.layout, self.dst)
        hit = np.repeat((emap >= e0) & (emap < e0 + n), self.ds)
        a = self.lead + row * self.out_el * self.ds
        view = self.exp[a:a + self.out_el * self.ds]
        view[hit] = raw[hit]

    def sample(self, off, row, img, cuts=(), keep=None):
        """A whole sample placed at `off`, cut into pieces at `cuts`;
        `keep` lists the pieces that are passed on (default: all)."""
        self.place(off, img)
        edges = [0, *cuts, img.size]
        for i, (a, b) in enumerate(zip(edges, edges[1:])):
            assert a < b
            if keep is None or i in keep:
                self.piece(off + a, row, a, b - a, img)

    def run(self, reverse=False):
        pieces = self.pieces[::-1] if reverse else self.pieces
        self.arena.array_samples(pieces, self.rows, self.ptr, self.batch,
                                 self.shape, self.crop, self.scale,
                                 self.bias, self.D[self.dst], self.layout)
        self.check()

    def check(self):
        """Written elements, untouched elements and guards, byte for byte."""
        got = self.buf.cpu().numpy()
        if not np.array_equal(got, self.exp):
            i = int(np.nonzero(got != self.exp)[0][0])
            raise AssertionError(
                f"differs at byte {i} (element {(i - self.lead) // self.ds}"
                f" of {self.batch} x {self.out_el}): {got[i]:#x} != "
                f"{self.exp[i]:#x}; {self.dst} {self.layout} shape="
                f"{self.shape} crop={self.crop} rows={self.rows[:4]} "
                f"pieces={self.pieces[:4]}")


# -------------------------------------------------------------------- cases

def exhaustive_image(C):
    p = np.arange(256, dtype=np.int64).reshape(16, 16, 1)
    c = np.arange(C, dtype=np.int64).reshape(1, 1, C)
    return ((p + 85 * c) % 256).astype(np.uint8)


def case_exhaustive(arena, D, device, dst):
    """All 256 byte values in every channel, C = 1..4, full frame, four
    normalisations: ImageNet, the default, scale 1000 (F16 overflows to
    inf) and a tiny scale (F16 subnormals)."""
    for C in (1, 2, 3, 4):
        img = exhaustive_image(C)
        assert all(len(set(img[:, :, c].ravel().tolist())) == 256
                   for c in range(C))
        one = np.ones(C, np.float32)
        sets = [norm(IMAGENET_MEAN, IMAGENET_STD, C), default_norm(C),
                (1000 * one, np.linspace(-3, 3, C).astype(np.float32)),
                (np.float32(1e-7) * one, np.zeros(C, np.float32))]
        for k, (scale, bias) in enumerate(sets):
            for layout in LAYOUTS:
                c = Call(arena, D, device, dst, (16, 16, C), (16, 16),
                         [(0, 0, 0)], scale, bias, layout, el_off=k)
                c.sample(4096 + 3 * k + C, 0, img)
                c.run()
    # the sets do what they are there for
    if dst == "F16":
        raw, _ = ref_sample(exhaustive_image(1), 0, 0, 0, (16, 16),
                            np.float32([1000]), np.float32([0]), "NCHW", dst)
        assert torch.isinf(torch.from_numpy(raw.copy()).view(
            torch.float16)).any()
        raw, _ = ref_sample(exhaustive_image(1), 0, 0, 0, (16, 16),
                            np.float32([1e-7]), np.float32([0]), "NCHW", dst)
        t = torch.from_numpy(raw.copy()).view(torch.float16).float()
        assert ((t > 0) & (t < 2.0 ** -14)).any()


def case_residues(arena, D, device, dst):
    """5x7x3 samples (105 bytes) from arena byte 4096 + r, r in 0..15: one
    call holds a sample per (dy, dx, flip) of the 3x5 crop, for destination
    element offsets 0..3 and both layouts."""
    rng = np.random.default_rng(7)
    shape, crop = (5, 7, 3), (3, 5)
    rows = [(dy, dx, f) for dy in range(3) for dx in range(3)
            for f in (0, 1)]
    scale, bias = norm(IMAGENET_MEAN, IMAGENET_STD, 3)
    for r in range(16):
        imgs = rng.integers(0, 256, (len(rows),) + shape).astype(np.uint8)
        for el_off in range(4):
            for layout in LAYOUTS:
                c = Call(arena, D, device, dst, shape, crop, rows, scale,
                         bias, layout, el_off)
                for b in range(len(rows)):
                    c.sample(4096 + r + 105 * b, b, imgs[b])
                c.run()


def case_splits(arena, D, device, dst):
    """9x11xC samples, crop 7x8 at (1, 2): one call holds a sample per cut
    k in 1..n-1; three pieces with a one-byte middle piece, listed in
    reversed order; one piece of two only."""
    rng = np.random.default_rng(11)
    for C in (3, 4):
        shape, crop = (9, 11, C), (7, 8)
        n = 9 * 11 * C
        scale, bias = norm(IMAGENET_MEAN, IMAGENET_STD, C)
        img = rng.integers(0, 256, shape).astype(np.uint8)
        for flip in (0, 1):
            for layout in LAYOUTS:
                rows = [(1, 2, flip)] * (n - 1)
                c = Call(arena, D, device, dst, shape, crop, rows, scale,
                         bias, layout)
                for k in range(1, n):
                    c.sample(4096 + (n + 1) * (k - 1), k - 1, img, (k,))
                c.run()
                mids = (1, C * 11 * 2 + C * 3 + 1, n // 2, n - 3, n - 2)
                rows = [(1, 2, flip)] * len(mids)
                c = Call(arena, D, device, dst, shape, crop, rows, scale,
                         bias, layout, el_off=3)
                for b, m in enumerate(mids):
                    c.sample(4099 + (n + 3) * b, b, img, (m, m + 1))
                c.run(reverse=True)
                rows = [(1, 2, flip)] * 4
                c = Call(arena, D, device, dst, shape, crop, rows, scale,
                         bias, layout, el_off=2)
                for b, (k, keep) in enumerate(((n // 2, 0), (n // 2, 1),
                                               (n // 3 + 1, 0), (7, 1))):
                    c.sample(4097 + (n + 5) * b, b, img, (k,), keep=(keep,))
                c.run()


def long_shape(tile):
    """61x67x3 for the 4096-byte tile; longer than 2 * tile + 1 bytes, with
    W*C no multiple of 4, whatever the tile is."""
    if tile == 4096:
        return (61, 67, 3)
    return (-(-(2 * tile + 2) // 201) + 8, 67, 3)


def case_long(arena, D, device, dst, tile, cap):
    """Three samples longer than two tiles in one call, crops 53x64 and
    53x63 with a different (dy, dx, flip) per row, whole and cut around the
    tile size; the last sample ends at the arena's last byte."""
    rng = np.random.default_rng(13)
    shape = long_shape(tile)
    H, W, C = shape
    n = H * W * C
    assert n > 2 * tile + 1 and (W * C) % 4
    imgs = rng.integers(0, 256, (3,) + shape).astype(np.uint8)
    scale, bias = norm(IMAGENET_MEAN, IMAGENET_STD, C)
    offs = (4097, 4097 + n + 2, cap - n)
    for crop in ((53, 64), (53, 63)):
        h, w = crop
        rows = [(H - h, W - w, 1), (0, 0, 0), ((H - h) // 2, 1, 1)]
        for cuts in ((), (tile - 1,), (tile,), (tile + 1,)):
            for layout in LAYOUTS:
                c = Call(arena, D, device, dst, shape, crop, rows, scale,
                         bias, layout, el_off=len(cuts) + 2 * (w & 1))
                for b in range(3):
                    c.sample(offs[b], b, imgs[b], cuts)
                c.run(reverse=bool(cuts))


def case_empty(arena, D, device, dst):
    for layout in LAYOUTS:
        scale, bias = default_norm(3)
        c = Call(arena, D, device, dst, (5, 7, 3), (3, 5), [(0, 0, 0)] * 2,
                 scale, bias, layout)
        c.run()


BASE = dict(shape=(5, 7, 3), crop=(3, 5), batch=2,
            rows=[(1, 1, 0), (2, 2, 1)], scale=[0.5, 0.25, 2.0],
            bias=[0.0, 1.0, -1.0], dst="F32", layout="NCHW", shift=0)


def reject_calls(cap):
    """(what, overrides of BASE, extra pieces): calls that must raise
    ValueError.  The valid piece comes first in each, so a call that ran
    anyway would show in the destination.  `shift` moves out_ptr (None =
    null, above 4096 = an absolute address); `dst` may be a raw code."""
    big = 2 ** 64 - 1
    inf, nan = float("inf"), float("nan")
    out = [("dtype %s" % d, dict(dst=d), []) for d in
           ("I64", "U8", "F64", "F8_E4M3", "I32", "U16")]
    out += [
        ("unknown dtype code", dict(dst=99), []),
        ("dtype code 15", dict(dst=15), []),
        ("C 0", dict(shape=(5, 7, 0), scale=[], bias=[]), []),
        ("C 5", dict(shape=(5, 7, 5), scale=[1.0] * 5, bias=[0.0] * 5), []),
        ("H 0", dict(shape=(0, 7, 3)), []),
        ("W 0", dict(shape=(5, 0, 3)), []),
        ("h 0", dict(crop=(0, 5)), []),
        ("w 0", dict(crop=(3, 0)), []),
        ("batch 0", dict(batch=0, rows=[]), []),
        ("h > H", dict(crop=(6, 5)), []),
        ("w > W", dict(crop=(3, 8)), []),
        ("rows short", dict(rows=[(1, 1, 0)]), []),
        ("rows long", dict(rows=[(1, 1, 0)] * 3), []),
        ("dy + h > H", dict(rows=[(3, 1, 0), (0, 0, 0)]), []),
        ("dx + w > W", dict(rows=[(0, 0, 0), (1, 3, 0)]), []),
        ("dy overflow", dict(rows=[(big, 1, 0), (0, 0, 0)]), []),
        ("dx overflow", dict(rows=[(0, big - 2, 0), (0, 0, 0)]), []),
        ("flip 2", dict(rows=[(1, 1, 2), (0, 0, 0)]), []),
        ("scale inf", dict(scale=[0.5, inf, 2.0]), []),
        ("scale nan", dict(scale=[nan, 0.25, 2.0]), []),
        ("bias -inf", dict(bias=[0.0, 1.0, -inf]), []),
        ("bias nan", dict(bias=[0.0, nan, 0.0]), []),
        ("scale short", dict(scale=[0.5, 0.25]), []),
        ("scale long", dict(scale=[0.5] * 4), []),
        ("bias short", dict(bias=[0.5]), []),
        ("bias long", dict(bias=[0.5] * 4), []),
        ("layout", dict(layout="NCWH"), []),
        ("n 0", {}, [(4096, 1, 0, 0)]),
        ("row >= batch", {}, [(4096, 2, 0, 1)]),
        ("past sample", {}, [(4096, 1, 1, 105)]),
        ("e0 past sample", {}, [(4096, 1, 105, 1)]),
        ("past arena", {}, [(cap - 104, 1, 0, 105)]),
        ("src_off overflow", {}, [(big, 1, 0, 2)]),
        ("n overflow", {}, [(4096, 1, 0, big)]),
        ("e0 overflow", {}, [(4096, 1, big, 2)]),
        ("batch overflow", dict(batch=2 ** 62, rows=[]), []),
        ("sample overflow", dict(shape=(2 ** 40, 2 ** 40, 3)), []),
        ("sample 2^31", dict(shape=(2 ** 16, 2 ** 15, 1), scale=[1.0],
                             bias=[0.0], crop=(1, 1)), []),
        ("out null", dict(shift=None), []),
        ("out misaligned", dict(shift=2), []),
        ("out odd", dict(shift=1, dst="BF16"), []),
        ("out odd f16", dict(shift=3, dst="F16"), []),
    ]
    return out


def run_rejects(arena, D, device, cap, raises, extra=()):
    """Every reject raises ValueError and leaves the destination
    untouched."""
    rng = np.random.default_rng(19)
    img = rng.integers(0, 256, (5, 7, 3)).astype(np.uint8)
    for what, over, more in list(reject_calls(cap)) + list(extra):
        kw = dict(BASE)
        kw.update(over)
        c = Call(arena, D, device, "F32", BASE["shape"], BASE["crop"],
                 BASE["rows"], BASE["scale"], BASE["bias"])
        c.place(4096, img)
        shift = kw["shift"]
        ptr = 0 if shift is None else (shift if shift > 4096
                                       else c.ptr + shift)
        dst = D[kw["dst"]] if isinstance(kw["dst"], str) else kw["dst"]
        with raises(ValueError):
            arena.array_samples([(4096, 0, 0, 105)] + more, kw["rows"], ptr,
                                kw["batch"], kw["shape"], kw["crop"],
                                kw["scale"], kw["bias"], dst, kw["layout"])
            raise AssertionError(f"accepted: {what}")
        c.check()


# ------------------------------------------------------------- end to end

E2E = dict(shape=(5, 7, 3), counts=(7, 9), batch=3, block=64)


def npy_bytes(arr, version=(1, 0)):
    f = io.BytesIO()
    np.lib.format.write_array(f, arr, version=version)
    return f.getvalue()


def e2e_files():
    """Two .npy files of 5x7x3 samples and their '<i8' labels; with 64-byte
    blocks every 105-byte sample is cut, most between the channels of a
    pixel."""
    rng = np.random.default_rng(23)
    data, labels = [], []
    for k, n in enumerate(E2E["counts"]):
        data.append(rng.integers(0, 256, (n,) + E2E["shape"]).astype(np.uint8))
        labels.append((rng.integers(-5, 1000, n) + k * 10 ** 10).astype("<i8"))
    blobs = [npy_bytes(a, v) for a, v in zip(data, ((1, 0), (2, 0)))]
    lblobs = [npy_bytes(a) for a in labels]
    return np.concatenate(data), np.concatenate(labels), blobs, lblobs


def ref_order(n, shuffle, seed, epoch, rank, world, shape, crop, random_crop,
              random_flip):
    """The stated recipe, recomputed: (order, aug) of one rank."""
    H, W, _ = shape
    h, w = crop
    order = list(range(n))
    rng = random.Random(seed + epoch)
    if shuffle:
        rng.shuffle(order)
    aug = []
    for _ in range(n):
        dy, dx, flip = (H - h) // 2, (W - w) // 2, 0
        if random_crop:
            dy = rng.randrange(H - h + 1)
            dx = rng.randrange(W - w + 1)
        if random_flip:
            flip = rng.randrange(2)
        aug.append((dy, dx, flip))
    keep = n - n % world
    return order[:keep][rank::world], aug[:keep][rank::world]


def check_epoch(ld, src, labels, order, aug, dst="F32", layout="NCHW",
                drop_last=True, with_labels=True):
    """The loader's batches are the reference of src[order] under aug, cut
    into batches; returns the batches."""
    bs = E2E["batch"]
    n = len(order) // bs * bs if drop_last else len(order)
    assert ld.augmentation() == aug
    scale = np.array(ld.scale, np.float32)
    bias = np.array(ld.bias, np.float32)
    ref = ref_batch(src, order[:n], aug[:n], ld.crop, scale, bias, layout,
                    dst)
    xs, ls = [], []
    for item in ld:
        x, lab = item if with_labels else (item, None)
        assert x.is_contiguous() and x.dtype == TORCH_DST[dst]
        assert x.device.type == torch.device(ld.device).type
        xs.append(x.cpu())
        if with_labels:
            assert lab.dtype == torch.int64 and lab.device == x.device
            ls.append(lab.cpu())
    assert len(xs) == len(ld) == -(-n // bs)
    got = torch.cat(xs)
    assert got.shape == ref.shape
    assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8))
    if with_labels:
        assert np.array_equal(torch.cat(ls).numpy(), labels[order[:n]])
    return xs


def check_loader(make, src, labels):
    """The loader properties every tier has to show.  make(**kw) builds a
    loader over the two files with their labels; the caller closes what
    make returned."""
    n, bs, shape = len(src), E2E["batch"], E2E["shape"]
    assert n % bs and (n // 2) % bs, "the short batch must exist"
    full = shape[:2]
    mean, std = IMAGENET_MEAN[:3], IMAGENET_STD[:3]

    def recipe(**kw):
        a = dict(shuffle=False, seed=0, epoch=0, rank=0, world=1,
                 crop=full, random_crop=False, random_flip=False)
        a.update(kw)
        return ref_order(n, a["shuffle"], a["seed"], a["epoch"], a["rank"],
                         a["world"], shape, a["crop"], a["random_crop"],
                         a["random_flip"])

    ld = make()
    assert ld.num_samples == n and ld.shape == shape and ld.crop == full
    s, b = default_norm(3)
    assert ld.scale == tuple(float(v) for v in s)
    assert ld.bias == tuple(float(v) for v in b)
    check_epoch(ld, src, labels, *recipe())
    check_epoch(ld, src, labels, *recipe())        # replayed plans
    xs = check_epoch(make(drop_last=False), src, labels, *recipe(),
                     drop_last=False)
    assert len(xs[-1]) == n % bs

    ld = make(mean=mean, std=std, crop=(3, 5))
    s, b = norm(mean, std, 3)
    assert ld.scale == tuple(float(v) for v in s)
    assert ld.bias == tuple(float(v) for v in b)
    order, aug = recipe(crop=(3, 5))
    assert set(aug) == {(1, 1, 0)}
    check_epoch(ld, src, labels, order, aug)

    ld = make(shuffle=True, seed=5, mean=mean, std=std)
    orders = []
    for epoch in (0, 1):
        ld.set_epoch(epoch)
        order, aug = recipe(shuffle=True, seed=5, epoch=epoch)
        check_epoch(ld, src, labels, order, aug)
        orders.append(order)
    assert orders[0] != orders[1] and sorted(orders[0]) == list(range(n))

    for drop_last in (True, False):
        seen = []
        for rank in (0, 1):
            ld = make(rank=rank, world=2, drop_last=drop_last)
            order, aug = recipe(rank=rank, world=2)
            assert ld.num_samples == len(order) == n // 2
            xs = check_epoch(ld, src, labels, order, aug,
                             drop_last=drop_last)
            assert len(xs[-1]) == (bs if drop_last else (n // 2) % bs)
            seen += order
        assert sorted(seen) == list(range(n))

    for kw in (dict(random_crop=True), dict(random_flip=True),
               dict(random_crop=True, random_flip=True, shuffle=True)):
        ld = make(crop=(3, 5), seed=3, mean=mean, std=std, **kw)
        augs = []
        for epoch in (0, 1):
            ld.set_epoch(epoch)
            order, aug = recipe(crop=(3, 5), seed=3, epoch=epoch, **kw)
            check_epoch(ld, src, labels, order, aug)
            augs.append(aug)
        assert augs[0] != augs[1]
        if kw.get("random_flip"):
            assert {a[2] for a in augs[0]} == {0, 1}
        if kw.get("random_crop"):
            assert len({a[:2] for a in augs[0]}) > 3
    # both ranks draw from one table
    tables = []
    for rank in (0, 1):
        ld = make(crop=(3, 5), seed=3, random_crop=True, random_flip=True,
                  rank=rank, world=2)
        tables.append(ld.augmentation())
    whole = recipe(crop=(3, 5), seed=3, random_crop=True,
                   random_flip=True)[1]
    assert tables[0] == whole[0::2] and tables[1] == whole[1::2]

    ld = make(out_dtype=torch.bfloat16, crop=(3, 5), random_flip=True,
              mean=mean, std=std)
    check_epoch(ld, src, labels, *recipe(crop=(3, 5), random_flip=True),
                dst="BF16")
    ld = make(out_dtype=torch.float16, layout="NHWC", crop=4,
              random_crop=True, random_flip=True)
    assert ld.crop == (4, 4)
    check_epoch(ld, src, labels,
                *recipe(crop=(4, 4), random_crop=True, random_flip=True),
                dst="F16", layout="NHWC")
    ld = make(layout="NHWC", labels=None, mean=mean, std=std)
    check_epoch(ld, src, labels, *recipe(), layout="NHWC",
                with_labels=False)
