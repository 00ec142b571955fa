"""FsReader: positioned reads across blocks with replica fallback.

Analog of /root/reference/crates/client/curvine-client-core/src/file/
fs_reader.rs + block/block_reader.rs:111-230 (local short-circuit first,
remote fallback on failure, failed-worker tracking) and
fs_reader_parallel.rs (sliced parallel reads for large requests);
`ReadDetector` (read_detector.rs:42-134) gates sequential prefetch.
"""
from __future__ import annotations

import asyncio

from curvine_amd import errors as err
from curvine_amd.client.block_client import (BlockReaderHole, BlockReaderLocal,
                                             BlockReaderRemote)
from curvine_amd.client.fs_client import FsClient
from curvine_amd.model import FileBlocks, LocatedBlock


class ReadDetector:
    """Sequential-vs-random pattern detection (read_detector.rs analog)."""

    def __init__(self):
        self.last_end = 0
        self.seq_count = 0
        self.rand_count = 0

    def observe(self, off: int, n: int) -> None:
        if off == self.last_end:
            self.seq_count += 1
        else:
            self.rand_count += 1
        self.last_end = off + n

    @property
    def is_sequential(self) -> bool:
        return self.seq_count >= self.rand_count



def _slow_scales(scale, n):
    """The scales a slow extent of `n` elements needs, by the scale fields
    of its resolve_convert entry: (ctypes element type, first index, count,
    convert).  scale_ptr[first : first + count] is fetched into a ctypes
    array and convert(raw, src_code, dst_code, array) is the host converter
    with its scale arguments rebased onto that array."""
    import ctypes

    from curvine_amd import native
    if not scale:
        return ctypes.c_float, 0, 0, \
            lambda raw, sc, dc, _sbuf: native.convert_host(raw, sc, dc, n)
    if len(scale) == 4:
        # the E8M0 bytes of the blocks this extent touches
        _sptr, e0, _spitch, blk = scale
        g0, g1 = e0 // blk, (e0 + n - 1) // blk
        return ctypes.c_uint8, g0, g1 - g0 + 1, \
            lambda raw, sc, dc, sbuf: native.mx_convert_host(
                raw, sc, dc, n, sbuf, e0 - g0 * blk)
    if len(scale) == 7:
        # the tile scales of the tensor rows this extent touches
        _sptr, e0, _spitch, m, k, bm, bn = scale
        tm, tn = -(-m // bm), -(-k // bn)

        def tile_row(row):
            return (row // m * tm + row % m // bm) * tn
        g0 = tile_row(e0 // k)
        return ctypes.c_float, g0, tile_row((e0 + n - 1) // k) + tn - g0, \
            lambda raw, sc, dc, sbuf: native.block_convert_host(
                raw, sc, dc, n, sbuf, e0, m, k, bm, bn, g0)
    # the groups this extent touches
    _sptr, every, e0 = scale
    g0 = e0 // every if every else 0
    g1 = (e0 + n - 1) // every if every else 0
    return ctypes.c_float, g0, g1 - g0 + 1, \
        lambda raw, sc, dc, sbuf: native.convert_host(
            raw, sc, dc, n, scales=sbuf, scale_every=every,
            scale_e0=e0 - g0 * every)


def _hole_span(offs, blocks, length, pos) -> int:
    """Length of the zero hole at file offset pos, or 0 when pos falls
    inside a cached block extent.  Metadata length may exceed block
    coverage (extending truncate, sparse tails): the uncovered range
    reads back as zeros, like the reference's hole synthesis
    (block_reader_hole.rs)."""
    import bisect
    idx = bisect.bisect_right(offs, pos) - 1
    nxt = idx + 1
    if idx >= 0:
        lb = blocks[idx]
        if pos < lb.offset + lb.block.length:
            return 0
    end = offs[nxt] if nxt < len(offs) else length
    return max(0, end - pos)


class SyncLocalReader:
    """Synchronous short-circuit reader: all blocks resolved to in-process
    store readers at construction; pread_* are plain function calls safe
    from any OS thread — no event loop in the per-op path.  This is the
    IOPS path (4 KiB random reads must not pay two thread hops + loop
    scheduling per op).  Remote blocks -> construction fails (caller keeps
    the async FsReader)."""

    def __init__(self, file_blocks: FileBlocks, ipc_resolver=None):
        from curvine_amd.worker import registry
        self.fb = file_blocks
        self.length = file_blocks.status.length
        self._offs = [b.offset for b in file_blocks.blocks]
        self._readers = []
        self._native_rid = None
        try:
            for lb in file_blocks.blocks:
                r = None
                for addr in lb.locations:
                    store = registry.lookup(addr.worker_id)
                    if store is not None:
                        r = store.open_reader(lb.block.block_id)
                        break
                if r is None and ipc_resolver is not None:
                    # colocated other-process worker: hipIpc-mapped view
                    r = ipc_resolver(lb)
                if r is None:
                    raise err.BlockNotFound(
                        f"block {lb.block.block_id} has no in-process replica")
                self._readers.append(r)
        except Exception:
            self.close()
            raise
        self._try_register_native()

    def _try_register_native(self) -> None:
        """Pin the extent table in C++ when every block is arena-backed:
        batched preads then resolve+issue+sync GIL-free (reader_register
        in csrc/module.cpp).  The store readers stay open for the whole
        registration (refcounts defer delete/demote), mirroring the
        native FUSE read contract."""
        exts = []
        for lb, r in zip(self.fb.blocks, self._readers):
            meta = r.meta
            arena = getattr(r.layout, "arena", None)
            if meta.get("kind") != "arena" or arena is None:
                return
            exts.append((lb.offset, lb.block.length, arena.handle,
                         meta["offset"]))
        if not exts:
            return
        try:
            from curvine_amd import native
            self._native = native.load()
            self._native_rid = self._native.reader_register(
                exts, self.length)
        except Exception:  # noqa: BLE001 — extension absent on this host
            self._native_rid = None

    def pread_into(self, off: int, out, out_off: int, n: int) -> int:
        import bisect
        n = max(0, min(n, self.length - off))
        got = 0
        while got < n:
            pos = off + got
            hole = _hole_span(self._offs, self.fb.blocks, self.length, pos)
            if hole > 0:
                fill = min(hole, n - got)
                out[out_off + got:out_off + got + fill] = b"\x00" * fill
                got += fill
                continue
            idx = bisect.bisect_right(self._offs, pos) - 1
            if idx < 0 or idx >= len(self._readers):
                break
            lb = self.fb.blocks[idx]
            boff = pos - lb.offset
            want = min(n - got, lb.block.length - boff)
            got += self._readers[idx].read_into(boff, out, out_off + got, want)
        return got

    def pread_into_ptr(self, off: int, ptr: int, n: int) -> int:
        """Pinned/device-pointer destination (direct DMA).  A registered
        reader serves the whole range in one GIL-free native call
        (reader_pread: block-spanning reads included); holes, sparse tails
        and unregistered readers take the Python loop below."""
        if self._native_rid is not None and off >= 0 and n > 0:
            got = self._native.reader_pread(self._native_rid, off, n, ptr)
            if got >= 0:
                return got
        import bisect
        import ctypes
        n = max(0, min(n, self.length - off))
        got = 0
        while got < n:
            pos = off + got
            hole = _hole_span(self._offs, self.fb.blocks, self.length, pos)
            if hole > 0:
                fill = min(hole, n - got)
                ctypes.memset(ptr + got, 0, fill)
                got += fill
                continue
            idx = bisect.bisect_right(self._offs, pos) - 1
            if idx < 0 or idx >= len(self._readers):
                break
            lb = self.fb.blocks[idx]
            boff = pos - lb.offset
            want = min(n - got, lb.block.length - boff)
            got += self._readers[idx].read_to_ptr(boff, ptr + got, want, False)
        return got

    def pread(self, off: int, n: int) -> bytes:
        out = bytearray(max(0, min(n, self.length - off)))
        got = self.pread_into(off, out, 0, len(out))
        return bytes(out[:got])

    def pread_batch_ptr(self, file_offs: list[int], n: int, dst_ptr: int,
                        stride: int) -> int:
        """Batched fixed-size reads (fio iodepth analog): read n bytes at
        each file offset into dst_ptr + i*stride.  Arena-resident reads
        issue async on one thread-local stream with ONE sync; anything
        else (file tier, block-spanning) falls back per-read.  Returns the
        number of reads served."""
        if self._native_rid is not None and len(file_offs) == 1:
            # a batch of one is a ranged read (the sequential path at
            # depth 1): no offset list to convert, block-spanning included
            if self._native.reader_pread(self._native_rid, file_offs[0], n,
                                         dst_ptr) == n:
                return 1
        import bisect
        import ctypes
        from curvine_amd import native
        if not self.fb.blocks:
            return 0
        if self._native_rid is not None:
            skipped = native.load().reader_pread_batch(
                self._native_rid, file_offs, n, dst_ptr, stride)
            for i in skipped:
                buf = bytearray(n)
                got = self.pread_into(file_offs[i], buf, 0, n)
                ctypes.memmove(dst_ptr + i * stride, bytes(buf[:got]), got)
            return len(file_offs)
        groups: dict[int, tuple[list, list]] = {}  # arena handle -> offs, dsts
        slow: list[tuple[int, int]] = []
        for i, off in enumerate(file_offs):
            idx = max(0, bisect.bisect_right(self._offs, off) - 1)
            lb = self.fb.blocks[idx]
            boff = off - lb.offset
            r = self._readers[idx]
            meta = r.meta
            if meta.get("kind") == "arena" and boff + n <= lb.block.length:
                offs, dsts = groups.setdefault(r.layout.arena.handle, ([], []))
                offs.append(meta["offset"] + boff)
                dsts.append(dst_ptr + i * stride)
            else:
                slow.append((i, off))
        mod = native.load()
        for h, (offs, dsts) in groups.items():
            mod.arena_read_batch(h, offs, dsts, n)
        for i, off in slow:
            buf = bytearray(n)
            got = self.pread_into(off, buf, 0, n)
            ctypes.memmove(dst_ptr + i * stride, bytes(buf[:got]), got)
        return len(file_offs)

    def pread_gather(self, samples: list[tuple[int, int, int]],
                     dst_ptr: int, dst_on_device: bool = False) -> int:
        """Scatter-gather variable-size reads: for each (file_off, n,
        dst_off), land bytes at dst_ptr + dst_off.  Arena-resident extents
        are grouped per arena into ONE gather call (device arenas: the
        on-chip copy_extents_kernel — the HBM-cache -> torch-device-tensor
        training-ingest path with no host hop); everything else falls back
        to pread_into_ptr DMA.  Returns total bytes gathered."""
        groups, slow, total = self.resolve_gather(samples, dst_on_device)
        self.exec_gather(groups, slow, dst_ptr)
        return total

    def resolve_gather(self, samples, dst_on_device: bool):
        """Resolution half of pread_gather, separable so callers with a
        static access pattern (CurvineDeviceLoader) resolve once and
        replay `exec_gather` per epoch.  Valid while this reader is open
        (its store readers pin the blocks)."""
        import bisect
        groups: dict[int, tuple[object, list]] = {}  # handle -> (arena, tri)
        slow: list[tuple[int, int, int]] = []
        total = 0
        for off, n, doff in samples:
            n = max(0, min(n, self.length - off))
            got = 0
            while got < n:
                idx = bisect.bisect_right(self._offs, off + got) - 1
                lb = self.fb.blocks[idx]
                boff = off + got - lb.offset
                want = min(n - got, lb.block.length - boff)
                if want <= 0:
                    break
                r = self._readers[idx]
                meta = r.meta
                arena = getattr(r.layout, "arena", None)
                is_arena = meta.get("kind") == "arena" and arena is not None
                # gather_ptr needs src and dst on the same side (device
                # kernel vs memcpy); cross-side extents use DMA fallback
                same_side = is_arena and \
                    ((arena.device >= 0) == bool(dst_on_device))
                if same_side:
                    _, tri = groups.setdefault(arena.handle, (arena, []))
                    tri.append((meta["offset"] + boff, doff + got, want))
                else:
                    slow.append((off + got, want, doff + got))
                got += want
            total += got
        return list(groups.values()), slow, total

    def exec_gather(self, groups, slow, dst_ptr: int) -> None:
        for arena, tri in groups:
            arena.gather_ptr(tri, dst_ptr)
        for off, want, doff in slow:
            self.pread_into_ptr(off, dst_ptr + doff, want)

    # ---------------- typed (dtype-converting) reads ----------------
    def resolve_convert(self, requests, dst_on_device: bool):
        """Typed analog of resolve_gather.  Each request is (file_off,
        rows, run, src_pitch, src_dtype, dst_dtype, dst_ptr) with dtype
        NAMES from native.DTYPES: `rows` runs of `run` elements,
        `src_pitch` bytes apart in the file, land densely at dst_ptr as
        dst_dtype.  Returns (groups, slow): groups = [(arena, segments)]
        ready for Arena.convert_ptr, slow = [(file_off, n_elems,
        src_dtype, dst_dtype, dst_ptr)] contiguous extents for the
        pread + host-convert path (file tier, cross-side arenas, and the
        single element that can straddle a block boundary when the data
        section starts at an odd offset).

        A request may append (scale_ptr, scale_every, scale_e0), the
        dequantising load of Arena.convert_ptr: every piece it is cut into
        carries the dense index it starts at, so each element keeps its
        own group's scale; its segments and slow entries are then 10 and 8
        fields long.

        An MX request appends (scale_ptr, scale_e0, scale_pitch, 32)
        instead: F8_E4M3 or F4 elements (`run` counts elements, two per
        byte for F4) under E8M0 block scales, scale_e0 the tensor index of
        the request's first element and scale_pitch the tensor elements
        between its runs.  Its pieces carry the tensor index THEY start
        at, which follows from where they start in the file.

        A block-scaled request appends (scale_ptr, scale_e0, scale_pitch,
        M, K, bm, bn): F8_E4M3 elements of a tensor (..., M, K) under one
        f32 scale per bm x bn tile, scale_ptr the whole scale tensor.  Its
        pieces carry the tensor index they start at in the same way, and
        every element finds its tile from its own tensor coordinates, so a
        request may cut rows and tiles anywhere."""
        import bisect

        from curvine_amd.native import DTYPE_BITS, DTYPES
        groups: dict[int, tuple[object, list]] = {}
        slow: list[tuple[int, int, str, str, int]] = []
        blocks = self.fb.blocks

        def block_at(pos):
            idx = bisect.bisect_right(self._offs, pos) - 1
            if idx < 0 or idx >= len(self._readers):
                return None
            lb = blocks[idx]
            if pos >= lb.offset + lb.block.length:
                return None
            return idx

        for off, rows, run, pitch, sdt, ddt, dptr, *scale in requests:
            if rows <= 0 or run <= 0:
                continue
            sbits, ds = DTYPE_BITS[sdt], DTYPE_BITS[ddt] // 8
            sc, dc = DTYPES[sdt], DTYPES[ddt]
            run_b = run * sbits // 8

            def scaled_at(dst, pos):
                """The scale fields of a piece that lands at dst and
                starts at file offset pos."""
                if not scale:
                    return ()
                if len(scale) == 4:
                    sptr, e0, spitch, blk = scale
                    return (sptr, e0 + (pos - off) * 8 // sbits, spitch, blk)
                if len(scale) == 7:
                    sptr, e0, spitch, *geom = scale
                    return (sptr, e0 + (pos - off) * 8 // sbits, spitch,
                            *geom)
                sptr, every, e0 = scale
                return (sptr, every, e0 + (dst - dptr) // ds)

            def emit(idx, pos, n_rows, n_run, dst):
                """n_rows runs of n_run elements, all inside block idx."""
                r = self._readers[idx]
                arena = getattr(r.layout, "arena", None)
                same_side = r.meta.get("kind") == "arena" and \
                    arena is not None and \
                    ((arena.device >= 0) == bool(dst_on_device))
                if same_side:
                    _, segs = groups.setdefault(arena.handle, (arena, []))
                    segs.append((r.meta["offset"] + pos - blocks[idx].offset,
                                 dst, n_rows, n_run, pitch, sc, dc)
                                + scaled_at(dst, pos))
                else:
                    for k in range(n_rows):
                        d_k = dst + k * n_run * ds
                        slow.append((pos + k * pitch, n_run, sdt, ddt, d_k)
                                    + scaled_at(d_k, pos + k * pitch))

            r_i = 0
            while r_i < rows:
                pos = off + r_i * pitch
                dst = dptr + r_i * run * ds
                idx = block_at(pos)
                if idx is not None:
                    end = blocks[idx].offset + blocks[idx].block.length
                    if pos + run_b <= end:
                        # every following run that also ends inside
                        cnt = rows - r_i
                        if pitch > 0:
                            cnt = min(cnt, (end - run_b - pos) // pitch + 1)
                        emit(idx, pos, cnt, run, dst)
                        r_i += cnt
                        continue
                # a run cut by a block boundary (or a hole): rows=1 pieces
                # split on whole elements
                e = 0
                while e < run:
                    p = pos + e * sbits // 8
                    idx = block_at(p)
                    if idx is None:       # hole: pread synthesizes zeros
                        slow.append((p, run - e, sdt, ddt, dst + e * ds)
                                    + scaled_at(dst + e * ds, p))
                        break
                    avail = blocks[idx].offset + blocks[idx].block.length - p
                    k = min(run - e, avail * 8 // sbits)
                    if k == 0:            # element straddles two blocks
                        slow.append((p, 1, sdt, ddt, dst + e * ds)
                                    + scaled_at(dst + e * ds, p))
                        e += 1
                        continue
                    emit(idx, p, 1, k, dst + e * ds)
                    e += k
                r_i += 1
        return list(groups.values()), slow

    def exec_convert(self, groups, slow, dst_on_device: bool) -> None:
        """Run a resolve_convert plan: one Arena.convert_ptr per arena,
        then the slow list through pread -> host convert (the kernel's own
        scalar routines) -> H2D copy or memcpy, the scales an extent needs
        fetched to the host first."""
        import ctypes

        from curvine_amd import native
        for arena, segs in groups:
            arena.convert_ptr(segs)
        for off, n, sdt, ddt, dptr, *scale in slow:
            sc, dc = native.DTYPES[sdt], native.DTYPES[ddt]
            ctype, first, count, convert = _slow_scales(scale, n)
            sbuf = (ctype * count)()
            if count:
                src = scale[0] + first * ctypes.sizeof(ctype)
                if dst_on_device:
                    native.load().memcpy_d2h(ctypes.addressof(sbuf), src,
                                             ctypes.sizeof(sbuf))
                else:
                    ctypes.memmove(sbuf, src, ctypes.sizeof(sbuf))
            nbytes = n * native.DTYPE_BITS[sdt] // 8
            raw = self.pread(off, nbytes)
            if len(raw) != nbytes:
                raise err.OutOfRange(
                    f"typed read at {off}: short read ({len(raw)} bytes)")
            self._land(convert(raw, sc, dc, sbuf), dptr, dst_on_device)

    # ---------------- token windows ----------------
    def resolve_token_windows(self, windows, src_dtype: str, seq_len: int,
                              dst_on_device: bool):
        """Resolution half of a token-window batch, modelled on
        resolve_convert.  windows = [(file_off, row)]: window `row` is
        seq_len + 1 tokens of `src_dtype` (a name from
        native.TOKEN_SOURCES) starting at byte file_off.  Returns (groups,
        slow): groups = [(arena, pieces)] with pieces (src_off, row, j0, n)
        ready for Arena.token_windows, for spans inside one arena block on
        the destinations' side; slow = [(file_off, row, j0, n)] for the
        pread + host path: file tier, cross-side arenas, holes (which read
        as zeros) and the single token that straddles two blocks when
        tokens sit at odd offsets.  Pieces split on whole tokens.  A window
        that runs past the end of the file is OutOfRange."""
        import bisect

        from curvine_amd.native import DTYPE_ITEMSIZE
        ss = DTYPE_ITEMSIZE[src_dtype]
        n_tok = seq_len + 1
        groups: dict[int, tuple[object, list]] = {}
        slow: list[tuple[int, int, int, int]] = []
        blocks = self.fb.blocks
        for off, row in windows:
            if off < 0 or off + n_tok * ss > self.length:
                raise err.OutOfRange(
                    f"token window at {off}: {n_tok} tokens run past the "
                    f"file's {self.length} bytes")
            e = 0
            while e < n_tok:
                p = off + e * ss
                hole = _hole_span(self._offs, blocks, self.length, p)
                if hole > 0:          # pread synthesizes zeros
                    k = min(n_tok - e, -(-hole // ss))
                    slow.append((p, row, e, k))
                    e += k
                    continue
                idx = bisect.bisect_right(self._offs, p) - 1
                lb = blocks[idx]
                k = min(n_tok - e, (lb.offset + lb.block.length - p) // ss)
                if k == 0:            # token straddles two blocks
                    slow.append((p, row, e, 1))
                    e += 1
                    continue
                r = self._readers[idx]
                arena = getattr(r.layout, "arena", None)
                same_side = r.meta.get("kind") == "arena" and \
                    arena is not None and \
                    ((arena.device >= 0) == bool(dst_on_device))
                if same_side:
                    _, pieces = groups.setdefault(arena.handle, (arena, []))
                    pieces.append((r.meta["offset"] + p - lb.offset, row, e, k))
                else:
                    slow.append((p, row, e, k))
                e += k
        return list(groups.values()), slow

    def exec_token_windows(self, groups, slow, x_ptr: int, y_ptr: int,
                           batch: int, seq_len: int, src_dtype: str,
                           dst_dtype: str, vocab_size: int,
                           dst_on_device: bool) -> int:
        """Run a resolve_token_windows plan into x and y, two dense
        [batch, seq_len] arrays of dst_dtype: one Arena.token_windows per
        arena, then the slow list through pread -> host widen (the kernel's
        own routine) -> H2D copy or memcpy, into the x span and the y span
        of each entry.  Returns the tokens outside [0, vocab_size), the
        slow ones counted here by the same rule (0 when vocab_size is 0)."""
        from curvine_amd import native
        sc, dc = native.DTYPES[src_dtype], native.DTYPES[dst_dtype]
        ss = native.DTYPE_ITEMSIZE[src_dtype]
        ds = native.DTYPE_ITEMSIZE[dst_dtype]
        fmt = {"U16": "H", "U32": "I", "I32": "i"}[src_dtype]
        bad = 0
        for arena, pieces in groups:
            bad += arena.token_windows(pieces, x_ptr, y_ptr, batch, seq_len,
                                       sc, dc, vocab_size)
        for off, row, j0, n in slow:
            raw = self.pread(off, n * ss)
            if len(raw) != n * ss:
                raise err.OutOfRange(
                    f"token read at {off}: short read ({len(raw)} bytes)")
            out = native.token_convert_host(raw, sc, dc, n)
            nx = min(j0 + n, seq_len) - j0      # tokens j < seq_len
            if nx > 0:
                self._land(out[:nx * ds], x_ptr + (row * seq_len + j0) * ds,
                           dst_on_device)
            y0 = max(j0, 1)                     # tokens j >= 1
            if j0 + n > y0:
                self._land(out[(y0 - j0) * ds:],
                           y_ptr + (row * seq_len + y0 - 1) * ds,
                           dst_on_device)
            if vocab_size > 0:
                bad += sum(1 for v in memoryview(raw).cast(fmt)
                           if v < 0 or v >= vocab_size)
        return bad

    # ---------------- array samples ----------------
    def resolve_array_samples(self, samples, sample_bytes: int,
                              dst_on_device: bool):
        """Resolution half of an array-sample batch, modelled on
        resolve_token_windows.  samples = [(file_off, row)]: sample `row`
        is sample_bytes uint8 bytes starting at byte file_off.  Returns
        (groups, slow): groups = [(arena, pieces)] with pieces (src_off,
        row, e0, n) ready for Arena.array_samples, one per arena block the
        sample touches, for samples whose every byte sits in arena blocks on
        the destination's side; slow = [(file_off, row)] for samples with a
        part elsewhere (file tier, cross-side arena, a hole), which go
        through pread and the host routine as a whole.  A sample that runs
        past the end of the file is OutOfRange."""
        import bisect
        groups: dict[int, tuple[object, list]] = {}
        slow: list[tuple[int, int]] = []
        blocks = self.fb.blocks
        for off, row in samples:
            if off < 0 or off + sample_bytes > self.length:
                raise err.OutOfRange(
                    f"array sample at {off}: {sample_bytes} bytes run past "
                    f"the file's {self.length} bytes")
            parts = []
            e = 0
            while e < sample_bytes:
                p = off + e
                if _hole_span(self._offs, blocks, self.length, p) > 0:
                    parts = None
                    break
                idx = bisect.bisect_right(self._offs, p) - 1
                lb = blocks[idx]
                r = self._readers[idx]
                arena = getattr(r.layout, "arena", None)
                same_side = r.meta.get("kind") == "arena" and \
                    arena is not None and \
                    ((arena.device >= 0) == bool(dst_on_device))
                if not same_side:
                    parts = None
                    break
                k = min(sample_bytes - e, lb.offset + lb.block.length - p)
                parts.append((arena, (r.meta["offset"] + p - lb.offset, row,
                                      e, k)))
                e += k
            if parts is None:
                slow.append((off, row))
                continue
            for arena, piece in parts:
                groups.setdefault(arena.handle, (arena, []))[1].append(piece)
        return list(groups.values()), slow

    def exec_array_samples(self, groups, slow, out_ptr: int, batch: int,
                           rows, shape, crop, scale, bias, dst_dtype: str,
                           layout: str, dst_on_device: bool) -> None:
        """Run a resolve_array_samples plan into a dense [batch, C, h, w]
        (or [batch, h, w, C]) array of dst_dtype at out_ptr, rows[b] = (dy,
        dx, flip): one Arena.array_samples per arena, then every slow sample
        through pread -> native.array_sample_host (the kernel's own routine)
        -> H2D copy or memcpy into its contiguous C*h*w range."""
        from curvine_amd import native
        dc = native.DTYPES[dst_dtype]
        H, W, C = shape
        for arena, pieces in groups:
            arena.array_samples(pieces, rows, out_ptr, batch, shape, crop,
                                scale, bias, dc, layout)
        sample_bytes = H * W * C
        out_b = C * crop[0] * crop[1] * native.DTYPE_ITEMSIZE[dst_dtype]
        for off, row in slow:
            raw = self.pread(off, sample_bytes)
            if len(raw) != sample_bytes:
                raise err.OutOfRange(
                    f"array read at {off}: short read ({len(raw)} bytes)")
            dy, dx, flip = rows[row]
            out = native.array_sample_host(raw, dy, dx, flip, shape, crop,
                                           scale, bias, dc, layout)
            self._land(out, out_ptr + row * out_b, dst_on_device)

    # ---------------- document-packed token batches ----------------
    def _token_parts(self, off: int, n_tok: int, ss: int,
                     dst_on_device: bool):
        """Cut n_tok tokens of ss bytes at file byte `off` on whole tokens
        at block boundaries: yields (arena or None, src_off or file_off,
        e, k) for tokens e .. e+k-1.  arena is None for what has to go
        through pread: file tier, cross-side arenas, holes (which read as
        zeros) and the single token that straddles two blocks."""
        import bisect
        blocks = self.fb.blocks
        e = 0
        while e < n_tok:
            p = off + e * ss
            hole = _hole_span(self._offs, blocks, self.length, p)
            if hole > 0:
                k = min(n_tok - e, -(-hole // ss))
                yield None, p, e, k
                e += k
                continue
            idx = bisect.bisect_right(self._offs, p) - 1
            lb = blocks[idx]
            k = min(n_tok - e, (lb.offset + lb.block.length - p) // ss)
            if k == 0:                # token straddles two blocks
                yield None, p, e, 1
                e += 1
                continue
            r = self._readers[idx]
            arena = getattr(r.layout, "arena", None)
            same_side = r.meta.get("kind") == "arena" and \
                arena is not None and \
                ((arena.device >= 0) == bool(dst_on_device))
            if same_side:
                yield arena, r.meta["offset"] + p - lb.offset, e, k
            else:
                yield None, p, e, k
            e += k

    def token_eos_index(self, src_dtype: str, header_bytes: int, eos_id: int,
                        dst_on_device: bool):
        """The document index of a token file: the ascending array('q') of
        the token indices (token t sits at byte header_bytes + t *
        itemsize) whose value is eos_id.  Spans inside arena blocks on the
        side `dst_on_device` names go through Arena.token_eos_index, one
        count call and one write call per arena and one copy back;
        everything else (file tier, cross-side arenas, holes, a token that
        straddles two blocks) through pread and native.token_eos_index_host
        in bounded chunks.  A trailing partial token is ignored."""
        import array
        import ctypes

        from curvine_amd import native
        sc = native.DTYPES[src_dtype]
        ss = native.DTYPE_ITEMSIZE[src_dtype]
        if header_bytes < 0:
            raise err.InvalidArgument("token eos index: negative header_bytes")
        n_tok = max(0, self.length - header_bytes) // ss
        groups: dict[int, tuple[object, list]] = {}
        runs = []                     # ascending arrays, one per source
        slow = array.array("q")
        step = (4 << 20) // ss        # tokens per pread
        for arena, at, e, k in self._token_parts(header_bytes, n_tok, ss,
                                                 dst_on_device):
            if arena is not None:
                groups.setdefault(arena.handle, (arena, []))[1].append(
                    (at, e, k))
                continue
            for c in range(0, k, step):
                kk = min(step, k - c)
                raw = self.pread(at + c * ss, kk * ss)
                if len(raw) != kk * ss:
                    raise err.OutOfRange(
                        f"token read at {at + c * ss}: short read "
                        f"({len(raw)} bytes)")
                slow.frombytes(native.token_eos_index_host(
                    raw, sc, eos_id, e + c, kk))
        if len(slow):
            runs.append(slow)
        for arena, spans in groups.values():
            total = arena.token_eos_index(spans, sc, eos_id, 0, 0)
            if not total:
                continue
            got = array.array("q")
            if arena.device >= 0:
                import torch
                t = torch.empty(total, dtype=torch.int64,
                                device=f"cuda:{arena.device}")
                arena.token_eos_index(spans, sc, eos_id, t.data_ptr(), total)
                got.frombytes(t.cpu().numpy().tobytes())
            else:
                buf = (ctypes.c_int64 * total)()
                arena.token_eos_index(spans, sc, eos_id,
                                      ctypes.addressof(buf), total)
                got.frombytes(bytes(buf))
            runs.append(got)
        if len(runs) == 1:
            return runs[0]
        merged = array.array("q")
        for r in runs:
            merged.extend(r)
        return array.array("q", sorted(merged))   # ascending runs: one merge

    def resolve_token_pack(self, items, src_dtype: str, dst_on_device: bool):
        """Resolution half of a packed batch, modelled on
        resolve_token_windows.  items = [(file_off, segment, n_tok)]:
        source segment `segment` of the batch reads n_tok tokens (its n,
        plus one when the document goes on) of `src_dtype` from byte
        file_off.  Returns (groups, slow): groups = [(arena, pieces)] with
        pieces (src_off, segment, j0, k) ready for Arena.token_pack, for
        spans inside one arena block on the destinations' side; slow =
        [(file_off, segment, j0, k)] for the pread + host path.  Pieces
        split on whole tokens.  A segment that runs past the end of the
        file is OutOfRange."""
        from curvine_amd.native import DTYPE_ITEMSIZE
        ss = DTYPE_ITEMSIZE[src_dtype]
        groups: dict[int, tuple[object, list]] = {}
        slow: list[tuple[int, int, int, int]] = []
        for off, seg, n_tok in items:
            if off < 0 or off + n_tok * ss > self.length:
                raise err.OutOfRange(
                    f"token segment at {off}: {n_tok} tokens run past the "
                    f"file's {self.length} bytes")
            for arena, at, e, k in self._token_parts(off, n_tok, ss,
                                                     dst_on_device):
                if arena is not None:
                    groups.setdefault(arena.handle, (arena, []))[1].append(
                        (at, seg, e, k))
                else:
                    slow.append((at, seg, e, k))
        return list(groups.values()), slow

    def exec_token_pack(self, groups, slow, segments, x_ptr: int, y_ptr: int,
                        pos_ptr: int, doc_ptr: int, cu_ptr: int, rows: int,
                        seq_len: int, src_dtype: str, dst_dtype: str,
                        pad_id: int, ignore_index: int, vocab_size: int,
                        dst_on_device: bool, fill: bool | None = None) -> int:
        """Run a resolve_token_pack plan into the outputs of a packed
        batch (`segments` as Arena.token_pack takes them; y_ptr, pos_ptr,
        doc_ptr and cu_ptr may be 0): one Arena.token_pack per arena, which
        also fills the pad segments and cu_seqlens, then the slow list
        through pread -> native.token_pack_piece_host -> H2D copy or
        memcpy, into every requested output.  With `fill` the pad
        segments and cu_seqlens go the slow way too; by default that
        happens when there is no arena call to do it.  A caller that
        spreads one batch over several readers passes fill=False to all
        but one.  Returns the tokens outside [0, vocab_size) (0 when
        vocab_size is 0)."""
        import struct

        from curvine_amd import native
        sc, dc = native.DTYPES[src_dtype], native.DTYPES[dst_dtype]
        ss = native.DTYPE_ITEMSIZE[src_dtype]
        ds = native.DTYPE_ITEMSIZE[dst_dtype]
        bad = 0
        for arena, pieces in groups:
            bad += arena.token_pack(segments, pieces, x_ptr, y_ptr, pos_ptr,
                                    doc_ptr, cu_ptr, rows, seq_len, sc, dc,
                                    pad_id, ignore_index, vocab_size)
        if fill is None:
            fill = not groups

        def land(parts, at, y_at):
            x, y, pos, doc, _bad = parts
            for out, ptr, a in ((x, x_ptr, at), (y, y_ptr, y_at),
                                (pos, pos_ptr, at), (doc, doc_ptr, at)):
                if ptr and out:
                    self._land(out, ptr + a * ds, dst_on_device)
            return _bad
        for off, seg, j0, k in slow:
            row, col, n, pos0, doc, _seq, flags = segments[seg]
            raw = self.pread(off, k * ss)
            if len(raw) != k * ss:
                raise err.OutOfRange(
                    f"token read at {off}: short read ({len(raw)} bytes)")
            at = row * seq_len + col
            bad += land(native.token_pack_piece_host(
                raw, n, pos0, doc, flags, j0, k, sc, dc, pad_id,
                ignore_index, vocab_size), at + j0, at + max(j0, 1) - 1)
        if fill:
            for row, col, n, pos0, doc, _seq, flags in segments:
                if flags & native.TOKEN_SEG_PAD:
                    at = row * seq_len + col
                    land(native.token_pack_piece_host(
                        b"", n, pos0, doc, flags, 0, n, sc, dc, pad_id,
                        ignore_index, 0), at, at)
            if cu_ptr:
                cu = [0] * (len(segments) + 1)
                for row, col, _n, _p, _d, seq, _f in segments:
                    cu[seq] = row * seq_len + col
                cu[len(segments)] = rows * seq_len
                self._land(struct.pack(f"<{len(cu)}i", *cu), cu_ptr,
                           dst_on_device)
        return bad

    @staticmethod
    def _land(out: bytes, dptr: int, dst_on_device: bool) -> None:
        import ctypes

        from curvine_amd import native
        if dst_on_device:
            buf = (ctypes.c_char * len(out)).from_buffer_copy(out)
            native.load().memcpy_h2d(dptr, ctypes.addressof(buf), len(out))
        else:
            ctypes.memmove(dptr, out, len(out))

    def verify(self) -> list[int]:
        """Recompute every resident block's CRC32C (HBM: device kernel)
        against the worker's publish-time value; returns block ids that
        no longer match (bit rot / unexpected mutation).  Blocks without
        a stored CRC (rewritten in place) are skipped."""
        bad = []
        for lb, r in zip(self.fb.blocks, self._readers):
            stored = r.meta.get("crc32c")
            if stored is None:
                continue
            if r.crc32c(0, lb.block.length) != stored:
                bad.append(lb.block.block_id)
        return bad

    def close(self) -> None:
        if getattr(self, "_native_rid", None) is not None:
            # unregister BEFORE releasing the store readers that pin the
            # registered extents
            try:
                from curvine_amd import native
                native.load().reader_unregister(self._native_rid)
            except Exception:  # noqa: BLE001
                pass
            self._native_rid = None
        for r in getattr(self, "_readers", []):
            try:
                r.close()
            except Exception:  # noqa: BLE001
                pass
        self._readers = []


class FsReader:
    def __init__(self, client: FsClient, file_blocks: FileBlocks):
        self.client = client
        self.fb = file_blocks
        try:
            self._loop = __import__("asyncio").get_running_loop()
        except RuntimeError:
            self._loop = None
        self.status = file_blocks.status
        self.length = self.status.length
        self.pos = 0
        self.detector = ReadDetector()
        self._readers: dict[int, object] = {}   # block index -> reader
        self.failed_workers: set[int] = set()
        self.chunk_size = client.conf.client.read_chunk_size
        self.parallel = max(1, client.conf.client.read_parallel)
        self.slice_size = client.conf.client.read_slice_size

    # ---------------- block reader selection ----------------
    def _block_at(self, off: int) -> tuple[int, LocatedBlock, int]:
        """(index, located block, offset within block).  Blocks can be
        shorter than block_size mid-file (appends), so search by offset."""
        import bisect
        offs = getattr(self, "_block_offs", None)
        if offs is None or len(offs) != len(self.fb.blocks):
            offs = [b.offset for b in self.fb.blocks]
            self._block_offs = offs
        idx = bisect.bisect_right(offs, off) - 1
        if idx < 0 or idx >= len(self.fb.blocks):
            raise err.OutOfRange(f"offset {off} beyond {self.length}")
        lb = self.fb.blocks[idx]
        return idx, lb, off - lb.offset

    async def _reader_for(self, idx: int):
        r = self._readers.get(idx)
        if r is not None:
            return r
        lb = self.fb.blocks[idx]
        r = await self._open_block_reader(lb)
        self._readers[idx] = r
        return r

    async def _open_block_reader(self, lb: LocatedBlock):
        if not lb.locations:
            # no cached replica: sparse hole (or caller falls back to UFS)
            return BlockReaderHole(lb.block.length)
        from curvine_amd.worker import registry
        candidates = [a for a in lb.locations
                      if a.worker_id not in self.failed_workers] or lb.locations
        # in-process short-circuit first
        if self.client.conf.client.short_circuit:
            for addr in candidates:
                store = registry.lookup(addr.worker_id)
                if store is not None:
                    try:
                        return BlockReaderLocal(store, lb.block.block_id)
                    except Exception:  # noqa: BLE001
                        self.failed_workers.add(addr.worker_id)
        # cross-process HBM short-circuit: a colocated worker in another
        # process discloses its arena via hipIpc — direct DMA reads here
        if self.client.conf.client.short_circuit:
            from curvine_amd.client.block_client import (AsyncIpcReader,
                                                         open_ipc_reader)
            for addr in candidates:
                ipc = await open_ipc_reader(self.client, addr,
                                            lb.block.block_id)
                if ipc is not None:
                    return AsyncIpcReader(ipc)
        last: Exception = err.BlockNotFound(str(lb.block.block_id))
        for addr in candidates:
            try:
                r = BlockReaderRemote(addr, lb.block.block_id)
                return r
            except Exception as e:  # noqa: BLE001
                self.failed_workers.add(addr.worker_id)
                last = e
        raise last

    # ---------------- reads ----------------
    async def pread(self, off: int, n: int) -> bytes:
        n = max(0, min(n, self.length - off))
        if n == 0:
            return b""
        out = bytearray(n)
        got = await self.pread_into(off, out, 0, n)
        return bytes(out[:got])

    async def pread_into(self, off: int, out, out_off: int, n: int) -> int:
        n = max(0, min(n, self.length - off))
        if n == 0:
            return 0
        self.detector.observe(off, n)
        if n >= self.slice_size and self.parallel > 1:
            return await self._pread_parallel(off, out, out_off, n)
        got = 0
        while got < n:
            pos = off + got
            hole = _hole_span(self._block_offsets(), self.fb.blocks,
                              self.length, pos)
            if hole > 0:
                fill = min(hole, n - got)
                out[out_off + got:out_off + got + fill] = b"\x00" * fill
                got += fill
                continue
            idx, lb, boff = self._block_at(pos)
            want = min(n - got, lb.block.length - boff)
            if want <= 0:
                break
            r = await self._reader_for(idx)
            rn = await self._read_with_fallback(idx, r, boff, out,
                                                out_off + got, want)
            if rn <= 0:
                break
            got += rn
        return got

    def _block_offsets(self) -> list:
        offs = getattr(self, "_block_offs", None)
        if offs is None or len(offs) != len(self.fb.blocks):
            offs = [b.offset for b in self.fb.blocks]
            self._block_offs = offs
        return offs

    async def _read_with_fallback(self, idx, reader, boff, out, out_off, want):
        try:
            return await reader.read_into(boff, out, out_off, want)
        except Exception:  # noqa: BLE001 — replica failed mid-read
            self._readers.pop(idx, None)
            lb = self.fb.blocks[idx]
            r2 = await self._open_block_reader(lb)
            self._readers[idx] = r2
            return await r2.read_into(boff, out, out_off, want)

    async def _pread_parallel(self, off, out, out_off, n) -> int:
        """Slice fan-out (fs_reader_parallel.rs:94-131 analog)."""
        k = min(self.parallel, (n + self.slice_size - 1) // self.slice_size)
        per = (n + k - 1) // k
        tasks = []
        for i in range(k):
            so = off + i * per
            sn = min(per, off + n - so)
            if sn <= 0:
                break
            tasks.append(self._pread_slice(so, out, out_off + i * per, sn))
        results = await asyncio.gather(*tasks)
        return sum(results)

    async def _pread_slice(self, off, out, out_off, n) -> int:
        got = 0
        while got < n:
            pos = off + got
            hole = _hole_span(self._block_offsets(), self.fb.blocks,
                              self.length, pos)
            if hole > 0:
                fill = min(hole, n - got)
                out[out_off + got:out_off + got + fill] = b"\x00" * fill
                got += fill
                continue
            idx, lb, boff = self._block_at(pos)
            want = min(n - got, lb.block.length - boff)
            if want <= 0:
                break
            r = await self._reader_for(idx)
            rn = await self._read_with_fallback(idx, r, boff, out,
                                                out_off + got, want)
            if rn <= 0:
                break
            got += rn
        return got

    async def read(self, n: int = -1) -> bytes:
        if n < 0:
            n = self.length - self.pos
        data = await self.pread(self.pos, n)
        self.pos += len(data)
        return data

    def seek(self, pos: int) -> None:
        self.pos = pos

    async def pread_to_device(self, off: int, dst_ptr: int, n: int) -> int:
        """Read file bytes directly into consumer GPU memory
        (hipMemcpyDtoD from the HBM arena when local, staged otherwise)."""
        n = max(0, min(n, self.length - off))
        got = 0
        while got < n:
            idx, lb, boff = self._block_at(off + got)
            want = min(n - got, lb.block.length - boff)
            if want <= 0:
                break
            r = await self._reader_for(idx)
            if isinstance(r, BlockReaderLocal):
                rn = await r.read_to_device(boff, dst_ptr + got, want)
            else:
                # remote block: fetch to pinned host memory, then H2D
                from curvine_amd import native
                pbuf = native.PinnedBuffer(want)
                try:
                    rn = await r.read_into(boff, pbuf.view, 0, want)
                    if rn > 0:
                        loop = asyncio.get_event_loop()
                        await loop.run_in_executor(
                            None, native.load().memcpy_h2d,
                            dst_ptr + got, pbuf.ptr, rn)
                finally:
                    pbuf.close()
            got += rn
        return got

    def to_sync(self) -> SyncLocalReader:
        """Short-circuit sync view (raises if any block lacks a local
        in-process OR hipIpc-mapped replica)."""
        return SyncLocalReader(self.fb, ipc_resolver=self._ipc_resolver)

    def _ipc_resolver(self, lb):
        """Sync bridge for SyncLocalReader: map a colocated
        other-process HBM block via the client's event loop."""
        import asyncio as _a
        if not self.client.conf.client.short_circuit or self._loop is None:
            return None
        try:
            if _a.get_running_loop() is self._loop:
                return None   # would deadlock; caller stays async
        except RuntimeError:
            pass
        from curvine_amd.client.block_client import open_ipc_reader
        for addr in lb.locations:
            try:
                fut = _a.run_coroutine_threadsafe(
                    open_ipc_reader(self.client, addr, lb.block.block_id),
                    self._loop)
                ipc = fut.result(30)
            except Exception:  # noqa: BLE001
                continue
            if ipc is not None:
                return ipc
        return None

    def close(self) -> None:
        for r in self._readers.values():
            try:
                r.close()
            except Exception:  # noqa: BLE001
                pass
        self._readers.clear()
