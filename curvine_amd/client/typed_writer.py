"""TypedFileWriter: writes a file whose whole layout is known up front —
some header bytes, then typed tensors back to back (a safetensors
checkpoint) — and lets every block whose content allows it take the typed
store: `BlockWriter.store_typed` converts and copies the sources where
they are (one store_segments_kernel launch per HBM block, csrc/
tensor_cast.hip), with no host hop and no host hashing.

A block takes the typed store when it has exactly one location, that
location is an in-process store and the block landed in an arena on the
same side as every source it holds (HBM of the tensors' own GPU, or a host
arena for cpu tensors).  Any other block (file tier, remote worker,
replicas > 1, sources elsewhere) is materialised on the host, cast with
`native.convert_host` — the kernel's own scalar routines, so both paths
give identical bits — and sent through the ordinary block writers.

A source stored as F8_E4M3 carries the f32 scales of its groups
(`scale_ptr`, `scale_every`): each piece of it tells the store which dense
element of the tensor it starts at, so a tensor cut by a block boundary
keeps dividing every row by that row's scale, and the byte path hands the
same scales to `convert_host`.

An MX source (`mx`: stored as F8_E4M3 or F4 under E8M0 block scales, one
byte per 32 elements at `scale_ptr`) is carried the same way: each piece
names the dense element it starts at, which may be mid-block, and the byte
path hands the scale bytes to `mx_convert_host`.  F4 packs two elements
per byte, so sizes here are counted in bits.

A block-scaled source (`block`: stored as F8_E4M3 under one f32 scale per
bm x bn tile of its last two dimensions) also names the dense element each
piece starts at; the store finds every element's tile from its tensor
coordinates, so a piece may be cut mid-row and mid-tile, and the byte path
hands the whole scale tensor to `block_convert_host`.
"""
from __future__ import annotations

import asyncio
from dataclasses import dataclass
from typing import Callable

from curvine_amd import errors as err
from curvine_amd.client.block_client import (BlockWriterLocal,
                                             make_block_writer)
from curvine_amd.client.fs_client import FsClient
from curvine_amd.model import FileStatus
from curvine_amd.native import (DTYPE_BITS, DTYPE_ITEMSIZE, DTYPES, MX_BLOCK,
                                block_quantize_supported, convert_supported,
                                mx_quantize_supported, quantize_supported)


@dataclass
class TypedSource:
    """`rows` runs of `run` elements of `src_dt`, `pitch` bytes apart at
    the absolute address `ptr`, stored densely as `dst_dt` from `file_off`.
    `device` is -1 for host memory or the GPU index.  `read_host(e0, e1)`
    returns the source-dtype bytes of dense elements [e0, e1) as a host
    buffer (the byte path).

    Stored as F8_E4M3 the source is quantised: `scale_ptr` is the address
    (on the source's side) of the f32 scales of its tensor, dense element e
    using scale e // `scale_every` (0: one scale), and `scales_host()`
    returns the same scales as a host buffer (the byte path).

    `mx`: stored as F8_E4M3 or F4, `scale_ptr` the address of the tensor's
    E8M0 bytes, dense element e using byte e // 32; `scales_host()` as
    above.  The dense tensor's rows end on a block boundary, so `run` is a
    multiple of 32 wherever there is more than one row.

    `block` = (M, K, bm, bn): stored as F8_E4M3, the dense elements being a
    tensor (..., M, K) and `scale_ptr` the address of its f32 tile scales,
    shape (..., ceil(M/bm), ceil(K/bn)); `scales_host()` as above."""
    file_off: int
    ptr: int
    rows: int
    run: int
    pitch: int
    src_dt: str
    dst_dt: str
    device: int
    read_host: Callable[[int, int], object]
    scale_ptr: int = 0
    scale_every: int = 0
    scales_host: Callable[[], object] | None = None
    mx: bool = False
    block: tuple | None = None

    @property
    def scaled(self) -> bool:
        return self.scale_ptr != 0

    @property
    def numel(self) -> int:
        return self.rows * self.run

    @property
    def nbytes(self) -> int:
        return self.numel * DTYPE_BITS[self.dst_dt] // 8

    def pieces(self, e0: int, e1: int):
        """(ptr, rows, run) of dense elements [e0, e1): at most a partial
        first row, whole rows and a partial last row."""
        ss = DTYPE_ITEMSIZE[self.src_dt]
        if self.rows == 1 or self.pitch == self.run * ss:
            return [(self.ptr + e0 * ss, 1, e1 - e0)]
        r0, c0 = divmod(e0, self.run)
        r1, c1 = divmod(e1, self.run)
        if r0 == r1:
            return [(self.ptr + r0 * self.pitch + c0 * ss, 1, c1 - c0)]
        out = []
        if c0:
            out.append((self.ptr + r0 * self.pitch + c0 * ss, 1,
                        self.run - c0))
            r0 += 1
        if r1 > r0:
            out.append((self.ptr + r0 * self.pitch, r1 - r0, self.run))
        if c1:
            out.append((self.ptr + r1 * self.pitch, 1, c1))
        return out


def validate_layout(header: bytes, sources: list[TypedSource],
                    block_size: int) -> int:
    """Everything that can be refused without touching the cluster;
    returns the file length."""
    if block_size <= 0 or block_size % 8:
        raise err.InvalidArgument(
            f"typed write: block_size {block_size} is not a positive "
            f"multiple of 8 (an element could straddle two blocks)")
    pos = len(header)
    for s in sources:
        if s.src_dt not in DTYPES or s.dst_dt not in DTYPES:
            raise err.InvalidArgument(
                f"typed write: unknown dtype {s.src_dt!r}/{s.dst_dt!r}")
        if s.mx:
            if not mx_quantize_supported(s.src_dt, s.dst_dt):
                raise err.Unsupported(
                    f"typed write: no MX store of {s.src_dt} as {s.dst_dt}")
            if not s.scale_ptr or s.scales_host is None or \
                    s.numel % MX_BLOCK or (s.rows > 1 and s.run % MX_BLOCK):
                raise err.InvalidArgument(
                    "typed write: MX source without scales or not in "
                    "blocks of 32")
        elif s.block is not None:
            if s.dst_dt != "F8_E4M3" or \
                    not block_quantize_supported(s.src_dt):
                raise err.Unsupported(
                    f"typed write: no block-scaled store of {s.src_dt} as "
                    f"{s.dst_dt}")
            if not s.scale_ptr or s.scale_ptr % 4 or \
                    s.scales_host is None or len(s.block) != 4 or any(
                        not isinstance(v, int) or v <= 0 for v in s.block):
                raise err.InvalidArgument(
                    "typed write: block-scaled source without scales or "
                    "with a bad geometry")
        elif s.scaled:
            if s.dst_dt != "F8_E4M3" or not quantize_supported(s.src_dt):
                raise err.Unsupported(
                    f"typed write: no scaled store of {s.src_dt} as "
                    f"{s.dst_dt}")
            if s.scale_ptr % 4 or s.scale_every < 0 or s.scales_host is None:
                raise err.InvalidArgument(
                    "typed write: misaligned or incomplete scale")
        elif not convert_supported(s.src_dt, s.dst_dt):
            raise err.Unsupported(
                f"typed write: cannot store {s.src_dt} as {s.dst_dt}")
        ss = DTYPE_ITEMSIZE[s.src_dt]
        ds = max(1, DTYPE_BITS[s.dst_dt] // 8)
        if s.rows <= 0 or s.run <= 0 or s.ptr <= 0 or s.ptr % ss:
            raise err.InvalidArgument(
                "typed write: empty, null or misaligned source")
        if s.rows > 1 and s.pitch < s.run * ss:
            raise err.InvalidArgument("typed write: rows overlap")
        if s.file_off != pos or pos % ds:
            raise err.InvalidArgument(
                f"typed write: source at {s.file_off} leaves a gap or is "
                f"not aligned to its itemsize (expected {pos})")
        pos += s.nbytes
    return pos


class TypedFileWriter:
    def __init__(self, client: FsClient, status: FileStatus, header: bytes,
                 sources: list[TypedSource]):
        self.client = client
        self.status = status
        self.path = status.path
        self.block_size = status.block_size
        self.header = bytes(header)
        self.sources = sources
        # the master may have chosen the block size: check what it returned
        self.length = validate_layout(self.header, sources, self.block_size)
        self.chunk_size = client.conf.client.write_chunk_size
        self._crc_on = bool(client.conf.client.enable_crc)
        self._writers: list = []
        self._block_lens: list[int] = []
        self._commits: list[dict] = []
        self.fast_blocks = 0     # blocks that took the typed store
        self.byte_blocks = 0

    # ---- what lies in [b0, b1) of the file ----
    def _content(self, b0: int, b1: int):
        """(header part, [(source, block_off, e0, e1)])."""
        head = self.header[b0:b1] if b0 < len(self.header) else b""
        parts = []
        for s in self.sources:
            lo, hi = max(b0, s.file_off), min(b1, s.file_off + s.nbytes)
            if lo < hi:
                bits = DTYPE_BITS[s.dst_dt]
                parts.append((s, lo - b0, (lo - s.file_off) * 8 // bits,
                              (hi - s.file_off) * 8 // bits))
        return head, parts

    def _typed_target(self, parts) -> bool:
        """One in-process location whose block sits in an arena on the
        sources' side."""
        if len(self._writers) != 1:
            return False
        w = self._writers[0]
        if not isinstance(w, BlockWriterLocal):
            return False
        arena = getattr(w.writer.layout, "arena", None)
        return arena is not None and all(
            s.device == arena.device for s, _o, _e0, _e1 in parts)

    @staticmethod
    def _typed_pieces(parts):
        pieces = []
        for s, off, e0, e1 in parts:
            bits = DTYPE_BITS[s.dst_dt]
            e = e0                    # the piece's first dense element
            for ptr, rows, run in s.pieces(e0, e1):
                piece = (off, ptr, rows, run, s.pitch,
                         DTYPES[s.src_dt], DTYPES[s.dst_dt])
                if s.mx:              # the dense side is the tensor
                    piece += (s.scale_ptr, e, run, MX_BLOCK)
                elif s.block is not None:
                    piece += (s.scale_ptr, e, run) + tuple(s.block)
                elif s.scaled:
                    piece += (s.scale_ptr, s.scale_every, e)
                pieces.append(piece)
                off += rows * run * bits // 8
                e += rows * run
        return pieces

    @staticmethod
    def _host_bytes(parts, base: int, n: int) -> bytearray:
        """The data part [base, base + n) of a block, built on the host."""
        from curvine_amd import native
        buf = bytearray(n)
        for s, off, e0, e1 in parts:
            raw = s.read_host(e0, e1)
            if s.mx:
                raw = native.mx_convert_host(
                    raw, DTYPES[s.src_dt], DTYPES[s.dst_dt], e1 - e0,
                    s.scales_host(), e0)
            elif s.block is not None:
                raw = native.block_convert_host(
                    raw, DTYPES[s.src_dt], DTYPES[s.dst_dt], e1 - e0,
                    s.scales_host(), e0, *s.block)
            elif s.scaled:
                raw = native.convert_host(
                    raw, DTYPES[s.src_dt], DTYPES[s.dst_dt], e1 - e0,
                    scales=s.scales_host(), scale_every=s.scale_every,
                    scale_e0=e0)
            elif s.src_dt != s.dst_dt:
                raw = native.convert_host(raw, DTYPES[s.src_dt],
                                          DTYPES[s.dst_dt], e1 - e0)
            raw = memoryview(raw).cast("B")
            n_b = (e1 - e0) * DTYPE_BITS[s.dst_dt] // 8
            if len(raw) != n_b:
                raise err.FsError(
                    f"typed write: source gave {len(raw)} bytes for {n_b}")
            buf[off - base:off - base + n_b] = raw
        return buf

    async def _write_bytes(self, data, crc: int) -> int:
        from curvine_amd import native
        view = memoryview(data)
        for o in range(0, len(view), self.chunk_size):
            chunk = view[o:o + self.chunk_size]
            await asyncio.gather(*[w.write(chunk) for w in self._writers])
            if self._crc_on:
                crc = native.crc32c(chunk, crc)
        return crc

    async def _write_block(self, b0: int, b1: int) -> None:
        lb = await self.client.add_block(self.path)
        if not lb.locations:
            raise err.NoAvailableWorker(self.path)
        self._writers = [make_block_writer(addr, lb.block.block_id,
                                           self.block_size, tier)
                         for addr, tier in zip(lb.locations, lb.tiers)]
        head, parts = self._content(b0, b1)
        crc, crc_valid = 0, True
        if head:                      # header bytes: ordinary byte write
            crc = await self._write_bytes(head, crc)
        if parts:
            stored = False
            if self._typed_target(parts):
                loop = asyncio.get_running_loop()
                try:
                    await loop.run_in_executor(
                        None, self._writers[0].writer.store_typed,
                        self._typed_pieces(parts))
                    stored = True
                except err.Unsupported:
                    pass              # layout takes no pointer: write bytes
            if stored:
                # no client-side CRC of bytes that never were on the host:
                # the worker's publish-time CRC stands alone (as after
                # FsWriter.pwrite_at)
                crc_valid = False
                self.fast_blocks += 1
            else:
                loop = asyncio.get_running_loop()
                data = await loop.run_in_executor(
                    None, self._host_bytes, parts, len(head),
                    b1 - b0 - len(head))
                crc = await self._write_bytes(data, crc)
                self.byte_blocks += 1
        length = b1 - b0
        tiers = await asyncio.gather(
            *[w.commit(length) for w in self._writers])
        if self._crc_on and crc_valid:
            for w in self._writers:
                got = getattr(w, "last_crc", None)
                if got is not None and got != crc:
                    raise err.ChecksumMismatch(
                        f"block {lb.block.block_id}: worker crc {got:#010x} "
                        f"!= client {crc:#010x}")
        tiers = [t or hint for t, hint in zip(tiers, lb.tiers)]
        self._commits.append({
            "block_id": lb.block.block_id,
            "locations": [a.worker_id for a in lb.locations],
            "tiers": tiers})
        self._block_lens.append(length)
        self._writers = []

    async def run(self) -> FileStatus:
        """Write every block, then complete the file.  On any error the
        open block writers are aborted (as FsWriter.abort does)."""
        try:
            for b0 in range(0, self.length, self.block_size):
                await self._write_block(
                    b0, min(b0 + self.block_size, self.length))
            return await self.client.complete_file(
                self.path, self.length, self._block_lens, self._commits)
        except BaseException:
            await self.abort()
            raise

    async def abort(self) -> None:
        ws, self._writers = self._writers, []
        for w in ws:
            try:
                await w.abort()
            except Exception:  # noqa: BLE001
                pass
