"""Loader/wrapper for the native HIP data plane (csrc/ -> _native.so).

Policy: on a machine WITH a GPU the native extension is mandatory — ops
fail loudly rather than falling back to a silent CPU path.  On CPU-only
machines the same extension is still used (its host-memory arena code), so
CPU tests exercise the identical C++ code paths.

If the .so is missing, we build it in-tree with hipcc (gfx950 cross-compile
works without a GPU; ~15 s cold).
"""
from __future__ import annotations

import os
import subprocess
import sys
import sysconfig
import threading

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_REPO, "curvine_amd", "_native.so")
_CSRC = os.path.join(_REPO, "csrc")
_SRC = os.path.join(_CSRC, "module.cpp")   # includes every other file there
_lock = threading.Lock()
_mod = None


def build_native(force: bool = False) -> str:
    """Compile csrc/ into curvine_amd/_native.so for gfx950.  The .so is
    stale when any csrc/*.cpp, *.hip or *.h is newer than it."""
    if not force and os.path.exists(_SO) and os.path.exists(_SRC):
        sources = [os.path.join(_CSRC, f) for f in os.listdir(_CSRC)
                   if f.endswith((".cpp", ".hip", ".h"))]
        if os.path.getmtime(_SO) >= max(map(os.path.getmtime, sources)):
            return _SO
    import pybind11
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
           "-shared", "-msse4.2",
           f"-I{pybind11.get_include()}",
           f"-I{sysconfig.get_paths()['include']}",
           _SRC, "-o", _SO]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return _SO


def load():
    global _mod
    if _mod is not None:
        return _mod
    with _lock:
        if _mod is not None:
            return _mod
        # Load torch's bundled HIP runtime first: loading /opt/rocm's
        # libamdhip64 ahead of torch breaks torch.cuda init ("No HIP GPUs
        # are available") — observed on the MI355X pool (torch 2.10+rocm7.0
        # vs /opt/rocm 7.2).  Harmless when torch is absent.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            from curvine_amd import _native as mod  # type: ignore
        except ImportError:
            build_native()
            import importlib
            import curvine_amd
            importlib.invalidate_caches()
            from curvine_amd import _native as mod  # type: ignore
        _mod = mod
        return mod


def gpu_available() -> bool:
    try:
        return load().device_count() > 0
    except Exception:
        return False


def device_count() -> int:
    return load().device_count()


class Arena:
    """A contiguous byte arena: HBM (device >= 0) or host memory
    (device == -1).  Byte movement only; offset allocation is the caller's
    (see curvine_amd.worker.arena_alloc)."""

    def __init__(self, device: int, capacity: int,
                 staging_bytes: int = 4 << 20, staging_count: int = 8,
                 host_pinned: bool = False):
        self._n = load()
        self.device = device
        self.capacity = capacity
        self.handle = self._n.arena_create(device, capacity, staging_bytes,
                                           staging_count, host_pinned)
        self._closed = False

    # ---- byte movement ----
    def write(self, off: int, buf, buf_off: int = 0, n: int | None = None) -> None:
        if n is None:
            n = len(buf) - buf_off
        self._n.arena_write(self.handle, off, buf, buf_off, n)

    def read(self, off: int, out, out_off: int = 0, n: int | None = None) -> None:
        if n is None:
            n = len(out) - out_off
        self._n.arena_read(self.handle, off, out, out_off, n)

    def read_bytes(self, off: int, n: int) -> bytes:
        out = bytearray(n)
        self._n.arena_read(self.handle, off, out, 0, n)
        return bytes(out)

    def read_to_ptr(self, off: int, dst_ptr: int, n: int, device: bool) -> None:
        self._n.arena_read_ptr(self.handle, off, dst_ptr, n, device)

    def write_from_ptr(self, off: int, src_ptr: int, n: int, device: bool) -> None:
        self._n.arena_write_ptr(self.handle, off, src_ptr, n, device)

    def copy_to(self, dst: "Arena", dst_off: int, src_off: int, n: int) -> None:
        self._n.arena_copy(dst.handle, dst_off, self.handle, src_off, n)

    def fill(self, off: int, n: int, value: int = 0) -> None:
        self._n.arena_fill(self.handle, off, n, value)

    def crc32c(self, off: int, n: int) -> int:
        return self._n.arena_crc32c(self.handle, off, n)

    def gather(self, extents: list[tuple[int, int]], out, out_off: int = 0) -> None:
        """Pack [(off, len)...] into `out` contiguously (GPU kernel +
        pipelined D2H on device arenas)."""
        self._n.arena_gather(self.handle, extents, out, out_off)

    def gather_ptr(self, triples: list[tuple[int, int, int]],
                   dst_ptr: int) -> None:
        """Scatter-gather [(src_off, dst_off, len)...] into a raw pointer.
        Device arena requires a device dst (on-chip D2D kernel, no host
        hop); host arena requires a host dst (memcpy)."""
        self._n.arena_gather_ptr(self.handle, triples, dst_ptr)

    def convert_ptr(self, segments: list[tuple]) -> None:
        """Typed load: each segment (src_off, dst_ptr, rows, run,
        src_pitch, src_dtype, dst_dtype) moves `rows` runs of `run`
        elements, `src_pitch` bytes apart in the arena, densely to
        `dst_ptr`, converting src_dtype -> dst_dtype (codes from DTYPES).
        Device arena + device destinations = one convert_segments_kernel
        launch for the whole list; host arena + host destinations = the
        same scalar routines in C++.  Bad ranges, unknown codes and
        unsupported pairs raise ValueError before anything runs.

        A 10-tuple appends (scale_ptr, scale_every, scale_e0) and
        dequantises F8_E4M3 -> F32/F16/BF16: dense element e is multiplied
        by the f32 scale at scale_ptr[(scale_e0 + e) // scale_every]
        (scale_every 0: one scale), memory on the destinations' side.

        An 11-tuple appends (scale_ptr, scale_e0, scale_pitch, 32) and
        dequantises an MX tensor, F8_E4M3 or F4 (two per byte, `run` in
        elements) -> F32/F16/BF16: the element in row r, column c is
        multiplied by the E8M0 scale byte at
        scale_ptr[(scale_e0 + r * scale_pitch + c) // 32], one
        mx_load_kernel launch for all of them.

        A 14-tuple appends (scale_ptr, scale_e0, scale_pitch, M, K, bm,
        bn) and dequantises a block-scaled F8_E4M3 tensor (..., M, K) ->
        F32/F16/BF16: the element in row r, column c of the segment is
        element t = scale_e0 + r * scale_pitch + c of the tensor and is
        multiplied by the f32 scale of its bm x bn tile,
        scale_ptr[block_scale_index(t, M, K, bm, bn)], one
        block_load_kernel launch for all of them."""
        plain, mx, block = _split_mx(segments)
        if plain:
            self._n.arena_convert_ptr(self.handle, plain)
        if mx:
            self._n.arena_mx_convert_ptr(self.handle, mx)
        if block:
            self._n.arena_block_convert_ptr(self.handle, block)

    def store_ptr(self, segments: list[tuple]) -> None:
        """Typed store, the scatter direction of convert_ptr: each segment
        (src_ptr, dst_off, rows, run, src_pitch, src_dtype, dst_dtype)
        reads `rows` runs of `run` elements, `src_pitch` bytes apart from
        the absolute address `src_ptr` (a tensor or a row-strided view of
        one, aligned to its itemsize), and writes them densely at arena
        offset `dst_off`, converting src_dtype -> dst_dtype.  Device arena
        + sources on its GPU = one store_segments_kernel launch for the
        whole list; host arena + host sources = the same scalar routines in
        C++.  Bad ranges, alignment, codes and pairs raise ValueError
        before anything runs.  The sources are free to change on return.

        A 10-tuple appends (scale_ptr, scale_every, scale_e0) and quantises
        F32/F16/BF16 -> F8_E4M3: dense element e is divided by the f32
        scale at scale_ptr[(scale_e0 + e) // scale_every] (scale_every 0:
        one scale; see absmax_scales) and cast saturating.  Quantising
        without a scale_ptr is refused.

        An 11-tuple appends (scale_ptr, scale_e0, scale_pitch, 32) and
        quantises F32/F16/BF16 -> F8_E4M3 or F4 under the E8M0 block
        scales of mx_scales, as in convert_ptr: one mx_store_kernel launch
        for all of them.

        A 14-tuple appends (scale_ptr, scale_e0, scale_pitch, M, K, bm,
        bn) and quantises F32/F16/BF16 -> F8_E4M3 under the f32 tile
        scales of block_absmax_scales, as in convert_ptr: one
        block_store_kernel launch for all of them."""
        plain, mx, block = _split_mx(segments)
        if plain:
            self._n.arena_store_ptr(self.handle, plain)
        if mx:
            self._n.arena_mx_store_ptr(self.handle, mx)
        if block:
            self._n.arena_block_store_ptr(self.handle, block)

    def token_windows(self, pieces: list[tuple[int, int, int, int]],
                      x_ptr: int, y_ptr: int, batch: int, seq_len: int,
                      src_dtype: int, dst_dtype: int,
                      vocab_size: int = 0) -> int:
        """Token-window gather: `batch` windows of seq_len + 1 tokens each
        become x = w[:-1] and y = w[1:], two dense [batch, seq_len] arrays
        of dst_dtype at `x_ptr` and `y_ptr`.  Each piece (src_off, row, j0,
        n) holds n >= 1 consecutive src_dtype tokens at arena byte src_off
        (any alignment): tokens j0 .. j0+n-1 of window `row`.  Token j
        lands at x[row, j] when j < seq_len and at y[row, j - 1] when
        j >= 1, widened (see token_windows_supported; codes from DTYPES).
        Device arena + device destinations = one token_windows_kernel
        launch, synchronised on return; host arena + host destinations =
        the same scalar routines in C++.

        With vocab_size > 0 returns how many tokens read lie outside
        [0, vocab_size) (a token two windows share counts twice); they are
        still written.  vocab_size 0 checks nothing and returns 0.  Bad
        pairs, pieces, ranges, alignment and destinations on the wrong
        side raise ValueError before anything runs."""
        return self._n.arena_token_windows(self.handle, pieces, x_ptr, y_ptr,
                                           batch, seq_len, src_dtype,
                                           dst_dtype, vocab_size)

    def array_samples(self, pieces: list[tuple[int, int, int, int]],
                      rows: list[tuple[int, int, int]], out_ptr: int,
                      batch: int, shape: tuple[int, int, int],
                      crop: tuple[int, int], scale, bias, dst_dtype: int,
                      layout: str = "NCHW") -> None:
        """Array-sample gather: `batch` samples of shape = (H, W, C) uint8
        bytes each, HWC order, 1 <= C <= 4, become one dense array of
        dst_dtype (F32 / F16 / BF16, see array_samples_supported; codes from
        DTYPES) at `out_ptr`, [batch, C, h, w] for layout "NCHW" or
        [batch, h, w, C] for "NHWC", with crop = (h, w).  rows[b] = (dy, dx,
        flip) places sample b's crop: output row r, column q, channel c is
        source pixel (dy + r, dx + (w-1-q if flip else q)), as
        f32(f32(v) * scale[c]) + bias[c] rounded to f32, the two steps never
        fused, then cast; scale and bias hold C finite floats, used as
        float32.  Each piece (src_off, row, e0, n) holds n >= 1 source bytes
        at arena byte src_off (any alignment): bytes e0 .. e0+n-1 of sample
        `row`; pieces may cut a sample anywhere.  Every source byte inside
        the crop is converted once; elements whose byte is in no piece are
        not written.  out_ptr is aligned to the itemsize only.  Device
        arena + device destination = one array_samples_kernel launch over
        tiles of ARRAY_TILE bytes, synchronised on return; host arena + host
        destination = the same scalar routines in C++.  Bad dtypes, shapes,
        crops, rows, pieces, ranges, alignment and a destination on the
        wrong side raise ValueError before anything runs."""
        self._n.arena_array_samples(self.handle, pieces, rows, out_ptr, batch,
                                    tuple(shape), tuple(crop),
                                    [float(v) for v in scale],
                                    [float(v) for v in bias], dst_dtype,
                                    array_layout_code(layout))

    def token_eos_index(self, spans: list[tuple[int, int, int]],
                        src_dtype: int, eos_id: int, out_ptr: int = 0,
                        capacity: int = 0) -> int:
        """Where the end-of-document id occurs.  Each span (src_off, tok0,
        n) holds n >= 1 src_dtype tokens (U16 / U32 / I32, codes from
        DTYPES) at arena byte src_off (any alignment): tokens tok0 ..
        tok0+n-1 of a file; spans come in ascending tok0 and do not
        overlap.  The file indices of the tokens equal to eos_id (which is
        non-negative and fits the dtype, so a negative I32 never matches)
        are written to out_ptr as ascending int64, the first `capacity` of
        them; the return value is their total, so capacity 0 (out_ptr may
        be 0) is a pure count.  Device arena + device out_ptr = count,
        offsets and write kernels over tiles of TOKEN_EOS_TILE tokens,
        synchronised on return; host arena + host out_ptr = the same
        comparison in a C++ loop.  Bad arguments raise ValueError
        ("token eos index: ...") before anything runs."""
        return self._n.arena_token_eos_index(self.handle, spans, src_dtype,
                                             eos_id, out_ptr, capacity)

    def token_pack(self, segments: list[tuple], pieces: list[tuple],
                   x_ptr: int, y_ptr: int, pos_ptr: int, doc_ptr: int,
                   cu_ptr: int, rows: int, seq_len: int, src_dtype: int,
                   dst_dtype: int, pad_id: int, ignore_index: int = -100,
                   vocab_size: int = 0) -> int:
        """A document-packed batch [rows, seq_len].  A segment (row, col,
        n, pos0, doc, seq, flags) covers columns col .. col+n-1 of `row`
        with tokens d[0 .. n-1] of one document, plus d[n] when flags is
        TOKEN_SEG_NEXT (the document goes on), or with padding when flags
        is TOKEN_SEG_PAD.  For i in 0 .. n-1 of a source segment:
        x[row, col+i] = d[i] widened (see token_windows_supported),
        y[row, col+i] = d[i+1] when i+1 < n or NEXT, else ignore_index,
        position_ids = pos0 + i, doc_ids = doc; of a pad segment: x =
        pad_id, y = ignore_index, position_ids = i, doc_ids = -1.
        cu_seqlens[seq] = row*seq_len + col for every segment and
        cu_seqlens[len(segments)] = rows*seq_len (int32, rows*seq_len <
        2**31).  The four [rows, seq_len] arrays are dst_dtype; every
        pointer but x_ptr may be 0, which skips that output.

        A piece (src_off, segment, j0, k) holds k >= 1 src_dtype tokens at
        arena byte src_off (any alignment): tokens j0 .. j0+k-1 of source
        segment `segment`'s n (+1) tokens.  Token j lands in x (and its
        position and document id are written) when j < n, and in y one
        column to the left when j >= 1; the piece holding token n-1 of a
        segment without NEXT also writes its ignore_index.  Pad segments
        and cu_seqlens are written by every call, whatever its pieces
        cover.  Device arena + device destinations = one token_pack_kernel
        launch, synchronised on return; host arena + host destinations =
        the same scalar routines in C++.

        With vocab_size > 0 returns how many tokens read lie outside
        [0, vocab_size); they are still written.  Bad arguments raise
        ValueError ("token pack: ...") before anything runs."""
        return self._n.arena_token_pack(self.handle, segments, pieces, x_ptr,
                                        y_ptr, pos_ptr, doc_ptr, cu_ptr, rows,
                                        seq_len, src_dtype, dst_dtype, pad_id,
                                        ignore_index, vocab_size)

    def lz4_compress(self, off: int, n: int) -> bytes:
        """Compress arena bytes [off, off+n) into a CVLZ container (HIP
        kernel on device arenas: only compressed bytes cross D2H; host
        codec on host arenas).  At most 16 MiB per call."""
        return self._n.arena_lz4_compress(self.handle, off, n)

    def lz4_decompress_into(self, off: int, container) -> int:
        """Decompress a CVLZ container into the arena at `off` (HIP kernel
        on device arenas); returns the raw size."""
        return self._n.arena_lz4_decompress(self.handle, off, container)

    def base_ptr(self) -> int:
        return self._n.arena_base_ptr(self.handle)

    def ipc_handle(self) -> bytes:
        """hipIpc export of a device arena (64-byte handle another
        process opens with Arena.from_ipc)."""
        return self._n.arena_ipc_handle(self.handle)

    @classmethod
    def from_ipc(cls, handle: bytes, capacity: int, device: int) -> "Arena":
        """Map another process's device arena (hipIpcOpenMemHandle)."""
        self = cls.__new__(cls)
        self._n = load()
        self.device = device
        self.capacity = capacity
        self.handle = self._n.arena_ipc_open(handle, capacity, device)
        self._closed = False
        return self

    def close(self) -> None:
        if not self._closed:
            self._n.arena_destroy(self.handle)
            self._closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _split_mx(segments):
    """(7- and 10-tuples, 11-tuples, 14-tuples): the MX and the
    block-scaled segments have kernels of their own."""
    plain = [s for s in segments if len(s) not in (11, 14)]
    return plain, [s for s in segments if len(s) == 11], \
        [s for s in segments if len(s) == 14]


def hip_pool_stats() -> dict:
    """Counters of the native pinned-buffer and stream pools and of the
    native ranged pread: pinned_created / pinned_reused (allocations made
    vs. served from the free list), pinned_parked_bytes / _count (idle in
    the pool now), pinned_pool_max_count / _max_bytes / _max_buffer (the
    pool's bounds), streams_created / streams_reused, reader_pread_calls."""
    return dict(load().hip_pool_stats())


class PinnedBuffer:
    """hipHostMalloc'd buffer (plain malloc without a GPU): DMA-fast host
    memory exposed as a writable memoryview.  Used for FUSE request/reply
    buffers so device reads land directly in the bytes handed to writev.

    close() parks the memory in a native pool for the next PinnedBuffer of
    the same size, without a device sync: close only after every read into
    the buffer has returned.  Contents of a new buffer are unspecified."""

    def __init__(self, nbytes: int):
        self._n = load()
        self.nbytes = nbytes
        self.id = self._n.pinned_alloc(nbytes)
        self.view = self._n.pinned_view(self.id)
        self.ptr = self._n.pinned_ptr(self.id)
        self._closed = False

    def close(self) -> None:
        if not self._closed:
            self.view = None
            self._n.pinned_free(self.id)
            self._closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# dtype name (safetensors spelling) -> code understood by convert_ptr
DTYPES = {"F32": 0, "F16": 1, "BF16": 2, "F8_E4M3": 3, "F8_E5M2": 4,
          "F64": 5, "I64": 6, "I32": 7, "I16": 8, "I8": 9, "U8": 10,
          "BOOL": 11, "U16": 12, "U32": 13, "U64": 14,
          # the MX dtypes: known to the mx_* entry points only (code 15 and
          # these stay refused by convert_ptr / store_ptr / convert_host)
          "F8_E8M0": 16, "F4": 17}
DTYPE_ITEMSIZE = {"F32": 4, "F16": 2, "BF16": 2, "F8_E4M3": 1, "F8_E5M2": 1,
                  "F64": 8, "I64": 8, "I32": 4, "I16": 2, "I8": 1, "U8": 1,
                  "BOOL": 1, "U16": 2, "U32": 4, "U64": 8, "F8_E8M0": 1}
# bits per stored element: F4 (E2M1, two per byte) has no itemsize
DTYPE_BITS = {k: 8 * v for k, v in DTYPE_ITEMSIZE.items()}
DTYPE_BITS["F4"] = 4
# floating sources the kernel converts, and the targets it converts to
CONVERT_SOURCES = ("F32", "F16", "BF16", "F8_E4M3", "F8_E5M2")
CONVERT_TARGETS = ("F32", "F16", "BF16")


def convert_supported(src: str, dst: str) -> bool:
    return src == dst or (src in CONVERT_SOURCES and dst in CONVERT_TARGETS)


# the scaled fp8 pairs: F32/F16/BF16 <-> F8_E4M3 with a group scale
QUANTIZE_SOURCES = ("F32", "F16", "BF16")
DEQUANTIZE_TARGETS = ("F32", "F16", "BF16")


def quantize_supported(src: str) -> bool:
    """`src` can be stored as scaled F8_E4M3."""
    return src in QUANTIZE_SOURCES


def dequantize_supported(dst: str) -> bool:
    """Scaled F8_E4M3 can be loaded as `dst`."""
    return dst in DEQUANTIZE_TARGETS


# the MX pairs: F32/F16/BF16 <-> F8_E4M3 (MXFP8) or F4 (MXFP4), blocks of
# 32 elements under one E8M0 scale byte
MX_BLOCK = 32
MX_ELEMENTS = ("F8_E4M3", "F4")


def mx_quantize_supported(src: str, dst: str) -> bool:
    """`src` can be stored as MX elements `dst`."""
    return src in QUANTIZE_SOURCES and dst in MX_ELEMENTS


def mx_dequantize_supported(src: str, dst: str) -> bool:
    """MX elements `src` can be loaded as `dst`."""
    return src in MX_ELEMENTS and dst in DEQUANTIZE_TARGETS


def mx_scales(device: int, segments: list[tuple]) -> None:
    """E8M0 block scales of whole tensors.  Each segment is (src_ptr,
    rows, run, src_pitch, src_dtype, stored_dtype, out_ptr): `rows` runs of
    `run` F32/F16/BF16 elements (`run` a multiple of 32), `src_pitch` bytes
    apart; out_ptr[0 : rows * run // 32] receives one byte per block of 32,
    max(E - emax, 0) with E the biased f32 exponent of the block's largest
    finite |x| and emax 8 for F8_E4M3, 2 for F4.  device >= 0: one
    mx_scales_kernel launch for the whole list, synchronised on return;
    -1: the same routine in C++ over host memory.  Bad arguments raise
    ValueError before anything runs."""
    load().mx_scales(device, segments)


def mx_convert_host(buf, src_dtype: int, dst_dtype: int, n: int, scales,
                    scale_e0: int = 0) -> bytes:
    """Quantise (F32/F16/BF16 -> F8_E4M3 / F4) or dequantise (the reverse)
    `n` packed elements on the host with the kernels' own routines;
    element i uses the E8M0 byte scales[(scale_e0 + i) // 32]."""
    return load().mx_convert_host(buf, src_dtype, dst_dtype, n, scales,
                                  scale_e0)


# the block-scaled pairs: F32/F16/BF16 <-> F8_E4M3 with one f32 scale per
# bm x bn tile of the last two dimensions
BLOCK_DEFAULT = (128, 128)


def block_quantize_supported(src: str) -> bool:
    """`src` can be stored as block-scaled F8_E4M3."""
    return src in QUANTIZE_SOURCES


def block_dequantize_supported(dst: str) -> bool:
    """Block-scaled F8_E4M3 can be loaded as `dst`."""
    return dst in DEQUANTIZE_TARGETS


def block_scale_shape(shape, block) -> tuple:
    """Shape of the f32 scales of a tensor (..., M, K) under bm x bn tiles:
    shape[:-2] + (ceil(M / bm), ceil(K / bn))."""
    bm, bn = block
    return tuple(shape[:-2]) + (-(-shape[-2] // bm), -(-shape[-1] // bn))


def block_absmax_scales(device: int, segments: list[tuple]) -> None:
    """Fill the f32 tile scales for a block-quantising store.  Each
    segment is (src_ptr, rows, run, src_pitch, src_dtype, out_ptr,
    scale_e0, scale_pitch, M, K, bm, bn, n_slots): `rows` runs of `run`
    F32/F16/BF16 elements, `src_pitch` bytes apart at `src_ptr`; the
    element in row r, column c is element t = scale_e0 + r * scale_pitch +
    c of a tensor (..., M, K) and belongs to the tile
    ((t // K // M) * ceil(M/bm) + (t // K % M) // bm) * ceil(K/bn)
    + (t % K) // bn, whose scale is out_ptr[tile].  out_ptr[0:n_slots]
    becomes max(amax, 2**-40) / 448 with amax the largest finite |x| of the
    tile; edge tiles reduce over the elements that exist.  device >= 0: one
    block_absmax_kernel launch for the whole list on that GPU, synchronised
    on return; device == -1: the same routine in C++ over host memory.  Bad
    arguments raise ValueError before anything runs."""
    load().block_absmax_scales(device, segments)


def block_convert_host(buf, src_dtype: int, dst_dtype: int, n: int, scales,
                       scale_e0: int, m: int, k: int, bm: int, bn: int,
                       scale_g0: int = 0) -> bytes:
    """Quantise (F32/F16/BF16 -> F8_E4M3) or dequantise (the reverse) `n`
    packed elements on the host with the kernels' own routines; element i
    is element scale_e0 + i of a tensor (..., m, k) under bm x bn tile
    scales, `scales` holding the tensor's f32 scales from index scale_g0
    on."""
    return load().block_convert_host(buf, src_dtype, dst_dtype, n, scales,
                                     scale_e0, m, k, bm, bn, scale_g0)


# token files: the id dtypes a token window is read from, and the integer
# dtypes it is widened to (U16/U32 zero-extend, I32 sign-extends)
TOKEN_SOURCES = ("U16", "U32", "I32")
TOKEN_TARGETS = ("I32", "I64")


def token_windows_supported(src: str, dst: str) -> bool:
    """Arena.token_windows reads `src` tokens into `dst` tensors.  U32 ->
    I32 would change values and is refused."""
    return src in TOKEN_SOURCES and dst in TOKEN_TARGETS and \
        (src, dst) != ("U32", "I32")


def token_convert_host(buf, src_dtype: int, dst_dtype: int, n: int) -> bytes:
    """Widen `n` packed tokens on the host with the routine the
    token_windows kernel uses: the widened bytes."""
    return load().token_convert_host(buf, src_dtype, dst_dtype, n)


# array samples: uint8 image arrays read as normalised float tensors
ARRAY_TARGETS = ("F32", "F16", "BF16")
ARRAY_LAYOUTS = {"NCHW": 0, "NHWC": 1}


def array_samples_supported(dst: str) -> bool:
    """Arena.array_samples writes `dst` tensors."""
    return dst in ARRAY_TARGETS


def array_layout_code(layout: str) -> int:
    try:
        return ARRAY_LAYOUTS[layout]
    except (KeyError, TypeError):
        raise ValueError(f"array samples: unknown layout {layout!r}") from None


def array_sample_host(buf, dy: int, dx: int, flip: int,
                      shape: tuple[int, int, int], crop: tuple[int, int],
                      scale, bias, dst_dtype: int,
                      layout: str = "NCHW") -> bytes:
    """One whole sample (H*W*C uint8 bytes in `buf`) on the host with the
    routine the array_samples kernel uses: the bytes of its dense C*h*w
    output (arguments as in Arena.array_samples)."""
    return load().array_sample_host(buf, dy, dx, flip, tuple(shape),
                                    tuple(crop), [float(v) for v in scale],
                                    [float(v) for v in bias], dst_dtype,
                                    array_layout_code(layout))


def token_docs(device: int, x_ptr: int, rows: int, seq_len: int, dtype: int,
               eos_id: int, pos_ptr: int = 0, doc_ptr: int = 0,
               cu_ptr: int = 0) -> tuple[int, int]:
    """Document structure of x, a dense [rows, seq_len] array of I32 / I64
    ids at x_ptr, under the end-of-document id `eos_id` (a token equal to it
    ends its document and belongs to it).  For row r, column t:
    doc_ids[r, t] counts the eos in columns < t; position_ids[r, t] is
    t - start with start one past the last eos in columns < t, or 0; flat
    index r * seq_len + t starts a sequence iff t == 0 or x[r, t-1] is eos.
    pos_ptr / doc_ptr receive position_ids / doc_ids in x's dtype; cu_ptr
    (room for rows * seq_len + 1 int32, rows * seq_len < 2**31) receives the
    ascending starts followed by rows * seq_len, n_seqs + 1 entries.  Each of
    the three may be 0: that output is skipped.  Returns (n_seqs,
    max_seqlen), the number of starts and the longest sequence.  device >=
    0: three launches (chunk summaries, offsets, write) on that GPU,
    synchronised on return; device == -1: the same routines in C++ over host
    memory.  Bad arguments raise ValueError before anything runs."""
    return tuple(load().token_docs(device, x_ptr, rows, seq_len, dtype,
                                   eos_id, pos_ptr, doc_ptr, cu_ptr))


# flags of a packed-batch segment (Arena.token_pack)
TOKEN_SEG_NEXT = 1
TOKEN_SEG_PAD = 2


def token_eos_index_host(buf, src_dtype: int, eos_id: int, tok0: int,
                         n: int) -> bytes:
    """Scan `n` packed tokens, tokens tok0 .. tok0+n-1 of a file, on the
    host with the comparison the eos-index kernels use: the file indices of
    the tokens equal to eos_id as packed ascending int64."""
    return load().token_eos_index_host(buf, src_dtype, eos_id, tok0, n)


def token_pack_piece_host(buf, n: int, pos0: int, doc: int, flags: int,
                          j0: int, k: int, src_dtype: int, dst_dtype: int,
                          pad_id: int, ignore_index: int,
                          vocab_size: int = 0) -> tuple:
    """One piece of a packed batch on the host with the pack kernel's own
    routines.  `buf` holds tokens j0 .. j0+k-1 of a source segment (n, pos0,
    doc, flags as in Arena.token_pack); a pad segment is done whole (j0 = 0,
    k = n, buf ignored).  Returns (x, y, pos, doc, bad): dst_dtype bytes of
    x / position_ids / doc_ids for the segment's columns j0 ..
    min(j0+k, n)-1 and of y for its columns from max(j0, 1)-1 on (pad: all
    n), the ignore_index of a document that ends inside the piece included;
    bad counts the tokens outside [0, vocab_size)."""
    return tuple(load().token_pack_piece_host(
        buf, n, pos0, doc, flags, j0, k, src_dtype, dst_dtype, pad_id,
        ignore_index, vocab_size))


def convert_host(buf, src_dtype: int, dst_dtype: int, n: int, scales=None,
                 scale_every: int = 0, scale_e0: int = 0) -> bytes:
    """Convert `n` packed elements on the host with the kernel's own
    scalar routines (bit-identical to the device path).  With `scales` (a
    host buffer of the tensor's f32 group scales) the scaled pairs too:
    element i uses scales[(scale_e0 + i) // scale_every], or scales[0]
    when scale_every is 0."""
    return load().convert_host(buf, src_dtype, dst_dtype, n, scales,
                               scale_every, scale_e0)


def absmax_scales(device: int, segments: list[tuple]) -> None:
    """Fill f32 group scales for a quantising store.  Each segment is
    (src_ptr, rows, run, src_pitch, src_dtype, out_ptr, scale_every,
    scale_e0, n_groups): `rows` runs of `run` F32/F16/BF16 elements,
    `src_pitch` bytes apart at `src_ptr`; dense element e belongs to group
    (scale_e0 + e) // scale_every (0: one group) of its tensor, whose
    scale is out_ptr[group].  out_ptr[0:n_groups] becomes
    max(amax, 2**-40) / 448 with amax the largest finite |x| of the group.
    device >= 0: one absmax_segments_kernel launch for the whole list on
    that GPU, synchronised on return; device == -1: the same routine in
    C++ over host memory.  Bad arguments raise ValueError before anything
    runs."""
    load().absmax_scales(device, segments)


def crc32c(buf, init: int = 0) -> int:
    return load().crc32c(buf, init)


def crc32c_combine(crc1: int, crc2: int, len2: int) -> int:
    return load().crc32c_combine(crc1, crc2, len2)


def lz4_compress(buf) -> bytes:
    return load().lz4_compress(buf)


def lz4_decompress(buf) -> bytes:
    return load().lz4_decompress(buf)
