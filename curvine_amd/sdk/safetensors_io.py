"""Safetensors checkpoints in the cache -> typed torch tensors.

The model-distribution path (BASELINE: "Llama-3-70B shards S3->HBM"):
a `.safetensors` file whose blocks sit in the local worker's HBM arena is
turned into parameters by ONE fused pass per arena — dtype cast
(fp32/fp16/bf16 among each other, fp8 upcasts), tensor-parallel slicing
and the unaligned data section are all handled inside
`convert_segments_kernel` (csrc/tensor_cast.hip), with no temporary and no
host hop.  MEM-tier files loaded onto `cpu` run the same segments through
the same scalar routines in C++; anything else (file tier, cross-side)
takes the slow, correct pread + host-convert path.

`save_file` is the way back: torch tensors -> a safetensors file in the
cache, each block written by one `store_segments_kernel` launch where the
tensors and the arena share a device (see client/typed_writer.py).

FP8 checkpoints (a weight plus a `weight_scale`): `save_file(quantize=
"tensor" | "row")` stores the selected tensors as OCP `F8_E4M3` next to an
F32 `name + "_scale"`.  The scales come from one `absmax_segments_kernel`
launch per device for the whole checkpoint and the store divides by them
as it writes, so the weights are read twice and no full-size temporary
exists.  `load(dequantize=True)` multiplies such a weight by its scale
inside the load kernel.  Both directions are bitwise torch CPU's
`(w.float() / s).clamp(-448, 448).to(float8_e4m3fn)` and
`(q.float() * s).to(dst)`.

MX checkpoints (OCP Microscaling): `save_file(quantize="mxfp8" | "mxfp4")`
stores the selected tensors as `F8_E4M3` or `F4` (E2M1, two per byte) next
to an `F8_E8M0` `name + "_scale"` holding one power-of-two scale byte per
32 elements of the last dimension; `load(dequantize=True)` applies them in
`mx_load_kernel` (csrc/mx_cast.hip).  Scales and elements are defined bit
for bit: s = max(E - emax, 0) from the biased f32 exponent E of the block's
largest finite |x|, q = x * 2**(127-s) rounded once, ties to even,
saturating, y = value(q) * 2**(s-127) rounded once.

Block-scaled FP8 checkpoints (a `weight` plus a `weight_scale_inv`, the
`quant_method: fp8` / `weight_block_size: [128, 128]` layout):
`save_file(quantize="block", quantize_block=(128, 128))` stores the
selected tensors as `F8_E4M3` next to an F32 `name + "_scale_inv"` of shape
shape[:-2] + (ceil(M/bm), ceil(K/bn)), one scale per bm x bn tile of the
last two dimensions; `load(dequantize=True)` multiplies every element by
its tile's scale in `block_load_kernel` (csrc/block_cast.hip).  The
numerics are those of the "row" mode, per tile.

The header parser and writer are written here by hand: the `safetensors`
package is not a dependency.
"""
from __future__ import annotations

import json
import struct
from dataclasses import dataclass

from curvine_amd import errors as err
from curvine_amd.native import (BLOCK_DEFAULT, CONVERT_SOURCES, DTYPE_BITS,
                                DTYPE_ITEMSIZE, DTYPES, MX_BLOCK,
                                block_dequantize_supported,
                                block_quantize_supported, block_scale_shape,
                                convert_supported, dequantize_supported,
                                mx_dequantize_supported,
                                mx_quantize_supported, quantize_supported)

MAX_HEADER = 100 << 20
BLOCK_META_KEY = "weight_block_size"      # __metadata__: "bm,bn"


def _check_block(block, what: str) -> tuple:
    """`block` as two positive ints, else InvalidArgument."""
    try:
        ok = len(block) == 2 and all(
            isinstance(v, int) and not isinstance(v, bool) and v > 0
            for v in block)
    except TypeError:
        ok = False
    if not ok:
        raise err.InvalidArgument(
            f"safetensors: {what} must be two positive ints, not {block!r}")
    return tuple(block)


@dataclass(frozen=True)
class TensorInfo:
    name: str
    dtype: str                       # safetensors spelling, e.g. "BF16"
    shape: tuple
    data_offsets: tuple              # (begin, end) relative to the data section

    @property
    def numel(self) -> int:
        n = 1
        for d in self.shape:
            n *= d
        return n

    @property
    def nbytes(self) -> int:
        return self.data_offsets[1] - self.data_offsets[0]


def parse_header(head8: bytes, read, file_len: int):
    """Parse a safetensors header.  `head8` = first 8 bytes, `read(off, n)`
    fetches header bytes.  Returns (infos: dict name->TensorInfo in file
    order, metadata: dict, data_start: int)."""
    if len(head8) < 8:
        raise err.InvalidArgument("safetensors: file shorter than 8 bytes")
    (n,) = struct.unpack("<Q", head8)
    if n > MAX_HEADER or 8 + n > file_len:
        raise err.InvalidArgument(
            f"safetensors: header length {n} exceeds the file or 100 MiB")
    raw = read(8, n)
    if len(raw) != n:
        raise err.InvalidArgument("safetensors: short header read")

    def pairs(items):
        seen = {}
        for k, v in items:
            if k in seen:
                raise err.InvalidArgument(
                    f"safetensors: duplicate name {k!r}")
            seen[k] = v
        return seen

    try:
        doc = json.loads(bytes(raw).decode("utf-8"), object_pairs_hook=pairs)
    except err.InvalidArgument:
        raise
    except (ValueError, UnicodeDecodeError) as e:
        raise err.InvalidArgument(f"safetensors: bad header JSON: {e}")
    if not isinstance(doc, dict):
        raise err.InvalidArgument("safetensors: header is not a JSON object")
    data_start = 8 + n
    data_len = file_len - data_start
    metadata = {}
    infos: dict[str, TensorInfo] = {}
    for name, ent in doc.items():
        if name == "__metadata__":
            if not isinstance(ent, dict):
                raise err.InvalidArgument(
                    "safetensors: '__metadata__' is not an object")
            metadata = {str(k): str(v) for k, v in ent.items()}
            continue
        if not isinstance(ent, dict):
            raise err.InvalidArgument(
                f"safetensors: entry {name!r} is not an object")
        dt = ent.get("dtype")
        if dt not in DTYPE_BITS:
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: unknown dtype {dt!r}")
        shape = ent.get("shape")
        if not isinstance(shape, list) or any(
                not isinstance(d, int) or isinstance(d, bool) for d in shape):
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: bad shape {shape!r}")
        if any(d < 0 for d in shape):
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: negative dimension")
        offs = ent.get("data_offsets")
        if not isinstance(offs, list) or len(offs) != 2 or any(
                not isinstance(o, int) or isinstance(o, bool) for o in offs):
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: bad data_offsets {offs!r}")
        begin, end = offs
        if begin < 0 or begin > end or end > data_len:
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: data_offsets {offs} out of "
                f"range (data section is {data_len} bytes)")
        numel = 1
        for d in shape:
            numel *= d
        if dt == "F4" and (not shape or shape[-1] % 2):
            # the logical shape, two elements per byte: rows end on a byte
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: F4 shape {shape} has an odd "
                f"last dimension")
        if (end - begin) * 8 != numel * DTYPE_BITS[dt]:
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: {end - begin} bytes for "
                f"shape {shape} of {dt}")
        infos[name] = TensorInfo(name, dt, tuple(shape), (begin, end))
    return infos, metadata, data_start


def read_header(sync_fs, path: str):
    """Header-only parse through the async reader (no short-circuit
    needed): (infos, metadata, data_start, file_len)."""
    async def go():
        r = await sync_fs.fs.open(path)
        try:
            head = await r.pread(0, 8)
            n = struct.unpack("<Q", head)[0] if len(head) == 8 else 0
            body = b""
            if n <= MAX_HEADER and 8 + n <= r.length:
                body = await r.pread(8, n)
            return head, body, r.length
        finally:
            r.close()
    head, body, length = sync_fs.call(go())
    infos, meta, start = parse_header(head, lambda off, n: body, length)
    return infos, meta, start, length


def _torch_dtypes():
    import torch
    m = {"F32": torch.float32, "F16": torch.float16, "BF16": torch.bfloat16,
         "F64": torch.float64, "I64": torch.int64, "I32": torch.int32,
         "I16": torch.int16, "I8": torch.int8, "U8": torch.uint8,
         "BOOL": torch.bool}
    for name, attr in (("F8_E4M3", "float8_e4m3fn"),
                       ("F8_E5M2", "float8_e5m2"),
                       ("F8_E8M0", "float8_e8m0fnu"),
                       ("F4", "float4_e2m1fn_x2"), ("U16", "uint16"),
                       ("U32", "uint32"), ("U64", "uint64")):
        if hasattr(torch, attr):
            m[name] = getattr(torch, attr)
    return m


_FLOATING = CONVERT_SOURCES + ("F64",)
_MX_STORED = ("F8_E4M3", "F4")         # what an E8M0 scale can belong to
_MX_BYTES = ("F8_E8M0", "F4")          # stored dtypes that load as bytes


class CurvineSafetensors:
    """One cached safetensors file.  Holds the file's SyncLocalReader open
    (pinning its blocks) until close()."""

    def __init__(self, sync_fs, path: str):
        self.sync_fs = sync_fs
        self.path = path
        r = sync_fs.call(sync_fs.fs.open(path))
        try:
            self.reader = r.to_sync()
        finally:
            r.close()
        try:
            self._infos, self._meta, self.data_start = parse_header(
                self.reader.pread(0, 8), self.reader.pread,
                self.reader.length)
        except Exception:
            self.reader.close()
            raise
        self._t2s = None

    # ---- header views ----
    def keys(self) -> list[str]:
        return list(self._infos)

    def metadata(self) -> dict[str, str]:
        return dict(self._meta)

    def info(self, name: str) -> TensorInfo:
        try:
            return self._infos[name]
        except KeyError:
            raise err.InvalidArgument(f"safetensors: no tensor {name!r}")

    # ---- planning ----
    def _dst_dtype_name(self, info: TensorInfo, dtype) -> str:
        """Stored dtype unless `dtype` is given and the tensor is floating
        (integer/bool tensors keep theirs, as module.to(dtype) does)."""
        if dtype is None or info.dtype not in _FLOATING:
            return info.dtype
        if self._t2s is None:
            self._t2s = {v: k for k, v in _torch_dtypes().items()}
        dst = self._t2s.get(dtype)
        if dst is None or not convert_supported(info.dtype, dst):
            raise err.Unsupported(
                f"safetensors: tensor {info.name!r}: cannot load {info.dtype}"
                f" as {dtype}")
        return dst

    @staticmethod
    def _slice(info: TensorInfo, shard):
        """(out_shape, rows, run, src_pitch_elems, first_elem) of the
        tensor or of its equal shard (dim, rank, world)."""
        shape = info.shape
        if shard is None:
            return shape, 1, info.numel, info.numel, 0
        dim, rank, world = shard
        nd = len(shape)
        if not -nd <= dim < nd:
            raise err.InvalidArgument(
                f"safetensors: tensor {info.name!r}: shard dim {dim} out of "
                f"range for shape {shape}")
        dim %= nd
        if world <= 0 or not 0 <= rank < world:
            raise err.InvalidArgument(
                f"safetensors: tensor {info.name!r}: bad shard rank/world "
                f"{rank}/{world}")
        if shape[dim] % world:
            raise err.InvalidArgument(
                f"safetensors: tensor {info.name!r}: dimension {dim} of size "
                f"{shape[dim]} is not divisible by world {world}")
        outer = inner = 1
        for d in shape[:dim]:
            outer *= d
        for d in shape[dim + 1:]:
            inner *= d
        part = shape[dim] // world
        out_shape = shape[:dim] + (part,) + shape[dim + 1:]
        return (out_shape, outer, part * inner, shape[dim] * inner,
                rank * part * inner)

    def _block_of(self, scale_block) -> tuple:
        """(bm, bn) of this file's block-scaled tensors: the keyword, else
        `__metadata__["weight_block_size"]` ("bm,bn"; a value that does
        not read as two positive ints counts as absent), else (128, 128)."""
        if scale_block is not None:
            return _check_block(scale_block, "scale_block")
        try:
            bm, bn = (int(v) for v in
                      self._meta.get(BLOCK_META_KEY, "").strip("[]() ")
                      .split(","))
            return _check_block((bm, bn), BLOCK_META_KEY)
        except (ValueError, err.InvalidArgument):
            return BLOCK_DEFAULT

    def _scale_info(self, info: TensorInfo, block=BLOCK_DEFAULT):
        """The F32 `name + "_scale"` entry that makes a stored F8_E4M3
        tensor a scaled one (one scale, or one per index of dim 0), or
        the F8_E8M0 one of shape shape[:-1] + (K // 32,) that makes a
        stored F8_E4M3 or F4 tensor an MX one; failing both, the F32
        `name + "_scale_inv"` of shape shape[:-2] + (ceil(M/bm),
        ceil(K/bn)) that makes a stored F8_E4M3 tensor (..., M, K) a
        block-scaled one; else None."""
        s = self._plain_scale_info(info)
        if s is not None or info.dtype != "F8_E4M3" or len(info.shape) < 2:
            return s
        s = self._infos.get(info.name + "_scale_inv")
        if s is not None and s.dtype == "F32" and \
                s.shape == block_scale_shape(info.shape, block):
            return s
        return None

    @staticmethod
    def _is_block(info: TensorInfo, sinfo: TensorInfo) -> bool:
        return sinfo.name == info.name + "_scale_inv"

    def _plain_scale_info(self, info: TensorInfo):
        if info.dtype not in _MX_STORED:
            return None
        s = self._infos.get(info.name + "_scale")
        if s is None:
            return None
        if s.dtype == "F8_E8M0":
            if info.shape and info.shape[-1] % MX_BLOCK == 0 and s.shape == \
                    info.shape[:-1] + (info.shape[-1] // MX_BLOCK,):
                return s
            return None
        if info.dtype != "F8_E4M3" or s.dtype != "F32":
            return None
        if s.numel == 1 or (info.shape and s.numel == info.shape[0]):
            return s
        return None

    def _scale_fields(self, info: TensorInfo, sinfo: TensorInfo, shard,
                      out_shape, scale_ptr: int, block=BLOCK_DEFAULT):
        """(scale_ptr, scale_every, scale_e0) of a request for `info` or
        its shard, the tensor's scales being at scale_ptr.  For an MX
        tensor (scale_ptr, scale_e0, scale_pitch, 32): the request's first
        element and the distance of its runs, both in elements of the
        tensor and multiples of 32, so a run's block scales start at byte
        scale_e0 // 32 and lie scale_pitch // 32 bytes apart.  For a
        block-scaled tensor (scale_ptr, scale_e0, scale_pitch, M, K, bm,
        bn): the same two tensor indices, any shard, the whole scale
        tensor."""
        if self._is_block(info, sinfo):
            _, rows, run, pitch_el, first = self._slice(info, shard)
            return (scale_ptr, first, pitch_el) + info.shape[-2:] + \
                tuple(block)
        if sinfo.dtype == "F8_E8M0":
            _, rows, run, pitch_el, first = self._slice(info, shard)
            if run % MX_BLOCK:
                raise err.Unsupported(
                    f"safetensors: tensor {info.name!r}: shard "
                    f"{tuple(shard)} cuts the MX blocks of 32")
            return (scale_ptr, first, pitch_el, MX_BLOCK)
        if sinfo.numel == 1:
            return (scale_ptr, 0, 0)          # ignores the shard
        every = 1
        for d in out_shape[1:]:
            every *= d
        if shard is not None and shard[0] % len(info.shape) == 0:
            scale_ptr += 4 * shard[1] * out_shape[0]   # dim-0 shard's rows
        return (scale_ptr, every, 0)

    def _request(self, info: TensorInfo, dst_name: str, shard, dst_ptr: int):
        _, rows, run, pitch_el, first = self._slice(info, shard)
        bits = DTYPE_BITS[info.dtype]
        off = self.data_start + info.data_offsets[0] + first * bits // 8
        if rows > 1 and run == pitch_el:      # dim-0-like: one run
            rows, run = 1, rows * run
        return (off, rows, run, pitch_el * bits // 8, info.dtype, dst_name,
                dst_ptr)

    @staticmethod
    def _byte_view(info: TensorInfo, shard) -> TensorInfo:
        """A stored F8_E8M0 or F4 tensor as the U8 tensor of its bytes (F4:
        the last dimension halved, as torch.float4_e2m1fn_x2 has it): they
        load without a kernel of their own."""
        shape = info.shape
        if info.dtype == "F4":
            if shard is not None and shape and \
                    shard[0] % len(shape) == len(shape) - 1 and \
                    shard[2] > 0 and shape[-1] % shard[2] == 0 and \
                    (shape[-1] // shard[2]) % 2:
                raise err.Unsupported(
                    f"safetensors: tensor {info.name!r}: shard "
                    f"{tuple(shard)} splits a byte of F4")
            shape = shape[:-1] + (shape[-1] // 2,)
        return TensorInfo(info.name, "U8", shape, info.data_offsets)

    def _execute(self, requests, dev) -> None:
        on_dev = dev.type != "cpu"
        groups, slow = self.reader.resolve_convert(requests, on_dev)
        if on_dev:
            import torch
            # the kernel runs on the arena's own stream; the caching
            # allocator may hand out memory torch's stream still uses
            torch.cuda.current_stream(dev).synchronize()
        self.reader.exec_convert(groups, slow, on_dev)

    # ---- loading ----
    def load(self, device="cuda:0", dtype=None, names=None,
             shard_plan=None, dequantize: bool = False,
             scale_block=None) -> dict:
        """All (or `names`) tensors in one batched pass: every destination
        is allocated, every tensor resolved, then ONE convert call per
        arena covers the whole file.

        `dequantize=True`: a stored F8_E4M3 tensor N whose file also holds
        an F32 `N + "_scale"` with one element or one per index of dim 0
        comes back multiplied by it, as `dtype` (F32 when None), and the
        `_scale` entry is left out of the result unless `names` asks for
        it.  The same holds for an MX tensor: stored F8_E4M3 or F4 with an
        F8_E8M0 `N + "_scale"` of shape shape[:-1] + (K // 32,); a shard of
        it along the last dimension needs a part that is a multiple of 32
        (Unsupported otherwise).  Without `dequantize`, F8_E8M0 loads as
        torch.float8_e8m0fnu and F4 as torch.float4_e2m1fn_x2 with the
        last dimension halved.  That takes two batched passes: the scales go to F32 tensors
        on `device` first, then everything else with the weights pointing
        at them.  An F8_E4M3 tensor without such a scale loads as ever.

        Block-scaled tensors (`quant_method: fp8` with `weight_block_size`
        in Hugging Face terms): a stored F8_E4M3 tensor N of shape
        (..., M, K) without such a `_scale` whose file holds an F32
        `N + "_scale_inv"` of shape shape[:-2] + (ceil(M/bm), ceil(K/bn))
        comes back as `(q.float() * s_tile).to(dst)`, one scale per
        bm x bn tile of each matrix, applied in block_load_kernel
        (csrc/block_cast.hip); the `_scale_inv` entry is hidden like a
        `_scale`.  (bm, bn) is `scale_block`, or when None the file's
        `__metadata__["weight_block_size"]` ("bm,bn"), or (128, 128);
        anything but two positive ints is InvalidArgument.  A `_scale_inv`
        of another shape leaves the tensor unscaled.  Shards along any
        dimension and of any part size work, parts that cut tiles
        included: every element looks its scale up by its own
        coordinates, so the result is the slice of the whole dequantised
        tensor."""
        import torch
        dev = torch.device(device)
        tmap = _torch_dtypes()
        shard_plan = shard_plan or {}
        wanted = self.keys() if names is None else list(names)
        scaled = {}
        block = self._block_of(scale_block)
        if dequantize:
            for name in wanted:
                sinfo = self._scale_info(self.info(name), block)
                if sinfo is not None:
                    scaled[name] = sinfo
            if names is None:
                hidden = {s.name for s in scaled.values()}
                wanted = [n for n in wanted if n not in hidden]
        out, requests = {}, []
        for name in wanted:
            info = self.info(name)
            if name in scaled:
                dst_name = self._dequant_dtype_name(info, dtype)
            else:
                dst_name = self._dst_dtype_name(info, dtype)
            if dst_name not in tmap:
                raise err.Unsupported(
                    f"safetensors: tensor {name!r}: this torch has no {dst_name}")
            shard = shard_plan.get(name)
            if name not in scaled and info.dtype in _MX_BYTES:
                info, dst_name, dt = self._byte_view(info, shard), "U8", \
                    tmap[dst_name]
            else:
                dt = tmap[dst_name]
            shape = self._slice(info, shard)[0]
            t = torch.empty(shape, dtype=dt, device=dev)
            out[name] = t
            if t.numel():
                requests.append((name, shard, shape, self._request(
                    info, dst_name, shard, t.data_ptr())))
        scales = self._load_scales(scaled.values(), dev)
        self._execute(
            [req if name not in scaled else req + self._scale_fields(
                self.info(name), scaled[name], shard, shape,
                scales[scaled[name].name].data_ptr(), block)
             for name, shard, shape, req in requests], dev)
        return out

    def _dequant_dtype_name(self, info: TensorInfo, dtype) -> str:
        if dtype is None:
            return "F32"
        if self._t2s is None:
            self._t2s = {v: k for k, v in _torch_dtypes().items()}
        dst = self._t2s.get(dtype)
        if dst is None or not (dequantize_supported(dst) and
                               mx_dequantize_supported(info.dtype, dst)):
            raise err.Unsupported(
                f"safetensors: tensor {info.name!r}: cannot dequantize to "
                f"{dtype}")
        return dst

    def _load_scales(self, sinfos, dev) -> dict:
        """{scale name: F32 (or, for E8M0 bytes, U8) tensor on dev}, one
        batched pass."""
        import torch
        out, requests = {}, []
        for s in sinfos:
            if s.name in out:
                continue
            if s.dtype == "F8_E8M0":
                t = torch.empty(s.shape, dtype=torch.uint8, device=dev)
                req = self._request(self._byte_view(s, None), "U8", None,
                                    t.data_ptr())
            else:
                t = torch.empty(s.shape, dtype=torch.float32, device=dev)
                req = self._request(s, "F32", None, t.data_ptr())
            out[s.name] = t
            if t.numel():
                requests.append(req)
        if requests:
            self._execute(requests, dev)
        return out

    def get_tensor(self, name: str, device="cuda:0", dtype=None, shard=None,
                   dequantize: bool = False, scale_block=None):
        plan = None if shard is None else {name: shard}
        return self.load(device, dtype, [name], plan, dequantize,
                         scale_block)[name]

    def load_into(self, name: str, tensor, shard=None,
                  dequantize: bool = False, scale_block=None) -> None:
        """Fill an existing tensor (a module parameter): destination dtype
        and device come from `tensor`.  `dequantize` and `scale_block` as
        in load()."""
        info = self.info(name)
        block = self._block_of(scale_block)
        sinfo = self._scale_info(info, block) if dequantize else None
        stored = info.dtype
        if sinfo is None and stored in _MX_BYTES:
            info = self._byte_view(info, shard)
        shape = self._slice(info, shard)[0]
        if tuple(tensor.shape) != tuple(shape):
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: destination shape "
                f"{tuple(tensor.shape)} != {tuple(shape)}")
        if not tensor.is_contiguous():
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: destination is not contiguous")
        if tensor.device.type not in ("cpu", "cuda"):
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: unsupported destination "
                f"device {tensor.device}")
        t2s = {v: k for k, v in _torch_dtypes().items()}
        dst_name = t2s.get(tensor.dtype)
        if dst_name is None or not (
                (block_dequantize_supported(dst_name)
                 if self._is_block(info, sinfo)
                 else dequantize_supported(dst_name)) if sinfo is not None
                else convert_supported(stored, dst_name)):
            raise err.Unsupported(
                f"safetensors: tensor {name!r}: cannot load {stored} "
                f"into {tensor.dtype}")
        if tensor.numel():
            req = self._request(info, dst_name if info.dtype == stored
                                else "U8", shard, tensor.data_ptr())
            if sinfo is not None:
                scales = self._load_scales([sinfo], tensor.device)
                req += self._scale_fields(info, sinfo, shard, shape,
                                          scales[sinfo.name].data_ptr(),
                                          block)
            self._execute([req], tensor.device)

    def close(self) -> None:
        self.reader.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def load_file(sync_fs, path: str, device="cuda:0", dtype=None,
              dequantize: bool = False, scale_block=None) -> dict:
    """One-shot: cached safetensors path -> {name: tensor}."""
    with CurvineSafetensors(sync_fs, path) as f:
        return f.load(device=device, dtype=dtype, dequantize=dequantize,
                      scale_block=scale_block)


# ---------------------------------------------------------------- saving

def _rows_of_runs(t):
    """(rows, run, pitch in elements) when `t`, read in logical order, is
    rows of contiguous runs — contiguous, or at most one stride break after
    collapsing contiguous dimensions (`w[:, a:b]`, `w[a:b]`) — else None."""
    dims = [(n, st) for n, st in zip(t.shape, t.stride()) if n != 1]
    merged = []
    for n, st in dims:
        if merged and merged[-1][1] == st * n:
            merged[-1] = (merged[-1][0] * n, st)
        else:
            merged.append((n, st))
    if not merged:
        return 1, 1, 1
    if len(merged) == 1:
        n, st = merged[0]
        if st == 1:
            return 1, n, n
        return (n, 1, st) if st > 1 else None
    if len(merged) == 2:
        (rows, pitch), (run, st) = merged
        if st == 1 and pitch >= run:
            return rows, run, pitch
    return None


def _host_reader(t, rows: int, run: int, pitch: int):
    """read_host of a TypedSource: dense elements [e0, e1) of `t` as host
    bytes in the source dtype (only the rows that hold them are copied)."""
    import torch
    v = t.as_strided((rows, run), (pitch, 1))

    def read_host(e0: int, e1: int):
        r0, r1 = e0 // run, (e1 - 1) // run
        part = v[r0:r1 + 1].reshape(-1)[e0 - r0 * run:e1 - r0 * run]
        return part.cpu().contiguous().view(torch.uint8).numpy()
    return read_host


QUANTIZE_MODES = ("tensor", "row", "mxfp8", "mxfp4", "block")
MX_MODES = {"mxfp8": "F8_E4M3", "mxfp4": "F4"}     # mode -> element dtype


def _quantize_default(name, t) -> bool:
    return t.is_floating_point() and t.element_size() in (2, 4) and \
        t.ndim >= 2 and t.numel() > 0


def _numel(shape) -> int:
    n = 1
    for d in shape:
        n *= d
    return n


def _scales_host(scale):
    """scales_host of a TypedSource: the f32 scales (or E8M0 bytes) on
    the host, fetched once."""
    cache = []

    def scales_host():
        if not cache:
            cache.append(scale.reshape(-1).cpu().numpy())
        return cache[0]
    return scales_host


def _save_plan(tensors: dict, metadata, dtype, quantize=None,
               quantize_filter=None, quantize_block=None):
    """(header bytes, [TypedSource], tensors kept alive).  Raises before
    anything touches the cluster."""
    import torch

    from curvine_amd import native

    from curvine_amd.client.typed_writer import TypedSource
    if not isinstance(tensors, dict):
        raise err.InvalidArgument("safetensors: tensors must be a dict")
    if metadata is not None and (not isinstance(metadata, dict) or any(
            not isinstance(k, str) or not isinstance(v, str)
            for k, v in metadata.items())):
        raise err.InvalidArgument("safetensors: metadata must map str to str")
    if quantize is not None and quantize not in QUANTIZE_MODES:
        raise err.InvalidArgument(
            f"safetensors: quantize must be one of {QUANTIZE_MODES}, not "
            f"{quantize!r}")
    mx = MX_MODES.get(quantize)
    block = None
    if quantize == "block":
        # the tile geometry is part of the format a file is written in:
        # it is named by the caller, never assumed
        if quantize_block is None:
            raise err.InvalidArgument(
                'safetensors: quantize="block" needs quantize_block=(bm, '
                'bn), e.g. (128, 128)')
        block = _check_block(quantize_block, "quantize_block")
        want = f"{block[0]},{block[1]}"
        if metadata is not None and \
                metadata.get(BLOCK_META_KEY, want) != want:
            raise err.InvalidArgument(
                f"safetensors: metadata {BLOCK_META_KEY!r} is "
                f"{metadata[BLOCK_META_KEY]!r} but quantize_block gives "
                f"{want!r}")
        metadata = dict(metadata or {})
        metadata[BLOCK_META_KEY] = want
    elif quantize_block is not None:
        raise err.InvalidArgument(
            'safetensors: quantize_block needs quantize="block"')
    suffix = "_scale_inv" if block else "_scale"
    forced = quantize_filter is not None
    if quantize_filter is None:
        quantize_filter = _quantize_default
    t2s = {v: k for k, v in _torch_dtypes().items()}
    entries = []
    n_groups: dict[int, int] = {}        # device -> scale slots needed
    for name, t in tensors.items():
        if not isinstance(name, str) or name == "__metadata__":
            raise err.InvalidArgument(f"safetensors: bad tensor name {name!r}")
        if not isinstance(t, torch.Tensor):
            raise err.InvalidArgument(
                f"safetensors: value of {name!r} is not a tensor")
        if t.layout != torch.strided:
            raise err.Unsupported(
                f"safetensors: tensor {name!r}: layout {t.layout}")
        src = t2s.get(t.dtype)
        if src is None:
            raise err.Unsupported(
                f"safetensors: tensor {name!r}: cannot store {t.dtype}")
        dst = src
        shape = tuple(t.shape)
        if src == "F4":                  # two elements per stored byte
            if not shape:
                raise err.InvalidArgument(
                    f"safetensors: tensor {name!r}: F4 without a dimension")
            shape = shape[:-1] + (2 * shape[-1],)
        whole = t.ndim >= 1 and t.shape[-1] % MX_BLOCK == 0
        if quantize is not None and quantize_filter(name, t) and (
                mx is None or forced or whole):
            if not quantize_supported(src):
                raise err.Unsupported(
                    f"safetensors: tensor {name!r}: cannot quantize {src}")
            if quantize == "row" and t.ndim == 0:
                raise err.InvalidArgument(
                    f"safetensors: tensor {name!r}: no dim 0 to scale by")
            if mx is not None and not whole:
                raise err.InvalidArgument(
                    f"safetensors: tensor {name!r}: last dimension of shape "
                    f"{shape} is not a multiple of {MX_BLOCK}")
            if block and t.ndim < 2:
                raise err.InvalidArgument(
                    f"safetensors: tensor {name!r}: shape {shape} has no "
                    f"two dimensions to tile")
            if name + suffix in tensors:
                raise err.InvalidArgument(
                    f"safetensors: {name + suffix!r} is both a given "
                    f"tensor and the scale of {name!r}")
            if block and name + "_scale" in tensors:
                raise err.InvalidArgument(
                    f"safetensors: the given tensor {name + '_scale'!r} "
                    f"would win over {name + suffix!r} when {name!r} is "
                    f"loaded")
            dst = mx or "F8_E4M3"
        elif dtype is not None and src in _FLOATING:
            dst = t2s.get(dtype)
            if dst is None or not convert_supported(src, dst):
                raise err.Unsupported(
                    f"safetensors: tensor {name!r}: cannot save {src} as "
                    f"{dtype}")
        if t.device.type == "cpu":
            device = -1
        elif t.device.type == "cuda":
            device = t.device.index
        else:
            raise err.InvalidArgument(
                f"safetensors: tensor {name!r}: unsupported device {t.device}")
        entries.append((name, t, src, dst, device, shape))
        if dst != src and dst in _MX_STORED:
            n_groups[device] = n_groups.get(device, 0) + (
                t.numel() // MX_BLOCK if mx else
                _numel(block_scale_shape(shape, block)) if block else
                t.shape[0] if quantize == "row" else 1)

    # one buffer per device holds every scale of the checkpoint (F32, or
    # E8M0 bytes for the MX modes): each `name + "_scale"` (block mode:
    # `name + "_scale_inv"`) is a view of it, saved like any given tensor
    scale_of, used = {}, {}
    sdt = "F8_E8M0" if mx else "F32"
    bufs = {d: torch.empty(n, dtype=torch.uint8 if mx else torch.float32,
                           device="cpu" if d < 0 else f"cuda:{d}")
            for d, n in n_groups.items()}
    for name, t, src, dst, device, shape in list(entries):
        if dst == src or dst not in _MX_STORED:
            continue
        if mx:
            n, view = t.numel() // MX_BLOCK, \
                shape[:-1] + (shape[-1] // MX_BLOCK,)
        elif block:
            view = block_scale_shape(shape, block)
            n = _numel(view)
        else:
            n = t.shape[0] if quantize == "row" else 1
            view = (n, 1) if quantize == "row" else (1,)
        o = used.get(device, 0)
        used[device] = o + n
        scale = bufs[device][o:o + n].view(view)
        scale_of[name] = scale
        entries.append((name + suffix, scale, sdt, sdt, device, view))
    entries.sort(key=lambda e: (-DTYPE_BITS[e[3]], e[0]))

    hdr, keep, sources, pos = {}, list(bufs.values()), [], 0
    absmax: dict[int, list] = {}
    if metadata is not None:
        hdr["__metadata__"] = dict(metadata)
    for name, t, src, dst, device, shape in entries:
        numel = 1
        for d in shape:
            numel *= d
        nbytes = numel * DTYPE_BITS[dst] // 8
        hdr[name] = {"dtype": dst, "shape": list(shape),
                     "data_offsets": [pos, pos + nbytes]}
        scale = scale_of.get(name) if dst != src else None
        if src in _MX_BYTES:                 # E8M0 / F4 travel as bytes
            src = dst = "U8"
        if t.numel():
            lay = _rows_of_runs(t)
            if lay is None or (mx and scale is not None and lay[0] > 1
                               and lay[1] % MX_BLOCK):
                t = t.contiguous()           # allocates a temporary
                lay = (1, t.numel(), t.numel())
            rows, run, pitch = lay
            keep.append(t)
            source = TypedSource(
                pos, t.data_ptr(), rows, run, pitch * DTYPE_ITEMSIZE[src],
                src, dst, device, _host_reader(t, rows, run, pitch))
            if scale is not None and mx:
                source.mx = True
                source.scale_ptr = scale.data_ptr()
                source.scales_host = _scales_host(scale)
                absmax.setdefault(device, []).append(
                    (t.data_ptr(), rows, run, source.pitch, DTYPES[src],
                     DTYPES[dst], scale.data_ptr()))
            elif scale is not None and block:
                # the dense side is the tensor: tiles follow its last two
                # dimensions whatever the layout collapsed to
                source.block = tuple(shape[-2:]) + block
                source.scale_ptr = scale.data_ptr()
                source.scales_host = _scales_host(scale)
                absmax.setdefault(device, []).append(
                    (t.data_ptr(), rows, run, source.pitch, DTYPES[src],
                     scale.data_ptr(), 0, run) + source.block +
                    (scale.numel(),))
            elif scale is not None:
                # groups follow the tensor's dim 0 whatever the layout
                # collapsed to
                every = t.numel() // t.shape[0] if quantize == "row" else 0
                source.scale_ptr = scale.data_ptr()
                source.scale_every = every
                source.scales_host = _scales_host(scale)
                absmax.setdefault(device, []).append(
                    (t.data_ptr(), rows, run, source.pitch, DTYPES[src],
                     scale.data_ptr(), every, 0, scale.numel()))
            sources.append(source)
        pos += nbytes
    for device, buf in bufs.items():
        if not buf.numel():
            continue
        if device >= 0:
            # absmax runs on a stream of its own: what torch's stream
            # still has in flight for these tensors must be done
            torch.cuda.current_stream(device).synchronize()
        segs = absmax.get(device, [])
        if not segs and not mx and not block:   # only empty weights: floor
            segs = [(0, 0, 0, 0, DTYPES["F32"], buf.data_ptr(), 0, 0,
                     buf.numel())]
        try:
            if mx:
                native.mx_scales(device, segs)
            elif block:
                native.block_absmax_scales(device, segs)
            else:
                native.absmax_scales(device, segs)
        except ValueError as e:
            raise err.InvalidArgument(str(e))
    js = json.dumps(hdr, separators=(",", ":")).encode()
    js += b" " * (-(8 + len(js)) % 64)
    header = struct.pack("<Q", len(js)) + js
    for s in sources:
        s.file_off += len(header)
    return header, sources, keep


def save_file(sync_fs, tensors: dict, path: str, metadata=None, dtype=None,
              storage_tier: str = "", block_size: int = 0,
              overwrite: bool = False, replicas: int = 0, quantize=None,
              quantize_filter=None, quantize_block=None):
    """Save {name: tensor} as a safetensors file in the cache; returns its
    FileStatus.  Blocks that land in the HBM arena of the tensors' own GPU
    (or in a host arena, for cpu tensors) are written by the typed store:
    one store_segments_kernel launch per block converts and copies the
    tensors where they are.  Every other block (file tier, remote worker,
    replicas > 1, another GPU) is built on the host with the same scalar
    routines, so the file is bit-identical either way.  cpu and cuda
    tensors may be mixed.

    File layout: tensors ordered by descending itemsize of the stored
    dtype, then by name; a contiguous data section; a compact JSON header
    (`__metadata__` first when given) right-padded with spaces so the data
    section starts on a multiple of 64.

    `dtype` casts floating tensors where `convert_supported` allows it
    (integer and bool tensors keep theirs); anything else raises
    Unsupported.  A tensor is read in place when it is contiguous or rows
    of contiguous runs (`w[:, a:b]`, `w[a:b]`); any other view is made
    contiguous first, which allocates a temporary of its size.  Tensors
    sharing storage are written independently.  `block_size` must be a
    multiple of 8.

    `quantize` stores the selected tensors as scaled `F8_E4M3` (OCP E4M3)
    with their own shape, each next to an F32 `name + "_scale"`:
    "tensor" gives one scale of shape [1], "row" one per index of dim 0,
    shape [shape[0], 1].  scale = max(amax, 2**-40) / 448 with amax the
    largest finite |x| of the group, q = saturate(x / scale), both
    bitwise torch CPU's.  Selected are the F32/F16/BF16 tensors with
    ndim >= 2 and numel > 0, or those `quantize_filter(name, tensor)`
    accepts; everything else is saved as without `quantize`.

    `quantize="mxfp8" | "mxfp4"` stores them as OCP Microscaling tensors
    instead: `F8_E4M3` or `F4` (E2M1, two per byte, even element in the
    low nibble) with their own shape, next to an `F8_E8M0`
    `name + "_scale"` of shape shape[:-1] + (K // 32,), one power-of-two
    scale byte per 32 elements of the last dimension.  s = max(E - emax,
    0) with E the biased f32 exponent of the block's largest finite |x|
    and emax 8 or 2; q = x * 2**(127-s) rounded once, ties to even,
    saturating.  The default selection adds `shape[-1] % 32 == 0`; a
    tensor `quantize_filter` selects whose last dimension is no multiple
    of 32 is InvalidArgument.  The scales come from one mx_scales_kernel
    launch per device.  `F4` sorts after the one-byte dtypes in the file.
    Tensors that already are torch.float8_e8m0fnu or
    torch.float4_e2m1fn_x2 are saved as `F8_E8M0` / `F4` (the last
    dimension doubled), so a loaded MX checkpoint saves back byte for
    byte.  Refused
    before anything touches the cluster: an unknown mode or a
    `name + "_scale"` that is also a given tensor (InvalidArgument), a
    selected tensor that is not F32/F16/BF16 (Unsupported).  The scales
    are computed on the tensors' device, one absmax_segments_kernel launch
    per device for the whole checkpoint, and views are quantised in
    place.

    `quantize="block"` stores them as block-scaled `F8_E4M3` (the layout
    of `quant_method: fp8` checkpoints with `weight_block_size`): each
    next to an F32 `name + "_scale_inv"` of shape shape[:-2] +
    (ceil(M/bm), ceil(K/bn)), one scale per bm x bn tile of the last two
    dimensions (leading dimensions are batches of matrices), w = q *
    scale_inv.  (bm, bn) is `quantize_block`, which the mode requires:
    the geometry of a written file is named, never assumed, so
    `quantize="block"` alone is InvalidArgument; (128, 128) is what the
    checkpoints that ship this layout use and what load() assumes.  The
    scale and the cast are those of "row" applied per tile, edge tiles
    reducing over the elements that exist.  `weight_block_size: "bm,bn"`
    is added to `__metadata__` (created when none was given).  The default
    selection is that of "row".  Also refused before anything touches the
    cluster (InvalidArgument): a `quantize_block` that is not two positive
    ints or comes with another mode, a caller's own `weight_block_size`
    that differs, a `name + "_scale_inv"` that is also a given tensor (or
    a `name + "_scale"`, which would win over it on load), a
    selected tensor with fewer than two dimensions.  The scales come from
    one block_absmax_kernel launch per device (csrc/block_cast.hip)."""
    header, sources, keep = _save_plan(tensors, metadata, dtype, quantize,
                                       quantize_filter, quantize_block)
    devices = sorted({s.device for s in sources if s.device >= 0})
    if devices:
        import torch
        for d in devices:
            # the store runs on the arena's own stream: what torch's
            # stream still has in flight for these tensors must be done
            torch.cuda.current_stream(d).synchronize()
    st = sync_fs.call(sync_fs.fs.write_typed(
        path, header, sources, overwrite=overwrite, replicas=replicas,
        block_size=block_size, storage_tier=storage_tier))
    del keep
    return st
