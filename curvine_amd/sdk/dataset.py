"""PyTorch DataLoader integration: datasets over cached files.

The training-data path (BASELINE config[4]): WebDataset-style tar shards
cached in HBM/host tiers, consumed by a torch DataLoader.  Two entries:

* `CurvineShardDataset` — iterable dataset over tar shards stored in the
  cache (reads through the client short-circuit; optionally lands sample
  bytes straight into device tensors).
* `CurvineFileDataset` — map-style dataset of whole files.

Two batched loaders that bypass the DataLoader for files living in the
HBM tier:

* `CurvineDeviceLoader` — raw tar payloads gathered into one uint8 device
  tensor per batch.
* `CurvineTokenLoader` — flat token-id files (uint16 / uint32 / int32):
  windows of seq_len + 1 ids become the (x, y) tensors of a language-model
  step in one kernel launch per batch, with a vocabulary check; on request
  also position ids, document ids and cu_seqlens under an end-of-document
  id (native.token_docs).
* `CurvinePackedTokenLoader` — the same files as whole documents packed
  into rows (`pack_segments`): x, targets masked at document ends, position
  ids, document ids and cu_seqlens from one kernel launch per batch.

* `CurvineArrayLoader` — fixed-shape uint8 image arrays in .npy files:
  samples become one cropped, flipped, normalised float tensor per batch
  (NCHW or NHWC) in one kernel launch, with labels on request.

Multiprocess loading: pass ``worker_init_fn=curvine_worker_init`` so each
DataLoader worker builds its own client connection (connections must not
be shared across fork).
"""
from __future__ import annotations

import io
import tarfile
from typing import Iterator

from curvine_amd.conf import ClusterConf


class _LazySyncFs:
    """Per-process SyncFs holder (safe across DataLoader fork workers)."""

    def __init__(self, conf: ClusterConf):
        self.conf = conf
        self._fs = None
        self._pid = None

    def get(self):
        import os

        from curvine_amd.client.filesystem import SyncFs
        if self._fs is None or self._pid != os.getpid():
            self._fs = SyncFs(self.conf)
            self._pid = os.getpid()
        return self._fs


class CurvineFileDataset:
    """Map-style dataset: one item per file under a directory."""

    def __init__(self, conf: ClusterConf, root: str,
                 transform=None):
        self.holder = _LazySyncFs(conf)
        self.root = root
        self.transform = transform
        fs = self.holder.get()
        self.paths = [s.path for s in fs.list_status(root) if not s.is_dir]

    def __len__(self) -> int:
        return len(self.paths)

    def __getitem__(self, idx: int):
        data = self.holder.get().read_file(self.paths[idx])
        return self.transform(data) if self.transform else data


try:
    from torch.utils.data import IterableDataset as _TorchIterable
except ImportError:  # pragma: no cover
    class _TorchIterable:  # type: ignore[no-redef]
        pass


class CurvineShardDataset(_TorchIterable):
    """Iterable dataset over tar shards (WebDataset layout): yields
    (name, bytes) per tar member, sharded across DataLoader workers."""

    def __init__(self, conf: ClusterConf, shard_paths: list[str],
                 transform=None):
        self.holder = _LazySyncFs(conf)
        self.shards = list(shard_paths)
        self.transform = transform

    def _worker_shards(self) -> list[str]:
        try:
            import torch.utils.data as tud
            info = tud.get_worker_info()
        except ImportError:
            info = None
        if info is None:
            return self.shards
        return self.shards[info.id::info.num_workers]

    def __iter__(self) -> Iterator:
        fs = self.holder.get()
        for shard in self._worker_shards():
            blob = fs.read_file(shard)
            with tarfile.open(fileobj=io.BytesIO(blob)) as tf:
                for member in tf:
                    if not member.isfile():
                        continue
                    payload = tf.extractfile(member).read()
                    item = (member.name, payload)
                    yield self.transform(item) if self.transform else item


def curvine_worker_init(_worker_id: int) -> None:
    """No-op placeholder (per-process clients are rebuilt lazily)."""


# ---------------------------------------------------------------------------
# Zero-host-hop ingest: tar samples living in the HBM cache are gathered
# straight into torch device tensors (reader.pread_gather -> on-chip
# copy_extents_kernel).  This is the MI355X answer to BASELINE config[4]'s
# "2 TB WebDataset shards -> PyTorch DataLoader" path: indexing walks only
# the 512-byte tar headers through the local short-circuit reader; payload
# bytes never cross the host.
# ---------------------------------------------------------------------------

def index_tar(reader, length: int) -> list[tuple[str, int, int]]:
    """Walk ustar headers via pread: [(member_name, payload_off, size)].
    Only regular files are returned; other entry types are skipped by
    size.  GNU long-name entries ('L') apply to the next member."""
    out = []
    off = 0
    pending_name = None
    while off + 512 <= length:
        hdr = reader.pread(off, 512)
        if len(hdr) < 512 or hdr[0] == 0:
            break                      # end-of-archive zero block
        size = int(bytes(hdr[124:136]).split(b"\0")[0].strip() or b"0", 8)
        typ = hdr[156:157]
        payload = off + 512
        if typ == b"L":                # GNU longname: payload is the name
            pending_name = reader.pread(payload, size).rstrip(b"\0").decode()
        elif typ == b"x":              # pax extended header: path= record
            body = bytes(reader.pread(payload, size))
            pos = 0
            while pos < len(body):
                sp = body.index(b" ", pos)
                rec_len = int(body[pos:sp])
                rec = body[sp + 1:pos + rec_len - 1]   # strip trailing \n
                if rec.startswith(b"path="):
                    pending_name = rec[5:].decode()
                pos += rec_len
        elif typ in (b"0", b"\0"):
            name = pending_name or bytes(hdr[0:100]).split(b"\0")[0].decode()
            pending_name = None
            out.append((name, payload, size))
        elif typ != b"g":              # pax global header: keep pending
            pending_name = None
        off = payload + ((size + 511) & ~511)
    return out


class CurvineDeviceLoader:
    """Batched raw-sample ingest: yields (tensor, sections, names) per
    batch, where ``tensor`` is one uint8 tensor on ``device`` holding the
    concatenated payloads and ``sections`` is [(start, len)] per sample.

    HBM-tier shards + cuda device = pure D2D gather (no host hop); MEM
    tier + cpu device = host-side scatter memcpy (CPU-testable)."""

    def __init__(self, conf: ClusterConf, shard_paths: list[str],
                 device: str = "cuda:0", batch_size: int = 64,
                 shuffle: bool = False, seed: int = 0):
        from curvine_amd.client.filesystem import SyncFs
        from curvine_amd.client.reader import SyncLocalReader
        self.device = device
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.seed = seed
        self._fs = SyncFs(conf)
        self._readers = []
        self._samples = []             # (reader_idx, name, off, size)
        self._plans = None             # cached batch gather plans
        for sp in shard_paths:
            fb = self._fs.call(self._fs.fs.client.open(sp))
            r = SyncLocalReader(fb)
            ridx = len(self._readers)
            self._readers.append(r)
            for name, off, size in index_tar(r, fb.status.length):
                self._samples.append((ridx, name, off, size))

    def __len__(self) -> int:
        return (len(self._samples) + self.batch_size - 1) // self.batch_size

    @property
    def num_samples(self) -> int:
        return len(self._samples)

    def _plan(self, on_dev: bool):
        """Batch plans with sample extents pre-resolved down to arena
        triples (valid while the readers stay open — they pin the
        blocks): iteration is just torch.empty + replayed gather calls.
        The gather kernel runs ~13 µs per 16 MiB batch; Python must not
        dominate it."""
        order = list(range(len(self._samples)))
        if self.shuffle:
            import random
            random.Random(self.seed).shuffle(order)
        plans = []
        bs = self.batch_size
        for b0 in range(0, len(order), bs):
            batch = [self._samples[i] for i in order[b0:b0 + bs]]
            per_reader: dict[int, list] = {}
            sections, names = [], []
            pos = 0
            for ridx, name, off, size in batch:
                per_reader.setdefault(ridx, []).append((off, size, pos))
                sections.append((pos, size))
                names.append(name)
                pos += size
            execs = []
            for ridx, samples in per_reader.items():
                groups, slow, _ = self._readers[ridx].resolve_gather(
                    samples, on_dev)
                execs.append((self._readers[ridx], groups, slow))
            plans.append((pos, execs, sections, names))
        return plans

    def __iter__(self):
        import torch
        dev = torch.device(self.device)
        on_dev = dev.type != "cpu"
        if self._plans is None:
            self._plans = self._plan(on_dev)
        for total, execs, sections, names in self._plans:
            out = torch.empty(total, dtype=torch.uint8, device=dev)
            dst = out.data_ptr()
            for reader, groups, slow in execs:
                reader.exec_gather(groups, slow, dst)
            if on_dev:
                torch.cuda.synchronize(dev)
            yield out, sections, names

    def close(self) -> None:
        for r in self._readers:
            r.close()
        self._fs.shutdown()


# ---------------------------------------------------------------------------
# Token files: the LLM pre-training format.  A flat file of token ids
# (uint16 / uint32 / int32, after an optional header) from which every step
# draws B windows of T+1 tokens w and forms x = w[:-1], y = w[1:].  For
# HBM-tier files one token_windows_kernel launch reads each window once from
# the arena and writes both tensors, widened, counting ids outside the
# vocabulary on the way; no raw-byte tensor, no widen or slice kernels.
# Corpora are documents joined by an end-of-document id: native.token_docs
# derives position ids, document ids and cu_seqlens from the finished x.
# ---------------------------------------------------------------------------

TOKEN_DOCUMENT_OUTPUTS = ("position_ids", "doc_ids", "cu_seqlens")


class CurvineTokenLoader:
    """Batches of token windows: yields (x, y), two contiguous
    [B, seq_len] tensors of ``out_dtype`` on ``device``, fresh every batch
    and complete when yielded; y is x shifted by one token.

    File f holds n_f = (length - header_bytes) // itemsize tokens; its
    windows start at token k * stride for k in
    range((n_f - seq_len - 1) // stride + 1) (none when n_f < seq_len + 1).
    ``stride`` defaults to seq_len, so consecutive windows share one token.
    The global list is the files' windows in the order of ``paths``, or with
    ``shuffle`` that list under random.Random(seed + epoch).shuffle
    (``set_epoch``); it is cut to a multiple of ``world`` and rank r takes
    order[r::world].  Batches are consecutive groups of ``batch_size``; the
    short last one is dropped when ``drop_last``.

    With ``vocab_size`` > 0 a batch holding a token outside
    [0, vocab_size) raises InvalidArgument instead of being yielded: a
    wrong dtype or header size shows up here, not as an illegal access
    inside the embedding kernel.

    With ``documents``, any subset of ("position_ids", "doc_ids",
    "cu_seqlens"), and ``eos_id`` the loader yields (x, y, docs): a token
    equal to eos_id ends its document and belongs to it, and docs holds the
    requested tensors on ``device``, derived from x by one
    native.token_docs call per batch.  position_ids and doc_ids are
    [B, seq_len] of ``out_dtype``: positions restart at 0 after every
    eos_id (a window that begins mid-document counts from 0), doc_ids count
    the eos_id before each token in its row.  cu_seqlens is int32: the flat
    indices where a sequence starts (column 0 of every row and the token
    after every eos_id) followed by B * seq_len, n_seqs + 1 entries; it is
    a view of a B * seq_len + 1 buffer.  With it docs also holds
    "max_seqlen", an int.  y is not masked at document boundaries.

    HBM-tier files + cuda device = the device kernel; MEM tier + cpu
    device = its host twin; anything else (file tier, MEM tier + cuda
    device, tokens cut by a block boundary) goes through pread and the
    host routine.  Plans are resolved once per order and replayed; the
    readers stay open, which pins their blocks, until close()."""

    def __init__(self, conf: ClusterConf, paths: list[str], seq_len: int,
                 batch_size: int, device: str = "cuda:0",
                 src_dtype: str = "U16", out_dtype=None,
                 header_bytes: int = 0, stride: int | None = None,
                 shuffle: bool = False, seed: int = 0,
                 drop_last: bool = True, rank: int = 0, world: int = 1,
                 vocab_size: int = 0, eos_id: int | None = None,
                 documents: tuple[str, ...] = ()):
        import torch

        from curvine_amd import errors as err
        from curvine_amd import native
        from curvine_amd.client.filesystem import SyncFs
        from curvine_amd.client.reader import SyncLocalReader
        out_dtype = torch.int64 if out_dtype is None else out_dtype
        dst_dtype = {torch.int64: "I64", torch.int32: "I32"}.get(out_dtype)
        if dst_dtype is None or \
                not native.token_windows_supported(src_dtype, dst_dtype):
            raise err.Unsupported(
                f"token loader: {src_dtype} -> {out_dtype} is not a "
                "supported pair")
        stride = seq_len if stride is None else stride
        for name, v in (("seq_len", seq_len), ("batch_size", batch_size),
                        ("stride", stride)):
            if not isinstance(v, int) or v <= 0:
                raise err.InvalidArgument(
                    f"token loader: {name} must be a positive integer")
        if world <= 0 or not 0 <= rank < world:
            raise err.InvalidArgument(
                f"token loader: rank {rank} of world {world}")
        if header_bytes < 0:
            raise err.InvalidArgument("token loader: negative header_bytes")
        if vocab_size < 0:
            raise err.InvalidArgument("token loader: negative vocab_size")
        documents = tuple(documents)
        for name in documents:
            if name not in TOKEN_DOCUMENT_OUTPUTS:
                raise err.InvalidArgument(
                    f"token loader: unknown documents output {name!r}")
        if documents and eos_id is None:
            raise err.InvalidArgument(
                "token loader: documents need an eos_id")
        if eos_id is not None:
            if not isinstance(eos_id, int) or eos_id < 0:
                raise err.InvalidArgument(
                    "token loader: eos_id must be a non-negative integer")
            if vocab_size > 0 and eos_id >= vocab_size:
                raise err.InvalidArgument(
                    f"token loader: eos_id {eos_id} outside "
                    f"[0, {vocab_size})")
            if eos_id > torch.iinfo(out_dtype).max:
                raise err.InvalidArgument(
                    f"token loader: eos_id {eos_id} does not fit {out_dtype}")
        if "cu_seqlens" in documents and batch_size * seq_len >= 2 ** 31:
            raise err.InvalidArgument(
                "token loader: cu_seqlens needs batch_size * seq_len "
                "below 2**31")
        self.device = device
        self.seq_len = seq_len
        self.batch_size = batch_size
        self.src_dtype = src_dtype
        self.dst_dtype = dst_dtype
        self.out_dtype = out_dtype
        self.shuffle = shuffle
        self.seed = seed
        self.drop_last = drop_last
        self.rank = rank
        self.world = world
        self.vocab_size = vocab_size
        self.eos_id = eos_id
        self.documents = documents
        self.epoch = 0
        self._fs = SyncFs(conf)
        self._readers = []
        self._windows = []             # (reader_idx, file_off)
        self._plans = None             # (order key, batch plans)
        item = native.DTYPE_ITEMSIZE[src_dtype]
        try:
            for p in paths:
                fb = self._fs.call(self._fs.fs.client.open(p))
                ridx = len(self._readers)
                self._readers.append(SyncLocalReader(fb))
                body = fb.status.length - header_bytes
                if body < 0 or body % item:
                    raise err.InvalidArgument(
                        f"token loader: {p} is {fb.status.length} bytes, not "
                        f"a {header_bytes}-byte header plus whole "
                        f"{src_dtype} tokens")
                n_f = body // item
                if n_f >= seq_len + 1:
                    for k in range((n_f - seq_len - 1) // stride + 1):
                        self._windows.append(
                            (ridx, header_bytes + k * stride * item))
        except Exception:
            self.close()
            raise

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def _order(self) -> list[int]:
        order = list(range(len(self._windows)))
        if self.shuffle:
            import random
            random.Random(self.seed + self.epoch).shuffle(order)
        order = order[:len(order) - len(order) % self.world]
        return order[self.rank::self.world]

    @property
    def num_windows(self) -> int:
        """Windows this rank draws per epoch."""
        return len(self._windows) // self.world

    def __len__(self) -> int:
        n, bs = self.num_windows, self.batch_size
        return n // bs if self.drop_last else (n + bs - 1) // bs

    def _plan(self, on_dev: bool):
        """Batch plans with every window resolved down to arena pieces
        (valid while the readers stay open): iteration is torch.empty and
        replayed exec_token_windows calls."""
        order = self._order()
        bs = self.batch_size
        plans = []
        for b in range(len(self)):
            batch = order[b * bs:(b + 1) * bs]
            per_reader: dict[int, list] = {}
            for row, w in enumerate(batch):
                ridx, off = self._windows[w]
                per_reader.setdefault(ridx, []).append((off, row))
            execs = []
            for ridx, windows in per_reader.items():
                r = self._readers[ridx]
                groups, slow = r.resolve_token_windows(
                    windows, self.src_dtype, self.seq_len, on_dev)
                execs.append((r, groups, slow))
            plans.append((len(batch), execs))
        return plans

    def __iter__(self):
        import torch

        from curvine_amd import errors as err
        from curvine_amd import native
        dev = torch.device(self.device)
        on_dev = dev.type != "cpu"
        dev_index = -1
        if on_dev:
            dev_index = torch.cuda.current_device() if dev.index is None \
                else dev.index
        key = (self.epoch if self.shuffle else None, on_dev)
        if self._plans is None or self._plans[0] != key:
            self._plans = (key, self._plan(on_dev))
        T = self.seq_len
        for b, (rows, execs) in enumerate(self._plans[1]):
            x = torch.empty((rows, T), dtype=self.out_dtype, device=dev)
            y = torch.empty((rows, T), dtype=self.out_dtype, device=dev)
            bad = 0
            for reader, groups, slow in execs:
                bad += reader.exec_token_windows(
                    groups, slow, x.data_ptr(), y.data_ptr(), rows, T,
                    self.src_dtype, self.dst_dtype, self.vocab_size, on_dev)
            if bad:
                raise err.InvalidArgument(
                    f"token loader: {bad} token ids outside "
                    f"[0, {self.vocab_size}) in batch {b}")
            if not self.documents:
                yield x, y
                continue
            # x is complete: every exec_token_windows call has returned
            docs = {}
            ptrs = {}
            for name in self.documents:
                if name == "cu_seqlens":
                    t = torch.empty(rows * T + 1, dtype=torch.int32,
                                    device=dev)
                else:
                    t = torch.empty((rows, T), dtype=self.out_dtype,
                                    device=dev)
                docs[name] = t
                ptrs[name] = t.data_ptr()
            n_seqs, max_seqlen = native.token_docs(
                dev_index, x.data_ptr(), rows, T,
                native.DTYPES[self.dst_dtype], self.eos_id,
                ptrs.get("position_ids", 0), ptrs.get("doc_ids", 0),
                ptrs.get("cu_seqlens", 0))
            if "cu_seqlens" in docs:
                docs["cu_seqlens"] = docs["cu_seqlens"][:n_seqs + 1]
                docs["max_seqlen"] = max_seqlen
            yield x, y, docs

    def close(self) -> None:
        for r in self._readers:
            r.close()
        self._readers = []
        self._fs.shutdown()


# ---------------------------------------------------------------------------
# Document-packed batches: rows made of whole documents, targets masked at
# document ends.  The plan knows every position id, document id and sequence
# start before a batch is launched, so one kernel writes all five tensors.
# ---------------------------------------------------------------------------

TOKEN_SEG_NEXT = 1      # native.TOKEN_SEG_NEXT: the document goes on
TOKEN_SEG_PAD = 2       # native.TOKEN_SEG_PAD


def pack_segments(lengths, seq_len: int, batch_size: int):
    """First-fit packing of documents into batches of [batch_size, seq_len].

    A document of L = lengths[d] tokens becomes the segments
    [k*T, min((k+1)*T, L)) for k = 0, 1, ... with T = seq_len.  The
    segments are taken in order; each goes contiguously after the last one
    in the first row of the current batch with enough free columns; when no
    row has room the batch closes and the segment opens the next one.  A
    closed batch has batch_size rows, and every row with free columns gets
    one pad segment at its tail (a row left empty is one pad segment).

    Returns a list of batches (segments, sources), both in row-major order.
    segments[i] = (row, col, n, pos0, doc, seq, flags) as Arena.token_pack
    takes it: pos0 = k*T, doc the segment's ordinal within its row (0 for a
    pad segment), seq = i, its ordinal in the batch with pad segments
    included, flags TOKEN_SEG_NEXT when the segment does not end its
    document, TOKEN_SEG_PAD for padding, else 0.  sources[i] = (d, k*T), or
    None for a pad segment.  cu_seqlens of a batch is therefore
    [row*T + col of each segment] + [batch_size*T], strictly ascending."""
    T, B = seq_len, batch_size
    if T <= 0 or B <= 0:
        raise ValueError("pack_segments: seq_len and batch_size must be "
                         "positive")
    batches = []
    rows: list[list] = [[] for _ in range(B)]   # (n, pos0, flags, source)
    used = [0] * B
    first_open = 0                 # rows before it are full

    def close():
        segments, sources = [], []
        for r in range(B):
            col = 0
            for doc, (n, pos0, flags, src) in enumerate(rows[r]):
                segments.append((r, col, n, pos0, doc, len(segments), flags))
                sources.append(src)
                col += n
            if col < T:
                segments.append((r, col, T - col, 0, 0, len(segments),
                                 TOKEN_SEG_PAD))
                sources.append(None)
        batches.append((segments, sources))

    for d, L in enumerate(lengths):
        for t0 in range(0, L, T):
            n = min(T, L - t0)
            flags = TOKEN_SEG_NEXT if t0 + n < L else 0
            while True:
                while first_open < B and used[first_open] == T:
                    first_open += 1
                row = next((r for r in range(first_open, B)
                            if T - used[r] >= n), None)
                if row is not None:
                    break
                close()
                rows = [[] for _ in range(B)]
                used = [0] * B
                first_open = 0
            rows[row].append((n, t0, flags, (d, t0)))
            used[row] += n
    if any(used):
        close()
    return batches


class CurvinePackedTokenLoader:
    """Document-packed batches from flat token-id files: yields (x, y,
    docs) with x and y two contiguous [batch_size, seq_len] tensors of
    ``out_dtype`` on ``device``, fresh every batch and complete when
    yielded.

    A document of file f is a maximal run of tokens that ends with
    ``eos_id``; the tokens after the last eos_id form one more,
    unterminated, document when there are any.  Documents never cross
    files.  The index is built once, here: one
    SyncLocalReader.token_eos_index per file (device kernels for HBM-tier
    files with a cuda device).

    The documents are taken in file order, or with ``shuffle`` under
    random.Random(seed + epoch).shuffle (``set_epoch``); the list is cut to
    a multiple of ``world`` and rank r takes order[r::world].  They are
    packed by ``pack_segments``: whole documents side by side in a row,
    documents longer than seq_len in chunks of seq_len whose position ids
    continue, padding at the row tails.  y[r, c] is the next token of the
    same document, and ``ignore_index`` at a document's last token and in
    padding; x is ``pad_id`` (default eos_id) in padding.

    docs holds the requested ``outputs``: position_ids and doc_ids
    ([batch_size, seq_len] of ``out_dtype``; doc_ids count the segments
    of a row from 0 and are -1 in padding, position_ids count from 0 in
    padding), cu_seqlens (int32, one entry per segment in row-major order,
    pad segments included, then batch_size * seq_len) and with it
    "max_seqlen", an int.  All of them are known when the batch is
    planned: nothing is scanned per batch and no result word comes back,
    other than the vocabulary count when ``vocab_size`` > 0 (a batch
    holding a token outside [0, vocab_size) raises InvalidArgument).

    len(loader) is the minimum over all ranks of their batch counts: every
    rank computes the packing (not the block resolution) of every rank, so
    that all ranks take the same number of steps; a rank with more batches
    drops its last ones.

    HBM-tier files + cuda device = one token_pack_kernel launch per arena
    per batch; MEM tier + cpu device = its host twin; anything else (file
    tier, MEM tier + cuda device, tokens cut by a block boundary) goes
    through pread and the host routine.  A batch's plan is resolved when
    the batch is first drawn, once per order, and replayed from then on; the
    readers stay open, which pins their blocks, until close()."""

    def __init__(self, conf: ClusterConf, paths: list[str], seq_len: int,
                 batch_size: int, eos_id: int, device: str = "cuda:0",
                 src_dtype: str = "U16", out_dtype=None,
                 header_bytes: int = 0, pad_id: int | None = None,
                 ignore_index: int = -100,
                 outputs: tuple[str, ...] = TOKEN_DOCUMENT_OUTPUTS,
                 shuffle: bool = False, seed: int = 0, rank: int = 0,
                 world: int = 1, vocab_size: int = 0):
        import torch

        from curvine_amd import errors as err
        from curvine_amd import native
        from curvine_amd.client.filesystem import SyncFs
        from curvine_amd.client.reader import SyncLocalReader
        out_dtype = torch.int64 if out_dtype is None else out_dtype
        dst_dtype = {torch.int64: "I64", torch.int32: "I32"}.get(out_dtype)
        if dst_dtype is None or \
                not native.token_windows_supported(src_dtype, dst_dtype):
            raise err.Unsupported(
                f"packed token loader: {src_dtype} -> {out_dtype} is not a "
                "supported pair")
        for name, v in (("seq_len", seq_len), ("batch_size", batch_size)):
            if not isinstance(v, int) or v <= 0:
                raise err.InvalidArgument(
                    f"packed token loader: {name} must be a positive integer")
        if world <= 0 or not 0 <= rank < world:
            raise err.InvalidArgument(
                f"packed token loader: rank {rank} of world {world}")
        if header_bytes < 0:
            raise err.InvalidArgument(
                "packed token loader: negative header_bytes")
        if vocab_size < 0:
            raise err.InvalidArgument(
                "packed token loader: negative vocab_size")
        outputs = tuple(outputs)
        for name in outputs:
            if name not in TOKEN_DOCUMENT_OUTPUTS:
                raise err.InvalidArgument(
                    f"packed token loader: unknown output {name!r}")
        src_top = {"U16": 2 ** 16, "U32": 2 ** 32, "I32": 2 ** 31}[src_dtype]
        if not isinstance(eos_id, int) or not 0 <= eos_id < src_top:
            raise err.InvalidArgument(
                f"packed token loader: eos_id must be a non-negative "
                f"{src_dtype} value")
        if vocab_size > 0 and eos_id >= vocab_size:
            raise err.InvalidArgument(
                f"packed token loader: eos_id {eos_id} outside "
                f"[0, {vocab_size})")
        pad_id = eos_id if pad_id is None else pad_id
        info = torch.iinfo(out_dtype)
        for name, v in (("pad_id", pad_id), ("ignore_index", ignore_index)):
            if not isinstance(v, int) or not info.min <= v <= info.max:
                raise err.InvalidArgument(
                    f"packed token loader: {name} does not fit {out_dtype}")
        if "cu_seqlens" in outputs and batch_size * seq_len >= 2 ** 31:
            raise err.InvalidArgument(
                "packed token loader: cu_seqlens needs batch_size * seq_len "
                "below 2**31")
        self.device = device
        self.seq_len = seq_len
        self.batch_size = batch_size
        self.eos_id = eos_id
        self.src_dtype = src_dtype
        self.dst_dtype = dst_dtype
        self.out_dtype = out_dtype
        self.header_bytes = header_bytes
        self.pad_id = pad_id
        self.ignore_index = ignore_index
        self.outputs = outputs
        self.shuffle = shuffle
        self.seed = seed
        self.rank = rank
        self.world = world
        self.vocab_size = vocab_size
        self.epoch = 0
        self._on_dev = torch.device(device).type != "cpu"
        self._fs = SyncFs(conf)
        self._readers = []
        self._docs = []                # (reader_idx, first token, tokens)
        self._packs = None             # (order key, per-rank batches)
        self._plans = None             # (order key, batch plans)
        item = native.DTYPE_ITEMSIZE[src_dtype]
        try:
            for p in paths:
                fb = self._fs.call(self._fs.fs.client.open(p))
                ridx = len(self._readers)
                self._readers.append(SyncLocalReader(fb))
                body = fb.status.length - header_bytes
                if body < 0 or body % item:
                    raise err.InvalidArgument(
                        f"packed token loader: {p} is {fb.status.length} "
                        f"bytes, not a {header_bytes}-byte header plus whole "
                        f"{src_dtype} tokens")
                start = 0
                for e in self._readers[ridx].token_eos_index(
                        src_dtype, header_bytes, eos_id, self._on_dev):
                    self._docs.append((ridx, start, e + 1 - start))
                    start = e + 1
                if start < body // item:
                    self._docs.append((ridx, start, body // item - start))
        except Exception:
            self.close()
            raise

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    @property
    def num_documents(self) -> int:
        """Documents in all files."""
        return len(self._docs)

    def _key(self):
        return self.epoch if self.shuffle else None

    def _order(self, rank: int) -> list[int]:
        order = list(range(len(self._docs)))
        if self.shuffle:
            import random
            random.Random(self.seed + self.epoch).shuffle(order)
        order = order[:len(order) - len(order) % self.world]
        return order[rank::self.world]

    def _pack(self):
        """(this rank's documents, its batches cut to the common length)"""
        if self._packs is None or self._packs[0] != self._key():
            mine, batches, n = None, None, None
            for r in range(self.world):
                order = self._order(r)
                packed = pack_segments([self._docs[d][2] for d in order],
                                       self.seq_len, self.batch_size)
                n = len(packed) if n is None else min(n, len(packed))
                if r == self.rank:
                    mine, batches = order, packed
            self._packs = (self._key(), mine, batches[:n])
        return self._packs[1], self._packs[2]

    def __len__(self) -> int:
        return len(self._pack()[1])

    @property
    def pack_efficiency(self) -> float:
        """Non-pad columns over all columns of this rank's epoch."""
        batches = self._pack()[1]
        if not batches:
            return 0.0
        real = sum(s[2] for segments, _src in batches for s in segments
                   if not s[6] & TOKEN_SEG_PAD)
        return real / (len(batches) * self.batch_size * self.seq_len)

    def _plan(self, b: int):
        """The plan of batch b with every segment resolved down to arena
        pieces (valid while the readers stay open), made when the batch is
        first drawn and kept: iteration is torch.empty and replayed
        exec_token_pack calls."""
        from curvine_amd import native
        item = native.DTYPE_ITEMSIZE[self.src_dtype]
        order, batches = self._pack()
        segments, sources = batches[b]
        T = self.seq_len
        per_reader: dict[int, list] = {}
        for i, (seg, src) in enumerate(zip(segments, sources)):
            if src is None:
                continue
            ridx, start, _len = self._docs[order[src[0]]]
            off = self.header_bytes + (start + src[1]) * item
            per_reader.setdefault(ridx, []).append(
                (off, i, seg[2] + (seg[6] & TOKEN_SEG_NEXT)))
        merged: dict[int, tuple[object, list]] = {}
        slows = []
        for ridx, items in per_reader.items():
            r = self._readers[ridx]
            groups, slow = r.resolve_token_pack(items, self.src_dtype,
                                                self._on_dev)
            for arena, pieces in groups:
                merged.setdefault(arena.handle, (arena, []))[1].extend(pieces)
            slows.append((r, slow))
        # one arena call per arena per batch, made through the first reader;
        # it (or, without one, the first reader's slow path) also fills the
        # padding and cu_seqlens
        execs = [(r, list(merged.values()) if k == 0 else [], slow,
                  None if k == 0 else False)
                 for k, (r, slow) in enumerate(slows)]
        cu = [s[0] * T + s[1] for s in segments] + [self.batch_size * T]
        max_seqlen = max(b - a for a, b in zip(cu, cu[1:]))
        return segments, execs, max_seqlen

    def __iter__(self):
        import torch

        from curvine_amd import errors as err
        dev = torch.device(self.device)
        if self._plans is None or self._plans[0] != self._key():
            self._plans = (self._key(), [None] * len(self))
        plans = self._plans[1]
        B, T = self.batch_size, self.seq_len
        for b in range(len(plans)):
            if plans[b] is None:
                plans[b] = self._plan(b)
            segments, execs, max_seqlen = plans[b]
            x = torch.empty((B, T), dtype=self.out_dtype, device=dev)
            y = torch.empty((B, T), dtype=self.out_dtype, device=dev)
            docs = {}
            for name in self.outputs:
                if name == "cu_seqlens":
                    docs[name] = torch.empty(len(segments) + 1,
                                             dtype=torch.int32, device=dev)
                else:
                    docs[name] = torch.empty((B, T), dtype=self.out_dtype,
                                             device=dev)
            ptrs = {k: t.data_ptr() for k, t in docs.items()}
            bad = 0
            for reader, groups, slow, fill in execs:
                bad += reader.exec_token_pack(
                    groups, slow, segments, x.data_ptr(), y.data_ptr(),
                    ptrs.get("position_ids", 0), ptrs.get("doc_ids", 0),
                    ptrs.get("cu_seqlens", 0), B, T, self.src_dtype,
                    self.dst_dtype, self.pad_id, self.ignore_index,
                    self.vocab_size, self._on_dev, fill)
            if bad:
                raise err.InvalidArgument(
                    f"packed token loader: {bad} token ids outside "
                    f"[0, {self.vocab_size}) in batch {b}")
            if "cu_seqlens" in docs:
                docs["max_seqlen"] = max_seqlen
            yield x, y, docs

    def close(self) -> None:
        for r in self._readers:
            r.close()
        self._readers = []
        self._fs.shutdown()


# ---------------------------------------------------------------------------
# Array files: fixed-shape uint8 image arrays kept as .npy ([N, H, W, C] or
# [N, H, W]), the preprocessed-shard format of image, frame and patch
# datasets.  For HBM-tier files one array_samples_kernel launch per batch
# reads each sample's crop once from the arena and writes the normalised
# float tensor in its final layout; no raw-byte tensor, no f32 temporary, no
# per-sample crop and flip launches.
# ---------------------------------------------------------------------------

NPY_MAGIC = b"\x93NUMPY"
NPY_PROBE = 4096          # bytes read first when looking for a header


def _npy_header(buf):
    """(header_bytes, shape, descr, fortran_order) of the .npy file that
    begins with `buf`, format version 1.0, 2.0 or 3.0; InvalidArgument when
    `buf` ends inside the header, Unsupported for anything that is not such
    a header."""
    import ast
    import struct

    from curvine_amd import errors as err
    buf = bytes(buf)
    if len(buf) < 8 and NPY_MAGIC.startswith(buf[:6]):
        raise err.InvalidArgument("npy header: file ends inside the header")
    if buf[:6] != NPY_MAGIC:
        raise err.Unsupported("npy header: not a .npy file")
    version = (buf[6], buf[7])
    if version == (1, 0):
        pre, fmt = 10, "<H"
    elif version in ((2, 0), (3, 0)):
        pre, fmt = 12, "<I"
    else:
        raise err.Unsupported(f"npy header: format version {version}")
    if len(buf) < pre:
        raise err.InvalidArgument("npy header: file ends inside the header")
    hlen = struct.unpack_from(fmt, buf, 8)[0]
    if len(buf) < pre + hlen:
        raise err.InvalidArgument(
            f"npy header: {pre + hlen} header bytes, {len(buf)} given")
    text = buf[pre:pre + hlen].decode("utf-8" if version[0] == 3
                                      else "latin1")
    try:
        d = ast.literal_eval(text)
        shape, descr = tuple(d["shape"]), d["descr"]
        fortran = bool(d["fortran_order"])
        if not all(isinstance(n, int) and n >= 0 for n in shape):
            raise ValueError(shape)
    except Exception:  # noqa: BLE001 - whatever a malformed dict raises
        raise err.Unsupported("npy header: malformed dictionary") from None
    return pre + hlen, shape, descr, fortran


def parse_npy_header(buf):
    """Header of an image-array .npy file: (header_bytes, shape, descr,
    fortran_order) from the file's first bytes.  Only descr '|u1', C order
    and a 3-d [N, H, W] or 4-d [N, H, W, C] shape pass; anything else is
    Unsupported.  `buf` ending inside the header is InvalidArgument."""
    from curvine_amd import errors as err
    header_bytes, shape, descr, fortran = _npy_header(buf)
    if descr != "|u1":
        raise err.Unsupported(f"npy header: dtype {descr!r}, only '|u1'")
    if fortran:
        raise err.Unsupported("npy header: Fortran order")
    if len(shape) not in (3, 4):
        raise err.Unsupported(
            f"npy header: shape {shape}, only [N, H, W] and [N, H, W, C]")
    return header_bytes, shape, descr, fortran


def _pread_npy(reader, length: int, parse):
    """parse() over the first bytes of a file, the probe widened once to the
    length a long header asks for."""
    from curvine_amd import errors as err
    head = reader.pread(0, min(NPY_PROBE, length))
    try:
        return parse(head)
    except err.InvalidArgument:
        if len(head) == length:
            raise
    import struct
    want = 12 + struct.unpack_from("<I", head, 8)[0] if head[6] >= 2 \
        else 10 + struct.unpack_from("<H", head, 8)[0]
    return parse(reader.pread(0, min(want, length)))


def _f32(v: float) -> float:
    """v rounded once to float32."""
    import struct
    return struct.unpack("<f", struct.pack("<f", v))[0]


class CurvineArrayLoader:
    """Batches of image samples: yields x, one contiguous tensor of
    ``out_dtype`` (float32, float16 or bfloat16) on ``device``, [B, C, h, w]
    for layout "NCHW" or [B, h, w, C] for "NHWC", fresh every batch and
    complete when yielded; with ``labels`` it yields (x, labels), labels an
    int64 tensor on ``device``.

    Each path is a .npy file (format 1.0, 2.0 or 3.0) holding a C-order
    uint8 array [N, H, W, C] with 1 <= C <= 4, or [N, H, W] read as C = 1;
    other headers are Unsupported (`parse_npy_header`), files of different
    H, W, C or shorter than their header promises InvalidArgument.

    ``crop`` = (h, w), or one int for both, defaults to the whole frame.
    Element [b, c, r, q] is f32(f32(v) * scale[c]) + bias[c] cast to
    ``out_dtype``, v the source byte at pixel (dy + r, dx + q), or
    (dy + r, dx + w-1-q) when the sample is flipped; scale[c] =
    float32(1 / (255 * std[c])) and bias[c] = float32(-mean[c] / std[c])
    (``loader.scale``, ``loader.bias``; mean defaults to 0 and std to 1, so
    the default maps bytes to [0, 1]).

    The global list is the files' samples in the order of ``paths``, or
    with ``shuffle`` that list under random.Random(seed + epoch).shuffle
    (``set_epoch``); it is cut to a multiple of ``world`` and rank r takes
    order[r::world].  The same Random then draws, for every position of the
    global list in turn, dy = randrange(H-h+1) and dx = randrange(W-w+1)
    when ``random_crop`` and flip = randrange(2) when ``random_flip``, so
    every rank derives the same table; without ``random_crop`` the crop is
    centred, dy = (H-h)//2 and dx = (W-w)//2.  ``augmentation()`` returns
    this rank's [(dy, dx, flip)] for the current epoch.  Batches are
    consecutive groups of ``batch_size``; the short last one is dropped
    when ``drop_last``.

    ``labels`` is one .npy path per data path, 1-d '<i8' or '<i4' of
    length N, read once at construction; one index operation per plan puts
    this rank's labels on ``device`` in order and every batch is a slice.

    HBM-tier files + cuda device = the device kernel; MEM tier + cpu device
    = its host twin; any sample with a part elsewhere (file tier, MEM tier
    + cuda device, a hole) goes whole through pread and the host routine.
    Plans are resolved once per order and replayed; the readers stay open,
    which pins their blocks, until close()."""

    def __init__(self, conf: ClusterConf, paths: list[str], batch_size: int,
                 device: str = "cuda:0", out_dtype=None, crop=None,
                 random_crop: bool = False, random_flip: bool = False,
                 mean=None, std=None, layout: str = "NCHW", labels=None,
                 shuffle: bool = False, seed: int = 0,
                 drop_last: bool = True, rank: int = 0, world: int = 1):
        import torch

        from curvine_amd import errors as err
        from curvine_amd import native
        from curvine_amd.client.filesystem import SyncFs
        from curvine_amd.client.reader import SyncLocalReader
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        dst_dtype = {torch.float32: "F32", torch.float16: "F16",
                     torch.bfloat16: "BF16"}.get(out_dtype)
        if dst_dtype is None or not native.array_samples_supported(dst_dtype):
            raise err.Unsupported(
                f"array loader: {out_dtype} is not a supported output")
        if layout not in native.ARRAY_LAYOUTS:
            raise err.InvalidArgument(
                f"array loader: unknown layout {layout!r}")
        if not isinstance(batch_size, int) or batch_size <= 0:
            raise err.InvalidArgument(
                "array loader: batch_size must be a positive integer")
        if world <= 0 or not 0 <= rank < world:
            raise err.InvalidArgument(
                f"array loader: rank {rank} of world {world}")
        if labels is not None and len(labels) != len(paths):
            raise err.InvalidArgument(
                "array loader: one labels path per data path")
        self.device = device
        self.batch_size = batch_size
        self.out_dtype = out_dtype
        self.dst_dtype = dst_dtype
        self.layout = layout
        self.random_crop = random_crop
        self.random_flip = random_flip
        self.shuffle = shuffle
        self.seed = seed
        self.drop_last = drop_last
        self.rank = rank
        self.world = world
        self.epoch = 0
        self.shape = None              # (H, W, C)
        self._fs = SyncFs(conf)
        self._readers = []
        self._samples = []             # (reader_idx, file_off)
        self._labels = None            # int64 on the cpu, one per sample
        self._plans = None             # (order key, batch plans, labels)
        label_parts = []
        try:
            for i, p in enumerate(paths):
                fb = self._fs.call(self._fs.fs.client.open(p))
                ridx = len(self._readers)
                r = SyncLocalReader(fb)
                self._readers.append(r)
                length = fb.status.length
                hb, shp, _descr, _f = _pread_npy(r, length, parse_npy_header)
                n, hwc = shp[0], tuple(shp[1:]) + (1,) * (4 - len(shp))
                if not 1 <= hwc[2] <= 4 or 0 in hwc:
                    raise err.Unsupported(
                        f"array loader: {p} holds samples of shape {hwc}")
                if self.shape is None:
                    self.shape = hwc
                elif hwc != self.shape:
                    raise err.InvalidArgument(
                        f"array loader: {p} holds samples of shape {hwc}, "
                        f"the files before it {self.shape}")
                sb = hwc[0] * hwc[1] * hwc[2]
                if length < hb + n * sb:
                    raise err.InvalidArgument(
                        f"array loader: {p} is {length} bytes, its header "
                        f"promises {hb + n * sb}")
                self._samples += [(ridx, hb + k * sb) for k in range(n)]
                if labels is not None:
                    label_parts.append(self._read_labels(labels[i], n))
            if self.shape is None:
                raise err.InvalidArgument("array loader: no files")
            if labels is not None:
                self._labels = torch.cat(label_parts)
            H, W, C = self.shape
            crop = (H, W) if crop is None else crop
            crop = (crop, crop) if isinstance(crop, int) else tuple(crop)
            if len(crop) != 2 or not all(isinstance(v, int) for v in crop) \
                    or not (1 <= crop[0] <= H and 1 <= crop[1] <= W):
                raise err.InvalidArgument(
                    f"array loader: crop {crop} of a {H}x{W} frame")
            self.crop = crop
            self.scale, self.bias = self._normalisation(mean, std, C)
        except Exception:
            self.close()
            raise

    @staticmethod
    def _normalisation(mean, std, C: int):
        from curvine_amd import errors as err

        def per_channel(v, default):
            if v is None:
                return [default] * C
            if isinstance(v, (int, float)):
                return [float(v)] * C
            v = [float(t) for t in v]
            if len(v) != C:
                raise err.InvalidArgument(
                    f"array loader: {len(v)} mean/std values for {C} "
                    "channels")
            return v
        import math
        mean, std = per_channel(mean, 0.0), per_channel(std, 1.0)
        if any(s == 0 or not math.isfinite(s) for s in std) or \
                any(not math.isfinite(m) for m in mean):
            raise err.InvalidArgument(
                "array loader: mean and std must be finite, std not zero")
        scale = tuple(_f32(1.0 / (255.0 * s)) for s in std)
        bias = tuple(_f32(-m / s) for m, s in zip(mean, std))
        return scale, bias

    def _read_labels(self, path: str, n: int):
        """The labels of one data file as an int64 cpu tensor."""
        import torch

        from curvine_amd import errors as err
        from curvine_amd.client.reader import SyncLocalReader
        fb = self._fs.call(self._fs.fs.client.open(path))
        r = SyncLocalReader(fb)
        try:
            length = fb.status.length
            hb, shp, descr, fortran = _pread_npy(r, length, _npy_header)
            dt = {"<i8": torch.int64, "<i4": torch.int32}.get(descr)
            if dt is None or len(shp) != 1:
                raise err.Unsupported(
                    f"array loader: labels {path} are {descr!r} {shp}, "
                    "only 1-d '<i8' and '<i4'")
            if shp[0] != n:
                raise err.InvalidArgument(
                    f"array loader: {shp[0]} labels in {path} for {n} "
                    "samples")
            nbytes = n * dt.itemsize
            raw = r.pread(hb, nbytes)
            if len(raw) != nbytes:
                raise err.InvalidArgument(
                    f"array loader: labels {path} shorter than the header "
                    "promises")
            if n == 0:
                return torch.empty(0, dtype=torch.int64)
            return torch.frombuffer(bytearray(raw), dtype=dt).to(torch.int64)
        finally:
            r.close()

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def _order(self):
        """This rank's (sample indices, [(dy, dx, flip)]) for the epoch."""
        import random
        H, W, _C = self.shape
        h, w = self.crop
        order = list(range(len(self._samples)))
        rng = random.Random(self.seed + self.epoch)
        if self.shuffle:
            rng.shuffle(order)
        aug = []
        for _ in order:
            dy, dx, flip = (H - h) // 2, (W - w) // 2, 0
            if self.random_crop:
                dy = rng.randrange(H - h + 1)
                dx = rng.randrange(W - w + 1)
            if self.random_flip:
                flip = rng.randrange(2)
            aug.append((dy, dx, flip))
        keep = len(order) - len(order) % self.world
        return order[:keep][self.rank::self.world], \
            aug[:keep][self.rank::self.world]

    def augmentation(self) -> list[tuple[int, int, int]]:
        """This rank's (dy, dx, flip) per sample, in the order drawn, for
        the current epoch."""
        return self._order()[1]

    @property
    def num_samples(self) -> int:
        """Samples this rank draws per epoch."""
        return len(self._samples) // self.world

    def __len__(self) -> int:
        n, bs = self.num_samples, self.batch_size
        return n // bs if self.drop_last else (n + bs - 1) // bs

    def _plan(self, on_dev: bool, dev):
        """Batch plans with every sample resolved down to arena pieces
        (valid while the readers stay open), the pieces of one arena merged
        across files so a batch is one launch, and this rank's labels on
        the device in order."""
        import torch
        order, aug = self._order()
        H, W, C = self.shape
        bs = self.batch_size
        plans = []
        for b in range(len(self)):
            batch = order[b * bs:(b + 1) * bs]
            rows = aug[b * bs:(b + 1) * bs]
            per_reader: dict[int, list] = {}
            for row, i in enumerate(batch):
                ridx, off = self._samples[i]
                per_reader.setdefault(ridx, []).append((off, row))
            merged: dict[int, tuple[object, list]] = {}
            execs = []
            for ridx, samples in per_reader.items():
                r = self._readers[ridx]
                groups, slow = r.resolve_array_samples(samples, H * W * C,
                                                       on_dev)
                for arena, pieces in groups:
                    merged.setdefault(arena.handle, (arena, []))[1].extend(
                        pieces)
                if slow or not execs:
                    execs.append((r, [], slow))
            execs[0] = (execs[0][0], list(merged.values()), execs[0][2])
            plans.append((len(batch), rows, execs))
        labels = None
        if self._labels is not None:
            n = sum(p[0] for p in plans)
            labels = self._labels[torch.tensor(order[:n], dtype=torch.int64)]
            labels = labels.to(dev)
        return plans, labels

    def __iter__(self):
        import torch
        dev = torch.device(self.device)
        on_dev = dev.type != "cpu"
        varies = self.shuffle or self.random_crop or self.random_flip
        key = (self.epoch if varies else None, on_dev)
        if self._plans is None or self._plans[0] != key:
            self._plans = (key, *self._plan(on_dev, dev))
        _key, plans, labels = self._plans
        H, W, C = self.shape
        h, w = self.crop
        at = 0
        for n, rows, execs in plans:
            dims = (n, C, h, w) if self.layout == "NCHW" else (n, h, w, C)
            x = torch.empty(dims, dtype=self.out_dtype, device=dev)
            for reader, groups, slow in execs:
                reader.exec_array_samples(
                    groups, slow, x.data_ptr(), n, rows, self.shape,
                    self.crop, self.scale, self.bias, self.dst_dtype,
                    self.layout, on_dev)
            if labels is None:
                yield x
            else:
                yield x, labels[at:at + n]
            at += n

    def close(self) -> None:
        for r in self._readers:
            r.close()
        self._readers = []
        self._fs.shutdown()
