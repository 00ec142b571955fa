#!/usr/bin/env python3
"""Flagship benchmark: FUSE sequential-read GB/s (and 4K random IOPS) on
MI355X HBM cache tiers — the BASELINE.json metric.

Per rank (one per GPU, weak scaling): rank 0 hosts the master; every rank
spawns a cv-fuse daemon process embedding the worker that owns its GPU's
HBM arena, writes a synthetic random-byte dataset through the mount, then
times fio-style reads through the kernel mount (default: T threads x 1 MiB
sequential; --workload randread4k for the IOPS path).

Driver contract: rank 0 prints ONE JSON line; timing is bracketed by
barrier + torch.cuda.synchronize on both sides; value is the whole-job
aggregate (max elapsed over ranks).  --path client bypasses FUSE and reads
via the in-process client (plumbing mode / containers without /dev/fuse).

A plain run sets up, warms up, times --steps steps and prints the result
line.  --dump-outputs DIR also saves a fixed seeded sample of the bytes the
last timed step delivered (same arguments -> same inputs -> comparable
across builds).  --full is the switch for secondary measurements.
"""
from __future__ import annotations

import argparse
import asyncio
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

REFERENCE_PEAK_GIBPS = 9.5     # 256 KiB seq read, 32 threads
REFERENCE_PEAK_RAND_GIBPS = 9.0


DUMP_SAMPLE_BYTES = 64 << 10   # one sampled extent of a sequential file
DUMP_MAX_EXTENTS = 128         # 128 x 64 KiB x float32 = 32 MiB on disk
DUMP_RAND_OPS = 16             # 4 KiB reads kept per randread4k thread


def log(rank, *a):
    print(f"[bench r{rank}]", *a, file=sys.stderr, flush=True)


class OutputCapture:
    """--dump-outputs: a fixed, seeded sample of the bytes the timed path
    handed its caller in the LAST timed step.  Sequential workloads keep
    DUMP_SAMPLE_BYTES-long extents at seeded (file, offset) positions;
    randread4k keeps the first reads of every thread, up to DUMP_RAND_OPS
    or as many as the shortest thread issued (their offsets are seeded per
    thread, so they repeat from run to run).  Each thread fills rows of
    its own, so no lock is needed."""

    def __init__(self, args, rank):
        import random
        import numpy as np
        self.np = np
        self.workload = args.workload
        if args.workload == "randread4k":
            self.rows = np.zeros((args.threads, DUMP_RAND_OPS, 4096),
                                 dtype=np.uint8)
            self.filled = np.zeros((args.threads, DUMP_RAND_OPS),
                                   dtype=np.int64)
            self.want = 4096
            return
        rng = random.Random(0x5EED + rank)
        self.want = min(DUMP_SAMPLE_BYTES, args.file_size)
        n = min(args.files * 4, DUMP_MAX_EXTENTS)
        self.rows = np.zeros((n, self.want), dtype=np.uint8)
        self.filled = np.zeros(n, dtype=np.int64)
        self.extents: dict[int, list[tuple[int, int]]] = {}
        for row in range(n):
            off = rng.randrange(args.file_size - self.want + 1)
            self.extents.setdefault(row % args.files, []).append((off, row))

    def take(self, i, pos, view):
        """`view` holds bytes [pos, pos + len(view)) of file i."""
        end = pos + len(view)
        for off, row in self.extents.get(i, ()):
            lo, hi = max(off, pos), min(off + self.want, end)
            if lo < hi:
                self.rows[row, lo - off:hi - off] = self.np.frombuffer(
                    view, dtype=self.np.uint8)[lo - pos:hi - pos]
                self.filled[row] += hi - lo

    def take_rand(self, t, j, view):
        """`view` holds the j-th 4 KiB read of thread t."""
        self.rows[t, j, :len(view)] = self.np.frombuffer(
            view, dtype=self.np.uint8)
        self.filled[t, j] += len(view)

    def save(self, out_dir, rank):
        if self.workload == "randread4k":
            # a step issues the same number of reads on every thread
            k = int((self.filled != 0).all(axis=0).sum())
            if k == 0:
                raise RuntimeError("--dump-outputs: the last timed step "
                                   "issued no read on some thread")
            self.rows, self.filled = self.rows[:, :k], self.filled[:, :k]
        if (self.filled != self.want).any():
            raise RuntimeError(
                "--dump-outputs: the last timed step did not deliver every "
                f"sampled extent ({int((self.filled != self.want).sum())} "
                "incomplete)")
        os.makedirs(out_dir, exist_ok=True)
        dest = os.path.join(out_dir, f"{self.workload}_r{rank}.npy")
        self.np.save(dest, self.rows.astype(self.np.float32))
        return dest


class ClusterRuntime:
    """Master (rank0) + optional in-process worker + client on a dedicated
    asyncio loop thread."""

    def __init__(self):
        self.loop = asyncio.new_event_loop()
        self._t = threading.Thread(target=self._run, daemon=True)
        self._t.start()
        self.master = None
        self.worker = None
        self.fs = None

    def _run(self):
        from concurrent.futures import ThreadPoolExecutor
        asyncio.set_event_loop(self.loop)
        workers = min(64, (os.cpu_count() or 8) * 2)
        self.loop.set_default_executor(
            ThreadPoolExecutor(max_workers=workers, thread_name_prefix="cv-io"))
        self.loop.run_forever()

    def call(self, coro, timeout=600.0):
        return asyncio.run_coroutine_threadsafe(coro, self.loop).result(timeout)

    def stop(self):
        self.loop.call_soon_threadsafe(self.loop.stop)
        self._t.join(timeout=5)


def build_conf(args, tmp, rank):
    from curvine_amd.testing import test_conf
    conf = test_conf(tmp)
    conf.master.block_size = args.block_size
    conf.client.block_size = args.block_size
    conf.master.heartbeat_check_ms = 1000
    # seqwrite overwrites each step; block frees ride the heartbeat
    # command channel, so keep it snappy to bound transient capacity use
    conf.worker.heartbeat_interval_ms = \
        250 if args.workload == "seqwrite" else 1000
    conf.client.write_chunk_size = 4 << 20
    conf.client.read_chunk_size = args.read_chunk
    conf.worker.staging_buf_bytes = args.staging_bytes
    conf.worker.staging_buf_count = args.staging_count
    conf.fuse.mnt_number = args.fuse_channels
    return conf


def setup(args, rank, world, dist, has_gpu):
    from curvine_amd.master.server import Master
    from curvine_amd.worker.server import Worker
    from curvine_amd.client.filesystem import CurvineFileSystem

    tmp = tempfile.mkdtemp(prefix=f"curvine-bench-r{rank}-")
    conf = build_conf(args, tmp, rank)
    rt = ClusterRuntime()
    master_port = 0
    if rank == 0:
        conf.master.rpc_port = 0
        rt.master = rt.call(Master(conf).start())
        master_port = rt.master.rpc.port
    if world > 1:
        obj = [master_port]
        dist.broadcast_object_list(obj, src=0)
        master_port = obj[0]
    conf.client.master_addrs = [f"127.0.0.1:{master_port}"]
    conf.master.rpc_port = master_port

    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    if has_gpu:
        data_dirs = [f"[HBM:{args.hbm_gb}GB:{local_rank}]gpu{local_rank}"]
    else:
        data_dirs = [f"[MEM:{args.hbm_gb}GB]{tmp}/mem"]

    daemon_proc, mnt = None, None
    if args.path == "fuse":
        mnt = f"/tmp/curvine-bench-mnt-r{rank}"
        daemon_proc = subprocess.Popen(
            [sys.executable, "-m", "curvine_amd.fuse", "--mnt", mnt,
             "--master", f"127.0.0.1:{master_port}",
             "--embed-worker", "--device", str(local_rank if has_gpu else -1),
             "--channels", str(args.fuse_channels),
             "--log-level", "WARNING"] +
            [f"--data-dir={d}" for d in data_dirs],
            stdout=subprocess.PIPE, stderr=sys.stderr, text=True,
            cwd=os.path.dirname(os.path.abspath(__file__)))
        line = daemon_proc.stdout.readline()
        if not line.startswith("READY"):
            raise RuntimeError(f"cv-fuse failed to start: {line!r}")
    elif args.no_short_circuit or args.separate_worker:
        # faithful remote plane: the worker is its OWN process, every
        # byte crosses its streaming RPC over loopback
        hb = 250 if args.workload == "seqwrite" else 1000
        wp = subprocess.Popen(
            [sys.executable, "-m", "curvine_amd.server_main",
             "--service", "worker", "--master-port", str(master_port),
             "--worker-port", "0", "--heartbeat-ms", str(hb),
             "--device", str(local_rank if has_gpu else -1),
             "--log-level", "WARNING"] +
            [f"--data-dir={d}" for d in data_dirs],
            stderr=sys.stderr,
            cwd=os.path.dirname(os.path.abspath(__file__)))
        daemon_proc = wp

        async def wait_worker():
            from curvine_amd.client.filesystem import CurvineFileSystem as _C
            f = _C(conf)
            for _ in range(100):
                info = await f.get_master_info()
                if info["live_workers"]:
                    await f.close()
                    return
                await asyncio.sleep(0.2)
            raise RuntimeError("worker process never registered")
        rt.call(wait_worker())
    else:
        conf.worker.data_dirs = data_dirs
        conf.worker.rpc_port = 0
        rt.worker = rt.call(Worker(conf, worker_id=rank + 1,
                                   device_id=local_rank).start())

    async def mkfs():
        return CurvineFileSystem(conf)
    rt.fs = rt.call(mkfs())
    if rt.worker is not None:
        rt.fs.client.local_worker_id = rt.worker.worker_id
    return rt, conf, daemon_proc, mnt


def write_dataset(args, rank, rt, mnt):
    import numpy as np
    rng = np.random.default_rng(1234 + rank)
    base = rng.integers(0, 256, size=8 << 20, dtype=np.uint8).tobytes()
    if mnt is not None:
        os.makedirs(f"{mnt}/bench/r{rank}", exist_ok=True)
        for i in range(args.files):
            with open(f"{mnt}/bench/r{rank}/f{i}", "wb") as f:
                remaining = args.file_size
                while remaining > 0:
                    n = min(len(base), remaining)
                    f.write(base[:n])
                    remaining -= n
    else:
        async def write_one(i):
            w = await rt.fs.create(f"/bench/r{rank}/f{i}", overwrite=True,
                                   storage_tier="HBM")
            remaining = args.file_size
            while remaining > 0:
                n = min(len(base), remaining)
                await w.write(base[:n] if n < len(base) else base)
                remaining -= n
            await w.complete()
        for i in range(args.files):
            rt.call(write_one(i))


# ---------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------

def step_fuse_seq(args, rank, mnt, cap=None) -> int:
    """T threads, each sequentially reading its share of files in
    read_chunk chunks through the kernel mount."""
    paths = [f"{mnt}/bench/r{rank}/f{i}" for i in range(args.files)]
    total = [0] * args.threads
    errs = []

    def worker(t):
        try:
            buf = bytearray(args.read_chunk)
            mv = memoryview(buf)
            for i in range(t, len(paths), args.threads):
                fd = os.open(paths[i], os.O_RDONLY)
                pos = 0
                try:
                    while True:
                        n = os.readv(fd, [mv])
                        if n <= 0:
                            break
                        if cap is not None:
                            cap.take(i, pos, mv[:n])
                        pos += n
                        total[t] += n
                finally:
                    os.close(fd)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=worker, args=(t,))
               for t in range(args.threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]
    got = sum(total)
    expect = args.files * args.file_size
    if got != expect:
        raise RuntimeError(f"step read {got} != {expect}")
    return got


def step_fuse_rand4k(args, rank, mnt, lat_out: list, cap=None) -> int:
    """T threads x N random 4 KiB preads (the IOPS path)."""
    paths = [f"{mnt}/bench/r{rank}/f{i}" for i in range(args.files)]
    import random
    per_thread = args.rand_reads // args.threads
    total = [0] * args.threads
    lats: list[list[float]] = [[] for _ in range(args.threads)]
    errs = []

    def worker(t):
        try:
            rng = random.Random(t * 7919 + rank)
            fds = [os.open(p, os.O_RDONLY) for p in paths]
            try:
                for j in range(per_thread):
                    fd = fds[rng.randrange(len(fds))]
                    off = rng.randrange(max(1, args.file_size - 4096))
                    t0 = time.perf_counter_ns()
                    data = os.pread(fd, 4096, off)
                    lats[t].append((time.perf_counter_ns() - t0) / 1000.0)
                    if cap is not None and j < cap.rows.shape[1]:
                        cap.take_rand(t, j, data)
                    total[t] += len(data)
            finally:
                for fd in fds:
                    os.close(fd)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=worker, args=(t,))
               for t in range(args.threads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]
    alll = sorted(x for l in lats for x in l)
    if alll:
        lat_out.append({"p50_us": alll[len(alll) // 2],
                        "p99_us": alll[int(len(alll) * 0.99)],
                        "convention": "per-op pread wall time"})
    return sum(total)


def _sync_readers(args, rank, rt):
    """Open all rank-local files as synchronous short-circuit readers."""
    readers = []
    for i in range(args.files):
        r = rt.call(rt.fs.open(f"/bench/r{rank}/f{i}"))
        readers.append(r.to_sync())
        r.close()
    return readers


def step_client_seq_remote(args, rank, rt, disable_sc: bool = True,
                           cap=None) -> int:
    """Sequential reads with short-circuit DISABLED: every byte crosses
    the worker's streaming RPC (the inter-node data plane, exercised
    over loopback — one concurrent stream per file)."""
    async def run():
        if disable_sc:
            rt.fs.client.conf.client.short_circuit = False
        readers = [await rt.fs.open(f"/bench/r{rank}/f{i}")
                   for i in range(args.files)]

        async def read_file(i, r):
            buf = bytearray(args.read_chunk)
            pos = 0
            while pos < r.length:
                want = min(args.read_chunk, r.length - pos)
                got = await r.pread_into(pos, buf, 0, want)
                if got <= 0:
                    break
                if cap is not None:
                    cap.take(i, pos, memoryview(buf)[:got])
                pos += got
            return pos
        try:
            totals = await asyncio.gather(
                *(read_file(i, r) for i, r in enumerate(readers)))
        finally:
            for r in readers:
                r.close()
            rt.fs.client.conf.client.short_circuit = True
        return sum(totals)
    return rt.call(run())


def step_client_rand4k(args, rank, rt, lat_out: list, cap=None) -> int:
    """Random 4 KiB reads via the SYNC short-circuit path: plain OS
    threads, no event loop in the per-op path (this is the IOPS metric)."""
    import random
    readers = _sync_readers(args, rank, rt)
    per_thread = args.rand_reads // args.threads
    total = [0] * args.threads
    lats: list[list[float]] = [[] for _ in range(args.threads)]
    errs = []

    from curvine_amd import native
    use_pinned = native.gpu_available()
    depth = max(1, args.iodepth)

    def worker(t):
        try:
            rng = random.Random(t * 7919 + rank)
            pbuf = native.PinnedBuffer(4096 * depth) if use_pinned else None
            buf = bytearray(4096) if pbuf is None else None
            batches = per_thread // depth
            keep = cap.rows.shape[1] if cap is not None else 0
            done = 0   # 4 KiB reads this thread has finished
            for _ in range(max(1, batches)):
                r = readers[rng.randrange(len(readers))]
                t0 = time.perf_counter_ns()
                if pbuf is not None and depth > 1:
                    offs = [rng.randrange(max(1, r.length - 4096))
                            for _ in range(depth)]
                    r.pread_batch_ptr(offs, 4096, pbuf.ptr, 4096)
                    n = 4096 * depth
                elif pbuf is not None:
                    n = r.pread_into_ptr(
                        rng.randrange(max(1, r.length - 4096)), pbuf.ptr, 4096)
                else:
                    n = r.pread_into(
                        rng.randrange(max(1, r.length - 4096)), buf, 0, 4096)
                # latency per IO (batch wall / depth, the fio convention)
                lats[t].append((time.perf_counter_ns() - t0) / 1000.0 / depth)
                total[t] += n
                if done < keep:
                    got = pbuf.view if pbuf is not None else memoryview(buf)
                    for k in range(min(n // 4096, keep - done)):
                        cap.take_rand(t, done + k,
                                      got[k * 4096:(k + 1) * 4096])
                done += n // 4096
            if pbuf is not None:
                pbuf.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=worker, args=(t,))
           for t in range(args.threads)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for r in readers:
        r.close()
    if errs:
        raise errs[0]
    alll = sorted(x for l in lats for x in l)
    if alll:
        lat_out.append({"p50_us": alll[len(alll) // 2],
                        "p99_us": alll[int(len(alll) * 0.99)],
                        "convention": "iodepth-amortized (batch wall / depth)"})
    return sum(total)


def step_client_seq(args, rank, rt, cap=None) -> int:
    """Sequential reads via the SYNC short-circuit path: OS threads with
    pinned destination buffers (direct D2H DMA, no event loop per op).
    Covers in-process registry hits AND hipIpc-mapped other-process
    arenas; with neither available (CPU separate-worker), falls back to
    the async streaming path without touching the short-circuit conf."""
    from curvine_amd import native
    use_pinned = native.gpu_available()
    try:
        readers = _sync_readers(args, rank, rt)
    except Exception:
        return step_client_seq_remote(args, rank, rt, disable_sc=False,
                                      cap=cap)
    nthreads = min(args.threads, max(1, len(readers)))
    total = [0] * nthreads
    errs = []

    depth = max(1, args.seq_batch)

    def worker(t):
        try:
            pbuf = native.PinnedBuffer(args.read_chunk * depth) \
                if use_pinned else None
            buf = None if pbuf else bytearray(args.read_chunk)
            # thread t reads files t, t+T, ... fully (fio numjobs analog)
            for i in range(t, len(readers), nthreads):
                r = readers[i]
                pos = 0
                while pos < r.length:
                    if pbuf is not None and \
                            pos + args.read_chunk * depth <= r.length:
                        # depth chunks issued async on one stream, ONE
                        # sync — overlaps successive D2H DMAs
                        offs = [pos + k * args.read_chunk
                                for k in range(depth)]
                        r.pread_batch_ptr(offs, args.read_chunk, pbuf.ptr,
                                          args.read_chunk)
                        if cap is not None:
                            cap.take(i, pos, pbuf.view)
                        pos += args.read_chunk * depth
                        total[t] += args.read_chunk * depth
                        continue
                    want = min(args.read_chunk, r.length - pos)
                    if pbuf is not None:
                        n = r.pread_into_ptr(pos, pbuf.ptr, want)
                    else:
                        n = r.pread_into(pos, buf, 0, want)
                    if n <= 0:
                        break
                    if cap is not None:
                        cap.take(i, pos, (pbuf.view if pbuf is not None
                                          else memoryview(buf))[:n])
                    pos += n
                    total[t] += n
            if pbuf is not None:
                pbuf.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(nthreads)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for r in readers:
        r.close()
    if errs:
        raise errs[0]
    got = sum(total)
    expect = args.files * args.file_size
    if got != expect:
        raise RuntimeError(f"step read {got} != {expect}")
    return got


def step_client_seqwrite(args, rank, rt) -> int:
    """Sequential writes via the client path: one concurrent writer per
    file (short-circuit into the in-process worker's arena), overwrite
    per step so capacity stays bounded.  Metric = ingest GiB/s (the
    reference's fio write suite analog, build/tests/fio-test.sh)."""
    async def run():
        import numpy as np
        base = np.random.default_rng(4321 + rank).integers(
            0, 256, size=args.read_chunk, dtype=np.uint8).tobytes()

        async def write_file(i):
            w = await rt.fs.create(f"/bench/r{rank}/w{i}", overwrite=True,
                                   storage_tier="HBM")
            pos = 0
            while pos < args.file_size:
                n = min(args.read_chunk, args.file_size - pos)
                await w.write(base if n == len(base) else base[:n])
                pos += n
            await w.complete()
            return pos
        totals = await asyncio.gather(
            *(write_file(i) for i in range(args.files)))
        return sum(totals)
    return rt.call(run())


def step_fuse_seqwrite(args, rank, mnt) -> int:
    """T threads, each rewriting its share of files through the kernel
    mount in read_chunk chunks."""
    import numpy as np
    base = np.random.default_rng(4321 + rank).integers(
        0, 256, size=args.read_chunk, dtype=np.uint8).tobytes()
    os.makedirs(f"{mnt}/bench/r{rank}", exist_ok=True)
    paths = [f"{mnt}/bench/r{rank}/w{i}" for i in range(args.files)]
    total = [0] * args.threads
    errs = []

    def worker(t):
        try:
            for i in range(t, len(paths), args.threads):
                with open(paths[i], "wb") as f:
                    pos = 0
                    while pos < args.file_size:
                        n = min(args.read_chunk, args.file_size - pos)
                        f.write(base if n == len(base) else base[:n])
                        pos += n
                total[t] += args.file_size
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ths = [threading.Thread(target=worker, args=(t,))
           for t in range(args.threads)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if errs:
        raise errs[0]
    return sum(total)


def capture_written(args, rank, rt, cap) -> None:
    """seqwrite's output is the files themselves: read the sampled extents
    of what the last timed step wrote back through the client."""
    async def run():
        for i, extents in cap.extents.items():
            r = await rt.fs.open(f"/bench/r{rank}/w{i}")
            try:
                buf = bytearray(cap.want)
                for off, _row in extents:
                    got = 0
                    while got < cap.want:
                        n = await r.pread_into(off + got, buf, got,
                                               cap.want - got)
                        if n <= 0:
                            break
                        got += n
                    cap.take(i, off, memoryview(buf)[:got])
            finally:
                r.close()
    rt.call(run())


def run_scale_sweep(args, rank, world, dist, torch, rt, has_gpu,
                    one_step, barrier_sync):
    """one command produces the 1/2/4/8 weak-scaling
    curve (rank subgroups re-run the timed step; idle ranks wait at the
    global barrier) AND an RCCL BlockDistributor.broadcast_file number,
    written to profiles/scale_sweep_n<world>.json by rank 0.  At world=1
    this is the pre-flight: the same code path, degenerate collectives."""
    out = {"world": world, "workload": args.workload, "path": args.path,
           "tier": "HBM" if has_gpu else "MEM(cpu)", "per_n": {}}
    ns = [n for n in (1, 2, 4, 8) if n <= world]
    groups = {}
    for n in ns:
        # new_group is collective: every rank participates in creation
        groups[n] = (dist.new_group(ranks=list(range(n)))
                     if dist is not None and n < world else None)
    for n in ns:
        g = groups[n]
        if rank < n:
            if dist is not None:
                dist.barrier(group=g) if g is not None else dist.barrier()
            if has_gpu:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            bps = 0
            for _ in range(args.steps):
                bps = one_step()
            if has_gpu:
                torch.cuda.synchronize()
            elapsed = time.perf_counter() - t0
            if dist is not None and n > 1:
                t = torch.tensor([elapsed], dtype=torch.float64)
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=g)
                elapsed = t.item()
            if rank == 0:
                total = bps * args.steps * n
                out["per_n"][str(n)] = {
                    "GiBps": round(total / elapsed / (1 << 30), 3),
                    "ms_per_step": round(elapsed / args.steps * 1000, 2),
                    "bytes_per_rank_step": bps,
                }
        if dist is not None:
            dist.barrier()
    # ---- RCCL broadcast_file (xGMI on GPUs, gloo on CPU) ----
    if rt.worker is not None:
        try:
            from curvine_amd.parallel.distributor import BlockDistributor
            local_rank = int(os.environ.get("LOCAL_RANK", rank))
            if dist is None:
                import torch.distributed as dist_mod
                if not dist_mod.is_initialized():
                    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                    os.environ.setdefault("MASTER_PORT", "29571")
                    dist_mod.init_process_group(
                        "nccl" if has_gpu else "gloo", rank=0, world_size=1)
            bd = BlockDistributor(device=local_rank if has_gpu else None)
            path = "/bench/r0/f0"

            def open_file(p):
                return rt.call(rt.fs.client.open(p))

            barrier_sync()
            t0 = time.perf_counter()
            sizes = bd.broadcast_file(open_file, rt.worker.store, path, 0)
            barrier_sync()
            dt = time.perf_counter() - t0
            moved = sum(sizes.values())
            if rank == 0:
                out["broadcast_file"] = {
                    "bytes": moved, "seconds": round(dt, 4),
                    "GiBps_algo": round(moved / dt / (1 << 30), 3),
                    "GiBps_bus": round(moved * max(1, world - 1) / dt
                                       / (1 << 30), 3),
                    "backend": "nccl(RCCL)" if has_gpu else "gloo",
                    "blocks": len(sizes),
                }
        except Exception as e:  # noqa: BLE001 — sweep is best-effort
            if rank == 0:
                out["broadcast_file"] = {"error": str(e)}
    if rank == 0:
        os.makedirs("profiles", exist_ok=True)
        dest = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                            "profiles", f"scale_sweep_n{world}.json")
        with open(dest, "w") as f:
            json.dump(out, f)
        print("SCALE_SWEEP " + json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--path", choices=["fuse", "client"], default="fuse")
    p.add_argument("--workload",
                   choices=["seqread", "randread4k", "seqwrite"],
                   default="seqread")
    p.add_argument("--files", type=int, default=16)
    p.add_argument("--file-size", type=int, default=1 << 30)
    p.add_argument("--block-size", type=int, default=256 << 20)
    p.add_argument("--read-chunk", type=int, default=4 << 20)
    p.add_argument("--threads", type=int, default=32)
    p.add_argument("--rand-reads", type=int, default=200_000)
    p.add_argument("--iodepth", type=int, default=64,
                   help="queue depth per thread for randread4k (fio iodepth)")
    p.add_argument("--seq-batch", type=int, default=1,
                   help="chunks per sync in seqread (DMA pipelining depth)")
    p.add_argument("--separate-worker", action="store_true",
                   help="worker in its own process with short-circuit ON "
                        "(hipIpc cross-process arena mapping)")
    p.add_argument("--no-short-circuit", action="store_true",
                   help="force the streaming worker-RPC read path")
    p.add_argument("--hbm-gb", type=int, default=32)
    p.add_argument("--staging-bytes", type=int, default=8 << 20)
    p.add_argument("--staging-count", type=int, default=8)
    p.add_argument("--fuse-channels", type=int, default=8)
    p.add_argument("--scale-sweep", action="store_true",
                   help="after the main measurement, run the 1/2/4/8 "
                        "weak-scaling curve over rank subgroups plus a "
                        "BlockDistributor.broadcast_file xGMI benchmark, "
                        "writing profiles/scale_sweep_n<world>.json")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write a fixed seeded "
                        "sample of the bytes the last timed step delivered "
                        "to DIR/<workload>_r<rank>.npy (float32)")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements and checks; "
                        "a plain run only sets up, warms up, times --steps "
                        "steps and prints the result line (today every "
                        "secondary measurement already sits behind a "
                        "switch of its own, e.g. --scale-sweep)")
    args = p.parse_args()
    if args.dump_outputs and args.steps < 1:
        p.error("--dump-outputs needs at least one timed step")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))

    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group(
            "nccl" if torch.cuda.is_available() else "gloo")
        if torch.cuda.is_available():
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)))
    has_gpu = torch.cuda.is_available()

    if args.path == "fuse" and not os.path.exists("/dev/fuse") \
            and os.geteuid() == 0:
        # GPU pool boxes ship without the device node; create it (char 10:229)
        try:
            os.mknod("/dev/fuse", 0o666 | 0o020000, os.makedev(10, 229))
            log(rank, "created /dev/fuse")
        except OSError as e:
            log(rank, f"mknod /dev/fuse failed: {e}")
    if args.path == "fuse":
        ok = False
        if os.path.exists("/dev/fuse") and os.geteuid() == 0:
            try:  # probe a real mount: the node may exist without the module
                from curvine_amd.fuse.session import mount_fuse, umount
                probe = f"/tmp/curvine-fuse-probe-{os.getpid()}"
                fd = mount_fuse(probe)
                umount(probe)
                os.close(fd)
                ok = True
            except OSError as e:
                log(rank, f"fuse probe failed: {e}")
        if not ok:
            log(rank, "FUSE unavailable; falling back to client path")
            args.path = "client"
    if not has_gpu and args.file_size > 64 << 20:
        args.files, args.file_size = 4, 32 << 20   # CPU plumbing scale
        args.hbm_gb = 2
        args.rand_reads = 20_000
        # a writer reserves a whole block per open block: size blocks to
        # the plumbing-scale files so reserves match the data
        args.block_size = min(args.block_size, args.file_size)

    def barrier_sync():
        if dist is not None:
            dist.barrier()
        if has_gpu:
            torch.cuda.synchronize()

    rt, conf, daemon_proc, mnt = setup(args, rank, world, dist, has_gpu)
    try:
        _run_bench(args, rank, world, dist, torch, rt, mnt, has_gpu,
                   barrier_sync)
    finally:
        # a failed step must not strand the worker/daemon subprocess
        # (a stranded fixed-port worker breaks the NEXT bench run)
        if daemon_proc is not None:
            daemon_proc.terminate()
            try:
                daemon_proc.wait(timeout=10)
            except subprocess.TimeoutExpired:
                daemon_proc.kill()
        async def teardown():
            if rt.fs:
                await rt.fs.close()
            if rt.worker:
                await rt.worker.stop()
            if rt.master:
                await rt.master.stop()
        try:
            rt.call(teardown())
        except Exception:  # noqa: BLE001 — best-effort teardown
            pass
        rt.stop()
        if dist is not None:
            dist.destroy_process_group()


def _run_bench(args, rank, world, dist, torch, rt, mnt, has_gpu,
               barrier_sync):
    log(rank, f"cluster up ({args.path}); writing "
        f"{args.files}x{args.file_size >> 20}MiB")
    if args.workload != "seqwrite":   # writing IS the seqwrite workload
        t0 = time.perf_counter()
        write_dataset(args, rank, rt, mnt)
        log(rank, f"dataset written in {time.perf_counter() - t0:.1f}s")

    lat_out: list = []

    def one_step(cap=None):
        if args.workload == "seqwrite":
            if args.path == "fuse":
                return step_fuse_seqwrite(args, rank, mnt)
            return step_client_seqwrite(args, rank, rt)
        if args.workload == "randread4k":
            if args.path != "fuse":
                return step_client_rand4k(args, rank, rt, lat_out, cap)
            return step_fuse_rand4k(args, rank, mnt, lat_out, cap)
        if args.path == "fuse":
            return step_fuse_seq(args, rank, mnt, cap)
        if args.no_short_circuit:
            return step_client_seq_remote(args, rank, rt, cap=cap)
        return step_client_seq(args, rank, rt, cap)

    cap = OutputCapture(args, rank) if args.dump_outputs else None
    for _ in range(args.warmup):
        one_step()
    barrier_sync()
    t_start = time.perf_counter()
    bytes_per_step = 0
    for s in range(args.steps):
        # the read workloads copy their sampled extents in the last step
        bytes_per_step = one_step(cap if s == args.steps - 1 else None)
    barrier_sync()
    elapsed = time.perf_counter() - t_start

    if cap is not None:
        if args.workload == "seqwrite":
            capture_written(args, rank, rt, cap)
        log(rank, f"outputs written to {cap.save(args.dump_outputs, rank)}")

    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    total_bytes = bytes_per_step * args.steps * world
    gibps = total_bytes / elapsed / (1 << 30)

    if rank == 0:
        if args.workload == "randread4k":
            iops = (total_bytes / 4096) / elapsed
            metric = (f"{args.path}_rand_read_4k_IOPS")
            value, unit = round(iops, 1), "IOPS"
            # the reference publishes no 4 KiB IOPS figure (only 256 KiB
            # random GiB/s and a ~100 µs latency class) — no ratio to quote
            vs = None
        elif args.workload == "seqwrite":
            metric = ("fuse_seq_write_GiBps" if args.path == "fuse"
                      else "cached_seq_write_GiBps")
            value, unit = round(gibps, 3), "GiB/s"
            vs = None   # the reference publishes no write GiB/s figure
        else:
            metric = ("fuse_seq_read_GiBps" if args.path == "fuse"
                      else "cached_seq_read_GiBps")
            value, unit = round(gibps, 3), "GiB/s"
            vs = round(gibps / REFERENCE_PEAK_GIBPS, 3)
        result = {
            "metric": metric,
            "value": value,
            "unit": unit,
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": vs,
            "dtype": "bytes",
            "data": "synthetic random-byte files (numpy PRNG), cached in "
                    + ("HBM tier" if has_gpu else "MEM tier (cpu plumbing)"),
            "config": {
                "model": "curvine-amd cache engine",
                "workload": args.workload,
                "path": args.path,
                "tier": "HBM" if has_gpu else "MEM(cpu)",
                "files_per_rank": args.files,
                "file_size": args.file_size,
                "read_chunk": args.read_chunk,
                "threads": args.threads,
                "iodepth": args.iodepth,
                "block_size": args.block_size,
                "fuse_channels": args.fuse_channels,
                "short_circuit": not args.no_short_circuit,
                "GiBps": round(gibps, 3),
                "latency": lat_out[-1] if lat_out else None,
                "parallelism": f"shard-per-gpu x{world}",
            },
        }
        print(json.dumps(result), flush=True)

    if args.scale_sweep:
        run_scale_sweep(args, rank, world, dist, torch, rt, has_gpu,
                        one_step, barrier_sync)



if __name__ == "__main__":
    main()
