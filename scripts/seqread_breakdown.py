#!/usr/bin/env python3
"""Where a client sequential-read step spends its wall time.

Runs the benchmark's step shape on its own: T threads, each reading one
"file" of --file-size bytes in --chunk preads into a PinnedBuffer.  The
files are extents of one Arena, each behind its own registered reader;
nothing outside this tree is read.  Two variants:

  fresh  new OS threads and new PinnedBuffers every step (what bench.py does)
  kept   threads and buffers kept across steps

Each step's wall time is split into
  (a) start   step start -> a thread's first copy has returned (mean of threads)
  (b) copy    first copy returned -> last copy returned        (mean of threads)
  (c) close   last copy returned -> close() + join done        (rest of the wall)
so a + b + c is the step's wall time.  fresh minus kept is the churn that
pooling buffers and streams can remove.  One JSON line per variant, then a
summary line; --json FILE also writes them to a file.

  python scripts/seqread_breakdown.py               # 16 x 1 GiB, GPU 0
  python scripts/seqread_breakdown.py --small       # 2 x 8 MiB, host arena
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from curvine_amd import native  # noqa: E402


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--file-size", type=int, default=1 << 30)
    p.add_argument("--chunk", type=int, default=4 << 20)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--device", type=int, default=None,
                   help="arena device; -1 = host (default: 0 with a GPU)")
    p.add_argument("--small", action="store_true",
                   help="2 threads x 8 MiB in 1 MiB chunks: a rehearsal "
                        "that also fits a host arena")
    p.add_argument("--json", default=None, help="also write the result here")
    args = p.parse_args()
    if args.small:
        args.threads, args.file_size, args.chunk = 2, 8 << 20, 1 << 20
    if args.device is None:
        args.device = 0 if native.gpu_available() else -1

    mod = native.load()
    T, size, chunk = args.threads, args.file_size, args.chunk
    arena = native.Arena(args.device, T * size)
    rids = [mod.reader_register([(0, size, arena.handle, t * size)], size)
            for t in range(T)]
    # one ranged read; a build without reader_pread serves it as a batch of 1
    if hasattr(mod, "reader_pread"):
        def pread(rid, off, n, ptr):
            return mod.reader_pread(rid, off, n, ptr)
    else:
        def pread(rid, off, n, ptr):
            assert not mod.reader_pread_batch(rid, [off], n, ptr, n)
            return n

    def read_file(t, pbuf, marks):
        """marks[t] = (first copy returned, last copy returned)."""
        pos, first = 0, None
        while pos < size:
            n = pread(rids[t], pos, min(chunk, size - pos), pbuf.ptr)
            if first is None:
                first = time.perf_counter()
            pos += n
        marks[t] = (first, time.perf_counter())

    def split(t0, t1, marks):
        first = statistics.fmean(m[0] for m in marks)
        last = statistics.fmean(m[1] for m in marks)
        return {"wall_ms": (t1 - t0) * 1e3, "start_ms": (first - t0) * 1e3,
                "copy_ms": (last - first) * 1e3, "close_ms": (t1 - last) * 1e3}

    def step_fresh():
        marks = [None] * T

        def worker(t):
            pbuf = native.PinnedBuffer(chunk)
            read_file(t, pbuf, marks)
            pbuf.close()

        ths = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        t0 = time.perf_counter()
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        return split(t0, time.perf_counter(), marks)

    def run_kept(nsteps):
        marks = [None] * T
        # a worker that dies breaks the barrier instead of hanging the run
        go = threading.Barrier(T + 1, timeout=120)
        done = threading.Barrier(T + 1, timeout=120)

        def worker(t):
            pbuf = native.PinnedBuffer(chunk)
            for _ in range(nsteps):
                go.wait()
                read_file(t, pbuf, marks)
                done.wait()
            pbuf.close()

        ths = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for th in ths:
            th.start()
        out = []
        for _ in range(nsteps):
            t0 = time.perf_counter()
            go.wait()
            done.wait()
            out.append(split(t0, time.perf_counter(), list(marks)))
        for th in ths:
            th.join()
        return out

    def summarise(name, steps):
        steps = steps[args.warmup:]
        row = {"variant": name, "threads": T, "file_size": size,
               "chunk": chunk, "device": args.device, "steps": len(steps)}
        for k in ("wall_ms", "start_ms", "copy_ms", "close_ms"):
            v = [s[k] for s in steps]
            row[k] = {"median": statistics.median(v), "min": min(v),
                      "max": max(v)}
        row["GiBps_median"] = T * size / 2**30 / (row["wall_ms"]["median"] / 1e3)
        print(json.dumps(row), flush=True)
        return row

    n = args.warmup + args.steps
    fresh = summarise("fresh", [step_fresh() for _ in range(n)])
    kept = summarise("kept", run_kept(n))
    churn = fresh["wall_ms"]["median"] - kept["wall_ms"]["median"]
    spread = max(fresh["wall_ms"]["max"] - fresh["wall_ms"]["min"],
                 kept["wall_ms"]["max"] - kept["wall_ms"]["min"])
    result = {"fresh": fresh, "kept": kept,
              "churn_ms_per_step": churn, "spread_ms": spread}
    if hasattr(native, "hip_pool_stats"):
        result["pool_stats"] = native.hip_pool_stats()
    print(json.dumps({"churn_ms_per_step": churn, "spread_ms": spread,
                      "pool_stats": result.get("pool_stats")}), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    for rid in rids:
        mod.reader_unregister(rid)
    arena.close()


if __name__ == "__main__":
    main()
