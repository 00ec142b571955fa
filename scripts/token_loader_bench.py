#!/usr/bin/env python3
"""Token-window batches from an HBM-tier token file: CurvineTokenLoader
(one token_windows_kernel launch per batch) against the route the project
offered before it, in the same process on the same windows:

    resolve_gather / exec_gather of the windows' raw bytes into a uint8
    cuda tensor, then torch on the GPU: reinterpret, widen to int64, and
    the two shifted slices made contiguous.

Plans are resolved outside the timed region for both routes; the two
routes alternate batch by batch; every timed batch ends in a device
synchronise.  The first batch of each shape is compared for equality.
Needs a GPU: without one it stops, unless --rehearse asks for a tiny
host-memory walk through the same code that measures nothing.

    python scripts/token_loader_bench.py [--out profiles/token_loader.json]

With --docs the comparison is the document outputs instead: the loader
yielding (x, y, docs) with position_ids, doc_ids and cu_seqlens (one
native.token_docs call per batch: three launches) against the loader
yielding (x, y) followed by the torch expression for the same three outputs
on the GPU (eq, cumsum, cummax, nonzero, cat, diff, max).  The files carry
the eos id at about one token in 500.  The plain (x, y) batch time of the
same run is recorded beside both.

    python scripts/token_loader_bench.py --docs [--out profiles/token_docs.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("U16", 8), ("U16", 64), ("U32", 64)]
EOS = 1                                     # --docs: the end-of-document id
EOS_EVERY = 500
DOCS = ("position_ids", "doc_ids", "cu_seqlens")


def torch_docs(torch, x, eos):
    """The three document outputs of x as a chain of torch ops."""
    rows, T = x.shape
    is_eos = x == eos
    ind = is_eos.to(x.dtype)
    doc = torch.cumsum(ind, 1) - ind
    shifted = torch.zeros_like(is_eos)
    shifted[:, 1:] = is_eos[:, :-1]
    col = torch.arange(T, dtype=x.dtype, device=x.device).expand(rows, T)
    start = torch.cummax(torch.where(shifted, col, 0), 1).values
    pos = col - start
    shifted[:, 0] = True
    starts = torch.nonzero(shifted.view(-1)).view(-1)
    end = torch.tensor([rows * T], dtype=starts.dtype, device=x.device)
    cu = torch.cat([starts, end]).to(torch.int32)
    return {"position_ids": pos, "doc_ids": doc, "cu_seqlens": cu,
            "max_seqlen": int(torch.diff(cu).max())}


def bench_docs(args, torch, CurvineTokenLoader, cconf, paths, device, sync):
    """Per shape: (x, y, docs) from the loader against (x, y) from the
    loader + torch_docs, alternating batch by batch."""
    import statistics as st
    T = args.seq_len
    results = []
    for src, B in SHAPES:
        kw = dict(device=device, src_dtype=src, shuffle=True, seed=1)
        fused = CurvineTokenLoader(cconf, [paths[src]], T, B, eos_id=EOS,
                                   documents=DOCS, **kw)
        plain = CurvineTokenLoader(cconf, [paths[src]], T, B, **kw)
        n_batches = min(len(fused), args.warmup + args.batches)
        it_f, it_p = iter(fused), iter(plain)
        first_f, first_p = next(it_f), next(it_p)   # resolves the plans
        fused_t, plain_t, torch_t = [], [], []
        for b in range(n_batches):
            sync()
            t0 = time.perf_counter()
            x, y, docs = first_f if b == 0 else next(it_f)
            sync()
            t1 = time.perf_counter()
            px, py = first_p if b == 0 else next(it_p)
            sync()
            t2 = time.perf_counter()
            ref = torch_docs(torch, px, EOS)
            sync()
            t3 = time.perf_counter()
            if b == 0:
                assert torch.equal(x, px) and torch.equal(y, py)
                assert all(torch.equal(docs[k], ref[k]) for k in DOCS) and \
                    docs["max_seqlen"] == ref["max_seqlen"], \
                    "the two routes disagree"
                n_seqs = len(ref["cu_seqlens"]) - 1
            if b >= args.warmup:
                fused_t.append(t1 - t0)
                plain_t.append(t2 - t1)
                torch_t.append(t3 - t1)
        fused.close()
        plain.close()

        def stats(ts):
            return {"mean_us": round(st.mean(ts) * 1e6, 2),
                    "stdev_us": round(st.stdev(ts) * 1e6, 2)
                    if len(ts) > 1 else None,
                    "min_us": round(min(ts) * 1e6, 2),
                    "batches_us": [round(t * 1e6, 1) for t in ts]}
        results.append({
            "src_dtype": src, "out_dtype": "I64", "seq_len": T, "batch": B,
            "eos_every": EOS_EVERY, "n_seqs_first_batch": n_seqs,
            "timed_batches": len(fused_t), "warmup_batches": args.warmup,
            "loader_with_documents": stats(fused_t),
            "loader_then_torch": stats(torch_t),
            "loader_plain_xy": stats(plain_t),
            "outputs_equal": True})
        print(json.dumps(results[-1]), flush=True)
    return results


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--file-mb", type=int, default=1024)
    p.add_argument("--seq-len", type=int, default=4096)
    p.add_argument("--batches", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--docs", action="store_true",
                   help="time the document outputs against torch ops")
    p.add_argument("--rehearse", action="store_true",
                   help="tiny MEM-tier run on the CPU; writes no profile")
    args = p.parse_args()
    if args.out is None:
        args.out = "profiles/token_docs.json" if args.docs \
            else "profiles/token_loader.json"

    import numpy as np
    import torch

    from curvine_amd import native
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineTokenLoader
    from curvine_amd.testing import SyncMiniCluster, test_conf

    has_gpu = native.gpu_available()
    if not has_gpu and not args.rehearse:
        sys.exit("token_loader_bench: no GPU visible (use --rehearse to walk "
                 "the code on the CPU)")
    if args.rehearse:
        args.file_mb, args.seq_len = 2, 256
    device = "cuda:0" if has_gpu and not args.rehearse else "cpu"
    on_dev = device != "cpu"
    tier = "HBM" if on_dev else "MEM"
    T = args.seq_len

    def sync():
        if on_dev:
            torch.cuda.synchronize()

    tmp = tempfile.mkdtemp(prefix="token-bench-")
    conf = test_conf(tmp)
    block = (256 << 20) if on_dev else (1 << 20)
    conf.master.block_size = block
    conf.client.block_size = block
    room = 2 * args.file_mb // 1024 + 2
    smc = SyncMiniCluster(
        conf=conf, tmp_dir=tmp,
        worker_dirs=[[f"[HBM:{room}GB:0]gpu0" if on_dev
                      else f"[MEM:64MB]{tmp}/mem"]]).start()
    cconf = smc.client_conf()
    sf = SyncFs(cconf)
    sf.fs.client.local_worker_id = smc.workers[0].worker_id

    rng = np.random.default_rng(0)
    vocab = {"U16": 50257, "U32": 128256}
    np_dt = {"U16": np.uint16, "U32": np.uint32}
    paths = {}
    for src in ("U16", "U32"):
        n = (args.file_mb << 20) // np.dtype(np_dt[src]).itemsize
        toks = rng.integers(0, vocab[src], n, dtype=np_dt[src])
        if args.docs:
            toks[toks == EOS] = EOS + 1
            toks[rng.integers(0, EOS_EVERY, n) == 0] = EOS
        paths[src] = f"/tokens/{src}.bin"
        sf.write_file(paths[src], toks.tobytes(), storage_tier=tier)
        del toks

    # the cheapest widen torch offers here: a direct unsigned -> int64 cast
    # where this torch has one on the device, else signed cast + mask
    try:
        torch.zeros(8, dtype=torch.uint8, device=device).view(
            torch.uint16).to(torch.int64)
        torch.zeros(8, dtype=torch.uint8, device=device).view(
            torch.uint32).to(torch.int64)
        unsigned_cast = True
    except (RuntimeError, AttributeError, TypeError):
        unsigned_cast = False

    def parent_widen(raw, src, rows):
        """reinterpret + widen + two contiguous slices, in torch"""
        if unsigned_cast:
            dt = torch.uint16 if src == "U16" else torch.uint32
            w = raw.view(dt).view(rows, T + 1).to(torch.int64)
        elif src == "U16":
            w = raw.view(torch.int16).view(rows, T + 1).to(torch.int64) & 0xFFFF
        else:
            w = raw.view(torch.int32).view(rows, T + 1).to(torch.int64) \
                & 0xFFFFFFFF
        return w[:, :-1].contiguous(), w[:, 1:].contiguous()

    results = bench_docs(args, torch, CurvineTokenLoader, cconf, paths,
                         device, sync) if args.docs else []
    for src, B in ([] if args.docs else SHAPES):
        item = native.DTYPE_ITEMSIZE[src]
        ld = CurvineTokenLoader(cconf, [paths[src]], T, B, device=device,
                                src_dtype=src, shuffle=True, seed=1)
        n_batches = min(len(ld), args.warmup + args.batches)
        reader = ld._readers[0]
        order = ld._order()
        wbytes = (T + 1) * item
        t0 = time.perf_counter()
        parent_plans = []
        for b in range(n_batches):
            samples = [(ld._windows[w][1], wbytes, row * wbytes)
                       for row, w in enumerate(order[b * B:(b + 1) * B])]
            groups, slow, total = reader.resolve_gather(samples, on_dev)
            assert total == B * wbytes
            parent_plans.append((groups, slow))
        parent_plan_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        it = iter(ld)
        first = next(it)                    # resolves every batch plan
        new_plan_s = time.perf_counter() - t0

        new_t, old_t = [], []
        for b in range(n_batches):
            sync()
            t0 = time.perf_counter()
            x, y = first if b == 0 else next(it)
            sync()
            t1 = time.perf_counter()
            groups, slow = parent_plans[b]
            raw = torch.empty(B * wbytes, dtype=torch.uint8, device=device)
            reader.exec_gather(groups, slow, raw.data_ptr())
            px, py = parent_widen(raw, src, B)
            sync()
            t2 = time.perf_counter()
            if b == 0:
                assert torch.equal(x, px) and torch.equal(y, py), \
                    "the two routes disagree"
            if b >= args.warmup:
                new_t.append(t1 - t0)
                old_t.append(t2 - t1)
        ld.close()
        out_bytes = 2 * B * T * 8

        def stats(ts):
            m = statistics.mean(ts)
            return {"mean_us": round(m * 1e6, 2),
                    "stdev_us": round(statistics.stdev(ts) * 1e6, 2)
                    if len(ts) > 1 else None,
                    "min_us": round(min(ts) * 1e6, 2),
                    "written_GBps": round(out_bytes / m / 1e9, 3),
                    "batches_us": [round(t * 1e6, 1) for t in ts]}
        results.append({
            "src_dtype": src, "out_dtype": "I64", "seq_len": T, "batch": B,
            "bytes_written_per_batch": out_bytes,
            "timed_batches": len(new_t), "warmup_batches": args.warmup,
            "token_loader": stats(new_t),
            "gather_then_torch": stats(old_t),
            "plan_s": {"token_loader_all_batches": round(new_plan_s, 3),
                       "gather_timed_batches": round(parent_plan_s, 3)},
            "outputs_equal": True})
        print(json.dumps(results[-1]), flush=True)

    report = {"bench": "token_loader", "device": device, "tier": tier,
              "file_mb": args.file_mb, "shuffle": True,
              "timing": "host clock around one batch, device synchronised "
                        "at both ends; routes alternate per batch",
              "parent_widen": "unsigned cast" if unsigned_cast
              else "signed cast + mask", "results": results}
    if args.docs:
        del report["parent_widen"]
        report.update(
            bench="token_docs", eos_id=EOS,
            timing="host clock around one batch, device synchronised at "
                   "both ends; routes alternate per batch; "
                   "loader_then_torch includes its loader_plain_xy batch")
    sf.shutdown()
    smc.stop()
    if args.rehearse:
        print("rehearsal only: nothing measured, no profile written")
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
