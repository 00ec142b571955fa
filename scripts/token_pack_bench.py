#!/usr/bin/env python3
"""Document-packed token batches from an HBM-tier token file:
CurvinePackedTokenLoader (one token_pack_kernel launch per batch writes x,
masked y, position_ids, doc_ids and cu_seqlens) against two routes the
project offered before it, in the same process:

    (a) resolve_gather / exec_gather of the same source spans into a uint8
        cuda tensor, then torch on the GPU building the same five tensors
        from the bytes and a small per-segment table uploaded per batch
        (repeat_interleave, index, where, cat);
    (b) CurvineTokenLoader with all `documents` at the same shape: context
        only, its batches are windows, not packed documents.

Plans and tables are made outside the timed region for all routes; the
routes alternate batch by batch; every timed batch ends in a device
synchronise.  The first batch of (a) is compared with the packed batch for
equality.  Also times the one-time document index, reader.token_eos_index
of one file, against pread of the file + numpy.flatnonzero, and reports the
packing efficiency of the corpus.  The files carry the eos id at about one
token in 500.  Needs a GPU: without one it stops, unless --rehearse asks
for a tiny host-memory walk through the same code that measures nothing.

    python scripts/token_pack_bench.py [--out profiles/token_pack.json]
"""
import argparse
import json
import os
import statistics as st
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("U16", 8), ("U16", 64), ("U32", 64)]
EOS = 1
EOS_EVERY = 500
DOCS = ("position_ids", "doc_ids", "cu_seqlens")
PAD, NEXT = 2, 1


def stats(ts):
    return {"mean_us": round(st.mean(ts) * 1e6, 2),
            "stdev_us": round(st.stdev(ts) * 1e6, 2) if len(ts) > 1 else None,
            "min_us": round(min(ts) * 1e6, 2),
            "batches_us": [round(t * 1e6, 1) for t in ts]}


def gather_plan(torch, ld, reader, b, item, on_dev):
    """Route (a)'s plan of batch b: the gather of every source segment's
    n (+1) tokens, back to back, and the per-segment table."""
    order, batches = ld._pack()
    segments, sources = batches[b]
    samples, table, at = [], [], 0
    for seg, src in zip(segments, sources):
        row, col, n, pos0, doc, _seq, flags = seg
        if src is None:
            table.append((n, 1, 0, 0, -1, 0))
            continue
        _ridx, start, _len = ld._docs[order[src[0]]]
        tok = n + (flags & NEXT)
        samples.append((ld.header_bytes + (start + src[1]) * item, tok * item,
                        at * item))
        table.append((n, 0, flags & NEXT, pos0, doc, at))
        at += tok
    groups, slow, total = reader.resolve_gather(samples, on_dev)
    assert total == at * item
    return groups, slow, at * item, torch.tensor(table, dtype=torch.int64)


def torch_pack(torch, raw, table, src, B, T, pad_id, ignore):
    """The five tensors of a packed batch as a chain of torch ops."""
    dev = raw.device
    dt = {"U16": torch.uint16, "U32": torch.uint32}[src]
    try:
        w = raw.view(dt).to(torch.int64)
    except (RuntimeError, TypeError):
        sdt, mask = {"U16": (torch.int16, 0xFFFF),
                     "U32": (torch.int32, 0xFFFFFFFF)}[src]
        w = raw.view(sdt).to(torch.int64) & mask
    t = table.to(dev, non_blocking=True)
    n, is_pad, nxt, pos0, doc, src0 = t.unbind(1)
    starts = torch.cumsum(n, 0) - n
    seg = torch.repeat_interleave(torch.arange(len(n), device=dev), n,
                                  output_size=B * T)
    within = torch.arange(B * T, device=dev) - starts[seg]
    padm = is_pad[seg].bool()
    at = (src0[seg] + within).clamp_(0, max(len(w) - 1, 0))
    x = torch.where(padm, pad_id, w[at])
    end = (within == n[seg] - 1) & ~nxt[seg].bool()
    y = torch.where(padm | end, ignore, w[(at + 1).clamp_(max=len(w) - 1)])
    pos = torch.where(padm, within, pos0[seg] + within)
    dd = torch.where(padm, -1, doc[seg])
    cu = torch.cat([starts, starts.new_tensor([B * T])]).to(torch.int32)
    return (x.view(B, T), y.view(B, T),
            {"position_ids": pos.view(B, T), "doc_ids": dd.view(B, T),
             "cu_seqlens": cu})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--file-mb", type=int, default=1024)
    p.add_argument("--seq-len", type=int, default=4096)
    p.add_argument("--batches", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default="profiles/token_pack.json")
    p.add_argument("--rehearse", action="store_true",
                   help="tiny MEM-tier run on the CPU; writes no profile")
    args = p.parse_args()

    import numpy as np
    import torch

    from curvine_amd import native
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.client.reader import SyncLocalReader
    from curvine_amd.sdk import CurvinePackedTokenLoader, CurvineTokenLoader
    from curvine_amd.testing import SyncMiniCluster, test_conf

    has_gpu = native.gpu_available()
    if not has_gpu and not args.rehearse:
        sys.exit("token_pack_bench: no GPU visible (use --rehearse to walk "
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

    tmp = tempfile.mkdtemp(prefix="token-pack-bench-")
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
        toks[toks == EOS] = EOS + 1
        toks[rng.integers(0, EOS_EVERY, n) == 0] = EOS
        paths[src] = f"/tokens/{src}.bin"
        sf.write_file(paths[src], toks.tobytes(), storage_tier=tier)
        del toks
        print(f"wrote {paths[src]}", flush=True)

    # ---- the one-time index
    index = []
    for src in ("U16", "U32"):
        item = native.DTYPE_ITEMSIZE[src]
        r = SyncLocalReader(sf.call(sf.fs.client.open(paths[src])))
        dev_t, host_t = [], []
        for k in range(4):
            sync()
            t0 = time.perf_counter()
            got = r.token_eos_index(src, 0, EOS, on_dev)
            t1 = time.perf_counter()
            raw = r.pread(0, r.length)
            ref = np.flatnonzero(np.frombuffer(raw, np_dt[src]) == EOS)
            t2 = time.perf_counter()
            if k == 0:
                assert np.array_equal(np.frombuffer(got, np.int64), ref), \
                    "the two indices disagree"
            else:                           # the first round warms both up
                dev_t.append(t1 - t0)
                host_t.append(t2 - t1)
            del raw
        r.close()
        index.append({
            "src_dtype": src, "tokens": r.length // item, "eos": len(ref),
            "token_eos_index_ms": [round(t * 1e3, 2) for t in dev_t],
            "pread_flatnonzero_ms": [round(t * 1e3, 2) for t in host_t],
            "indices_equal": True})
        print(json.dumps(index[-1]), flush=True)

    # ---- the per-batch path
    results = []
    for src, B in SHAPES:
        item = native.DTYPE_ITEMSIZE[src]
        t0 = time.perf_counter()
        ld = CurvinePackedTokenLoader(cconf, [paths[src]], T, B, EOS,
                                      device=device, src_dtype=src,
                                      outputs=DOCS, shuffle=True, seed=1)
        build_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        n_batches = min(len(ld), args.warmup + args.batches)
        pack_s = time.perf_counter() - t0
        win = CurvineTokenLoader(cconf, [paths[src]], T, B, device=device,
                                 src_dtype=src, shuffle=True, seed=1,
                                 eos_id=EOS, documents=DOCS)
        reader = ld._readers[0]
        plans = [gather_plan(torch, ld, reader, b, item, on_dev)
                 for b in range(n_batches)]
        it = iter(ld)
        for _ in range(n_batches):          # resolves the timed batches' plans
            next(it)
        it, it_w = iter(ld), iter(win)
        first_w = next(it_w)
        new_t, old_t, win_t = [], [], []
        for b in range(n_batches):
            sync()
            t0 = time.perf_counter()
            x, y, docs = next(it)
            sync()
            t1 = time.perf_counter()
            groups, slow, nbytes, table = plans[b]
            raw = torch.empty(nbytes, dtype=torch.uint8, device=device)
            reader.exec_gather(groups, slow, raw.data_ptr())
            px, py, pd = torch_pack(torch, raw, table, src, B, T, ld.pad_id,
                                    ld.ignore_index)
            sync()
            t2 = time.perf_counter()
            _w = first_w if b == 0 else next(it_w)
            sync()
            t3 = time.perf_counter()
            if b == 0:
                assert torch.equal(x, px) and torch.equal(y, py) and \
                    all(torch.equal(docs[k], pd[k]) for k in DOCS), \
                    "the two routes disagree"
            if b >= args.warmup:
                new_t.append(t1 - t0)
                old_t.append(t2 - t1)
                win_t.append(t3 - t2)
        results.append({
            "src_dtype": src, "out_dtype": "I64", "seq_len": T, "batch": B,
            "eos_every": EOS_EVERY, "documents": ld.num_documents,
            "batches_per_epoch": len(ld),
            "pack_efficiency": round(ld.pack_efficiency, 5),
            "timed_batches": len(new_t), "warmup_batches": args.warmup,
            "packed_loader": stats(new_t),
            "gather_then_torch": stats(old_t),
            "window_loader_with_documents": stats(win_t),
            "setup_s": {"index_and_documents": round(build_s, 3),
                        "pack_segments": round(pack_s, 3)},
            "outputs_equal": True})
        ld.close()
        win.close()
        print(json.dumps(results[-1]), flush=True)

    report = {"bench": "token_pack", "device": device, "tier": tier,
              "file_mb": args.file_mb, "shuffle": True, "eos_id": EOS,
              "timing": "host clock around one batch, device synchronised "
                        "at both ends; routes alternate per batch; "
                        "window_loader_with_documents is context only (its "
                        "batches are windows, not packed documents)",
              "index": index, "results": results}
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
