#!/usr/bin/env python3
"""Image batches from HBM-tier .npy files: CurvineArrayLoader (one
array_samples_kernel launch per batch) against the route the project
offered before it, in the same process on the same samples:

    resolve_gather / exec_gather of the samples' raw bytes into a uint8
    cuda tensor, then torch on the GPU: view as [B, H, W, C], per-sample
    crop and flip (stacked), permute to NCHW, .float() * scale + bias,
    .to(dtype), contiguous.  With the full frame and no flip the torch
    route needs no per-sample loop.

Plans are resolved outside the timed region for both routes; both routes
run their warm-up batches first; then the two alternate batch by batch and
every timed batch ends in a device synchronise.  The first batch of each
shape is compared for equality.  `array_samples_call` is the host clock
around the replayed exec_array_samples call alone (table upload, one launch,
stream synchronise) on a destination that already exists: the loader's batch
time without torch.empty and the iterator.  The arena's kernel stream is the
module's own, so no event of this script can bracket the kernel by itself.
Needs a GPU: without one it stops, unless --rehearse asks for a tiny
host-memory walk through the same code that measures nothing.

    python scripts/array_loader_bench.py [--out profiles/array_loader.json]
"""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
# (file, batch, crop, random crop + flip, out dtype)
CASES = [("big", 64, 224, True, "BF16"), ("big", 256, 224, True, "BF16"),
         ("big", 256, 224, True, "F32"), ("big", 256, None, False, "BF16"),
         ("small", 1024, None, False, "BF16")]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--file-mb", type=int, default=1024)
    p.add_argument("--small-mb", type=int, default=96)
    p.add_argument("--batches", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default="profiles/array_loader.json")
    p.add_argument("--rehearse", action="store_true",
                   help="tiny MEM-tier run on the CPU; writes no profile")
    args = p.parse_args()

    import numpy as np
    import torch

    from curvine_amd import native
    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineArrayLoader
    from curvine_amd.testing import SyncMiniCluster, test_conf

    has_gpu = native.gpu_available()
    if not has_gpu and not args.rehearse:
        sys.exit("array_loader_bench: no GPU visible (use --rehearse to walk "
                 "the code on the CPU)")
    shapes = {"big": (256, 256, 3), "small": (32, 32, 3)}
    cases = CASES
    if args.rehearse:
        args.file_mb, args.small_mb, args.batches, args.warmup = 2, 1, 2, 1
        shapes["big"] = (64, 64, 3)
        cases = [(f, max(2, b // 64), 56 if c else None, r, d)
                 for f, b, c, r, d in CASES]
    device = "cuda:0" if has_gpu and not args.rehearse else "cpu"
    on_dev = device != "cpu"
    tier = "HBM" if on_dev else "MEM"
    tdt = {"BF16": torch.bfloat16, "F32": torch.float32}

    def sync():
        if on_dev:
            torch.cuda.synchronize()

    tmp = tempfile.mkdtemp(prefix="array-bench-")
    conf = test_conf(tmp)
    block = (256 << 20) if on_dev else (1 << 20)
    conf.master.block_size = block
    conf.client.block_size = block
    room = 2 * (args.file_mb + args.small_mb) // 1024 + 2
    smc = SyncMiniCluster(
        conf=conf, tmp_dir=tmp,
        worker_dirs=[[f"[HBM:{room}GB:0]gpu0" if on_dev
                      else f"[MEM:64MB]{tmp}/mem"]]).start()
    cconf = smc.client_conf()
    sf = SyncFs(cconf)
    sf.fs.client.local_worker_id = smc.workers[0].worker_id

    rng = np.random.default_rng(0)
    paths, counts = {}, {}
    for name, mb in (("big", args.file_mb), ("small", args.small_mb)):
        H, W, C = shapes[name]
        n = (mb << 20) // (H * W * C)
        f = io.BytesIO()
        np.lib.format.write_array(
            f, rng.integers(0, 256, (n, H, W, C), dtype=np.uint8),
            version=(1, 0))
        paths[name], counts[name] = f"/arrays/{name}.npy", n
        sf.write_file(paths[name], f.getvalue(), storage_tier=tier)
        del f

    results = []
    for name, B, crop, rand, dst in cases:
        H, W, C = shapes[name]
        ld = CurvineArrayLoader(cconf, [paths[name]], B, device=device,
                                out_dtype=tdt[dst], crop=crop,
                                random_crop=rand, random_flip=rand, mean=MEAN,
                                std=STD, shuffle=True, seed=1)
        h, w = ld.crop
        n_warm, n_timed = args.warmup, min(args.batches, len(ld))
        reader = ld._readers[0]
        order, aug = ld._order()
        sb = H * W * C
        scale_t = torch.tensor(ld.scale, device=device).view(1, C, 1, 1)
        bias_t = torch.tensor(ld.bias, device=device).view(1, C, 1, 1)
        t0 = time.perf_counter()
        parent_plans = []
        for b in range(n_timed):
            samples = [(ld._samples[i][1], sb, row * sb)
                       for row, i in enumerate(order[b * B:(b + 1) * B])]
            groups, slow, total = reader.resolve_gather(samples, on_dev)
            assert total == B * sb
            parent_plans.append((groups, slow, aug[b * B:(b + 1) * B]))
        parent_plan_s = time.perf_counter() - t0

        def parent(b):
            groups, slow, rows = parent_plans[b]
            raw = torch.empty(B * sb, dtype=torch.uint8, device=device)
            reader.exec_gather(groups, slow, raw.data_ptr())
            v = raw.view(B, H, W, C)
            if rand:
                v = torch.stack([
                    v[i, dy:dy + h, dx:dx + w].flip(1) if flip
                    else v[i, dy:dy + h, dx:dx + w]
                    for i, (dy, dx, flip) in enumerate(rows)])
            v = v.permute(0, 3, 1, 2).float() * scale_t + bias_t
            return v.to(tdt[dst]).contiguous()

        t0 = time.perf_counter()
        it = iter(ld)
        first = next(it)                    # resolves every batch plan
        new_plan_s = time.perf_counter() - t0
        assert torch.equal(first, parent(0)), "the two routes disagree"
        for b in range(1, min(n_warm, n_timed)):
            next(it)
            parent(b)
        sync()

        plans = ld._plans[1]
        new_t, old_t, call_t = [], [], []
        it = iter(ld)                       # the same plans, replayed
        keep = torch.empty((B, C, h, w), dtype=tdt[dst], device=device)
        for b in range(n_timed):
            sync()
            t0 = time.perf_counter()
            x = next(it)
            sync()
            t1 = time.perf_counter()
            px = parent(b)
            sync()
            t2 = time.perf_counter()
            _n, rows, execs = plans[b]
            for rd, groups, slow in execs:
                rd.exec_array_samples(groups, slow, keep.data_ptr(), B, rows,
                                      ld.shape, ld.crop, ld.scale, ld.bias,
                                      ld.dst_dtype, ld.layout, on_dev)
            t3 = time.perf_counter()
            assert x.shape == px.shape
            new_t.append(t1 - t0)
            old_t.append(t2 - t1)
            call_t.append(t3 - t2)
        assert torch.equal(x, px) and torch.equal(keep, px), \
            "the two routes disagree"
        ld.close()
        out_bytes = B * C * h * w * native.DTYPE_ITEMSIZE[dst]

        def stats(ts):
            m = statistics.mean(ts)
            return {"mean_us": round(m * 1e6, 2),
                    "stdev_us": round(statistics.stdev(ts) * 1e6, 2)
                    if len(ts) > 1 else None,
                    "min_us": round(min(ts) * 1e6, 2),
                    "written_GBps": round(out_bytes / m / 1e9, 3),
                    "batches_us": [round(t * 1e6, 1) for t in ts]}
        results.append({
            "sample_shape": [H, W, C], "samples_in_file": counts[name],
            "batch": B, "crop": [h, w], "random_crop_and_flip": rand,
            "out_dtype": dst, "layout": "NCHW",
            "bytes_read_per_batch": B * C * h * w,
            "bytes_written_per_batch": out_bytes,
            "timed_batches": len(new_t),
            "warmup_batches": min(n_warm, n_timed),
            "array_loader": stats(new_t),
            "gather_then_torch": stats(old_t),
            "array_samples_call": stats(call_t),
            "plan_s": {"array_loader_all_batches": round(new_plan_s, 3),
                       "gather_timed_batches": round(parent_plan_s, 3)},
            "outputs_equal": True})
        print(json.dumps(results[-1]), flush=True)

    report = {"bench": "array_loader", "device": device, "tier": tier,
              "file_mb": {"big": args.file_mb, "small": args.small_mb},
              "shuffle": True,
              "timing": "host clock around one batch, device synchronised "
                        "at both ends; warm-up batches of both routes first, "
                        "then the routes alternate per batch; "
                        "array_samples_call = the replayed "
                        "exec_array_samples call alone (upload, one launch, "
                        "stream synchronise) into an existing tensor",
              "results": results}
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
