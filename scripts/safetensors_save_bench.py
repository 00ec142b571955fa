#!/usr/bin/env python3
"""Checkpoint save into the HBM tier: sdk.save_file (typed store, one
store_segments_kernel launch per block) against what a user had to do
before it existed — tensor.cpu() (after a torch cast on the GPU), hand
serialisation, SyncFs.write_file into the same tier — and the store call
alone against Arena.write_from_ptr of the same bytes.

Every sample is a host clock around calls that end synchronised (save_file
and write_file return after the blocks are finalised; the arena calls
synchronise their stream).  The compared paths alternate inside one run;
the files they leave are compared byte for byte before any timing.
Needs a GPU: there is no CPU fallback.

    python scripts/safetensors_save_bench.py --out profiles/safetensors_save.json
"""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from curvine_amd import native  # noqa: E402

MiB = 1 << 20
NAME = {torch.float32: "F32", torch.bfloat16: "BF16"}


def stats(samples_s, calls=1):
    us = [s / calls * 1e6 for s in samples_s]
    return {"median_us": round(statistics.median(us), 1),
            "mean_us": round(statistics.fmean(us), 1),
            "min_us": round(min(us), 1), "max_us": round(max(us), 1),
            "stdev_us": round(statistics.stdev(us), 1) if len(us) > 1 else 0.0,
            "repeats": len(us)}


def alternate(fns: dict, warmup: int, repeats: int):
    """{name: [seconds]}: the paths take turns inside every round"""
    out = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i >= warmup:
                out[k].append(dt)
    return out


def hand_serialise(tensors: dict, dtype):
    """what a user writes without the safetensors package: cast on the
    GPU, .cpu(), a header in save_file's own layout, one joined blob"""
    host = {}
    for name, t in tensors.items():
        if dtype is not None and t.is_floating_point():
            t = t.to(dtype)
        host[name] = t.cpu().contiguous()
    order = sorted(host, key=lambda n: (-host[n].element_size(), n))
    hdr, pos = {}, 0
    for n in order:
        nb = host[n].numel() * host[n].element_size()
        hdr[n] = {"dtype": NAME[host[n].dtype], "shape": list(host[n].shape),
                  "data_offsets": [pos, pos + nb]}
        pos += nb
    js = json.dumps(hdr, separators=(",", ":")).encode()
    js += b" " * (-(8 + len(js)) % 64)
    parts = [struct.pack("<Q", len(js)), js]
    parts += [memoryview(host[n].view(-1).view(torch.uint8).numpy())
              for n in order]
    return b"".join(parts)


def file_case(sf, tensors, dtype, block_size, warmup, repeats, tag):
    from curvine_amd.sdk import save_file

    def fast():
        save_file(sf, tensors, f"/bench/{tag}_fast.safetensors", dtype=dtype,
                  storage_tier="HBM", block_size=block_size, overwrite=True)

    def parent():
        blob = hand_serialise(tensors, dtype)
        sf.write_file(f"/bench/{tag}_parent.safetensors", blob,
                      storage_tier="HBM", block_size=block_size)

    fast()
    parent()
    a = sf.read_file(f"/bench/{tag}_fast.safetensors")
    b = sf.read_file(f"/bench/{tag}_parent.safetensors")
    if a != b:
        raise SystemExit(f"{tag}: the two paths wrote different files")
    t = alternate({"save_file": fast, "cpu_serialise_write_file": parent},
                  warmup, repeats)
    res = {"file_bytes": len(a),
           "save_file": stats(t["save_file"]),
           "cpu_serialise_write_file": stats(t["cpu_serialise_write_file"]),
           "files_identical": True}
    res["save_over_parent"] = round(
        res["save_file"]["median_us"]
        / res["cpu_serialise_write_file"]["median_us"], 3)
    return res


def arena_case(n_elems, repeats, calls=8):
    a = native.Arena(0, 768 * MiB)
    src = torch.randn(n_elems, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    p, nb = src.data_ptr(), n_elems * 4
    D = native.DTYPES
    seg_copy = [(p, 0, 1, n_elems, nb, D["F32"], D["F32"])]
    seg_cast = [(p, 0, 1, n_elems, nb, D["F32"], D["BF16"])]

    def rep(fn):
        def go():
            for _ in range(calls):
                fn()
        return go
    a.write_from_ptr(0, p, nb, True)
    ref = a.crc32c(0, nb)
    a.fill(0, nb, 0)
    a.store_ptr(seg_copy)
    if a.crc32c(0, nb) != ref:
        raise SystemExit("store_ptr copy differs from write_from_ptr")
    t = alternate({
        "store_ptr_f32_copy": rep(lambda: a.store_ptr(seg_copy)),
        "write_from_ptr_d2d": rep(lambda: a.write_from_ptr(0, p, nb, True)),
        "store_ptr_f32_to_bf16": rep(lambda: a.store_ptr(seg_cast)),
    }, 3, repeats)
    res = {k: stats(v, calls) for k, v in t.items()}
    res["store_copy_over_d2d"] = round(
        res["store_ptr_f32_copy"]["median_us"]
        / res["write_from_ptr_d2d"]["median_us"], 3)
    res["store_copy_GBps_rd_plus_wr"] = round(
        2 * nb / res["store_ptr_f32_copy"]["median_us"] / 1e3, 1)
    res["store_cast_GBps_rd_plus_wr"] = round(
        (nb + nb // 2) / res["store_ptr_f32_to_bf16"]["median_us"] / 1e3, 1)
    # the binding's fixed cost: 300 small tensors in one call
    small = [torch.randn(8192, dtype=torch.float32, device="cuda:0")
             for _ in range(300)]
    torch.cuda.synchronize()
    segs = [(t.data_ptr(), i * 16384, 1, 8192, 32768, D["F32"], D["BF16"])
            for i, t in enumerate(small)]
    t = alternate({"x": rep(lambda: a.store_ptr(segs))}, 3, repeats)
    res["store_ptr_300_segments_of_8192"] = stats(t["x"], calls)
    a.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/safetensors_save.json")
    ap.add_argument("--elems", type=int, default=64 << 20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not native.gpu_available():
        raise SystemExit("needs a GPU")

    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.testing import SyncMiniCluster, test_conf

    out = {"source": (
        "scripts/safetensors_save_bench.py, one run on one MI355X. Host "
        "clock around whole calls that return after the blocks are "
        "finalised (file cases) or after the arena's stream is "
        "synchronised (arena case, 8 calls per sample); the compared paths "
        f"alternate inside the run; {args.warmup} warm-up rounds; median / "
        "min / max / sample stdev over the repeats.  Both file paths pay "
        "the publish-time CRC32C of every block; the parent path also "
        "hashes on the host (client enable_crc default).")}
    out["arena_64Mi_f32"] = dict(
        what=("one 64 Mi-element F32 cuda tensor (256 MiB) into the HBM "
              "arena: Arena.store_ptr same-dtype (raw-copy path of "
              "store_segments_kernel) against Arena.write_from_ptr "
              "(hipMemcpyAsync D2D) of the same bytes, and store_ptr "
              "F32->BF16; arena CRC32C equal before timing"),
        **arena_case(args.elems, 15))

    tmp = tempfile.mkdtemp(prefix="stsave-bench-")
    conf = test_conf(tmp)
    smc = SyncMiniCluster(conf=conf, tmp_dir=tmp,
                          worker_dirs=[["[HBM:3GB:0]gpu0"]]).start()
    try:
        sf = SyncFs(smc.client_conf())
        big = {"w": torch.randn(args.elems, dtype=torch.float32,
                                device="cuda:0")}
        for dt, tag in ((None, "f32_as_f32"), (torch.bfloat16, "f32_as_bf16")):
            out[f"file_64Mi_{tag}"] = dict(
                what=(f"one 64 Mi-element F32 cuda tensor saved "
                      f"{'as stored' if dt is None else 'as BF16'} into the "
                      "HBM tier, 64 MiB blocks: sdk.save_file against "
                      "cast-on-GPU + .cpu() + hand serialisation + "
                      "SyncFs.write_file"),
                **file_case(sf, big, dt, 64 * MiB, args.warmup, args.repeats,
                            tag))
        del big
        many = {f"layer{i:03d}.weight": torch.randn(
            1024, 2048, device="cuda:0").to(torch.bfloat16) for i in range(20)}
        many.update({f"layer{i:03d}.norm": torch.randn(
            8192, dtype=torch.float32, device="cuda:0") for i in range(280)})
        out["file_300_tensors"] = dict(
            what=("20 BF16 matrices of 1024x2048 and 280 F32 vectors of "
                  "8192 on cuda:0 saved as BF16, 64 MiB blocks: "
                  "sdk.save_file against the per-tensor .cpu() loop + hand "
                  "serialisation + SyncFs.write_file"),
            **file_case(sf, many, torch.bfloat16, 64 * MiB, args.warmup,
                        args.repeats, "many"))
        sf.shutdown()
    finally:
        smc.stop()
    a = out["file_64Mi_f32_as_f32"]
    b = out["file_64Mi_f32_as_bf16"]
    out["expectation_case_a_fast_path_not_slower_than_parent"] = bool(
        a["save_over_parent"] <= 1.0 and b["save_over_parent"] <= 1.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
