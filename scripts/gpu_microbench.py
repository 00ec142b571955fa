#!/usr/bin/env python3
"""Kernel/data-path microbenchmarks on the MI355X: arena H2D/D2H bandwidth,
CRC32C kernel throughput, gather (extent-pack) throughput, fill, D2D.

Run under rocprofv3 for per-kernel stats:
    rocprofv3 --kernel-trace --stats -d gpurun_out/prof -- \
        python scripts/gpu_microbench.py
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
from curvine_amd import native


def timeit(fn, n=5, warmup=2):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) / n


def bench_lz4(a, rng, results):
    mod = native.load()
    # LZ4 device decompress: 512 MiB of ~3:1-compressible data
    rep = np.frombuffer((b"curvine-amd lz4 block payload %06d " % 42) * 64,
                        dtype=np.uint8)
    block = np.tile(rep, (512 << 20) // len(rep) + 1)[:512 << 20].copy()
    noise_idx = rng.choice(len(block), len(block) // 64, replace=False)
    block[noise_idx] = rng.integers(0, 256, len(noise_idx), dtype=np.uint8)
    comp = native.lz4_compress(block.tobytes())
    results["lz4_ratio"] = round(len(block) / len(comp), 2)
    dt = timeit(lambda: mod.arena_lz4_decompress(a.handle, 0, comp))
    results["lz4_device_decompress_GBps"] = round(len(block) / dt / 1e9, 2)
    back = np.zeros(1 << 20, dtype=np.uint8)
    a.read(0, back, 0, 1 << 20)
    assert back.tobytes() == block[:1 << 20].tobytes()
    dt = timeit(lambda: native.lz4_decompress(comp))
    results["lz4_host_decompress_GBps"] = round(len(block) / dt / 1e9, 2)

    # LZ4 device compress: the first 16 MiB of that block (one call's
    # limit), read where it lives in the arena, against the host codec —
    # the only other way the product has to make a container
    cn = 16 << 20
    raw = block[:cn].tobytes()
    a.write(0, raw, 0, cn)
    dev_c = a.lz4_compress(0, cn)
    assert native.lz4_decompress(dev_c) == raw
    dt = timeit(lambda: a.lz4_compress(0, cn))
    dev_gbps = cn / dt / 1e9
    results["lz4_device_compress_GBps"] = round(dev_gbps, 2)
    host_c = native.lz4_compress(raw)
    dt = timeit(lambda: native.lz4_compress(raw))
    host_gbps = cn / dt / 1e9
    results["lz4_host_compress_GBps"] = round(host_gbps, 3)
    results["lz4_device_vs_host_size"] = round(len(dev_c) / len(host_c), 4)
    results["lz4_compress_raw_bytes"] = cn
    results["lz4_device_container_bytes"] = len(dev_c)
    results["lz4_host_container_bytes"] = len(host_c)
    # does compressing before the host link pay?  57 GB/s = pinned D2H
    link = 57.0
    t_lz4 = cn / dev_gbps / 1e9 + len(dev_c) / link / 1e9
    t_raw = cn / link / 1e9
    results["lz4_device_faster_than_host"] = bool(dev_gbps > host_gbps)
    results["lz4_compress_then_d2h_us"] = round(t_lz4 * 1e6, 1)
    results["raw_d2h_us"] = round(t_raw * 1e6, 1)
    results["lz4_compress_then_d2h_beats_raw_d2h"] = bool(t_lz4 < t_raw)


def _stats(ts):
    ts = sorted(ts)
    return {"median_us": round(float(np.median(ts)) * 1e6, 1),
            "min_us": round(ts[0] * 1e6, 1), "max_us": round(ts[-1] * 1e6, 1),
            "stdev_us": round(float(np.std(ts, ddof=1)) * 1e6, 1),
            "repeats": len(ts)}


def _alternate(fns, repeats=15, inner=8, warmup=3):
    """Time several callables in the same run, alternating them; every
    sample is `inner` back-to-back calls (each ends in a device sync)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            out[i].append((time.perf_counter() - t0) / inner)
    return [_stats(ts) for ts in out]


def bench_safetensors(results):
    """Typed loads out of the HBM arena (convert_segments_kernel) against
    what the same user does without it; see profiles/safetensors_load.json."""
    import tempfile

    import torch
    D = native.DTYPES
    n_el = 64 << 20
    a = native.Arena(0, (256 << 20) + (1 << 20))
    rng = np.random.default_rng(3)
    chunk = rng.integers(0, 2 ** 32, 4 << 20, dtype=np.uint32)
    chunk &= np.uint32(0xBFFFFFFF)
    for i in range(0, 256 << 20, chunk.nbytes):
        a.write(i, chunk.tobytes())
    a.write(256 << 20, b"\0" * 64)
    dev = torch.device("cuda:0")

    def fused_f32_bf16(off=0):
        out = torch.empty(n_el, dtype=torch.bfloat16, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        a.convert_ptr([(off, out.data_ptr(), 1, n_el, n_el * 4,
                        D["F32"], D["BF16"])])
        return out

    def two_pass_f32_bf16():
        tmp = torch.empty(n_el * 4, dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        a.read_to_ptr(0, tmp.data_ptr(), n_el * 4, True)
        out = tmp.view(torch.float32).to(torch.bfloat16)
        torch.cuda.synchronize(dev)
        return out

    assert torch.equal(fused_f32_bf16().view(torch.int16),
                       two_pass_f32_bf16().view(torch.int16))
    fused, two = _alternate([fused_f32_bf16, two_pass_f32_bf16])
    ratio = fused["median_us"] / two["median_us"]
    results["f32_to_bf16_64Mi"] = {
        "fused": fused, "two_pass_d2d_then_torch_cast": two,
        "fused_over_two_pass": round(ratio, 3),
        "fused_GBps_rd_plus_wr": round(n_el * 6 / fused["median_us"] / 1e3, 1),
        "bar_fused_not_slower_than_two_pass_plus_its_stdev": bool(
            fused["median_us"] <= two["median_us"] + two["stdev_us"])}

    nb = n_el * 2

    def same_bf16(off):
        def run():
            out = torch.empty(n_el, dtype=torch.bfloat16, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            a.convert_ptr([(off, out.data_ptr(), 1, n_el, nb,
                            D["BF16"], D["BF16"])])
            return out
        return run

    def d2d(off):
        def run():
            out = torch.empty(n_el, dtype=torch.bfloat16, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            a.read_to_ptr(off, out.data_ptr(), nb, True)
            torch.cuda.synchronize(dev)
            return out
        return run

    for tag, off in (("aligned", 0), ("odd_offset", 1)):
        assert torch.equal(same_bf16(off)().view(torch.int16),
                           d2d(off)().view(torch.int16))
        k, c = _alternate([same_bf16(off), d2d(off)])
        results[f"bf16_copy_64Mi_{tag}"] = {
            "convert_ptr": k, "read_to_ptr_d2d": c,
            "convert_over_d2d": round(k["median_us"] / c["median_us"], 3),
            "convert_GBps_rd_plus_wr": round(
                2 * nb / k["median_us"] / 1e3, 1)}
    a.close()

    # 300-tensor file through the whole stack: batched load() against a
    # loop of get_tensor()
    import json as _json
    import struct

    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors
    from curvine_amd.testing import SyncMiniCluster, test_conf
    hdr, parts, pos = {}, [], 0
    for i in range(300):
        shape = (1024, 2048) if i % 15 == 0 else (8192,)
        dt = "BF16" if i % 15 == 0 else "F32"
        nbytes = int(np.prod(shape)) * (2 if dt == "BF16" else 4)
        raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
        raw[1::2] &= 0xBF
        hdr[f"layer{i:03d}.w"] = {"dtype": dt, "shape": list(shape),
                                  "data_offsets": [pos, pos + nbytes]}
        parts.append(raw.tobytes())
        pos += nbytes
    js = _json.dumps(hdr).encode()
    js += b" " * (-(len(js) + 8) % 64)      # aligned data section
    blob = struct.pack("<Q", len(js)) + js + b"".join(parts)
    tmp = tempfile.mkdtemp(prefix="curvine-stbench-")
    conf = test_conf(tmp)
    conf.master.block_size = conf.client.block_size = 64 << 20
    smc = SyncMiniCluster(conf=conf, tmp_dir=tmp,
                          worker_dirs=[["[HBM:1GB:0]gpu0"]]).start()
    try:
        sf = SyncFs(smc.client_conf())
        sf.write_file("/bench/m.safetensors", blob, storage_tier="HBM")
        f = CurvineSafetensors(sf, "/bench/m.safetensors")

        def batched():
            return f.load(device="cuda:0", dtype=torch.bfloat16)

        def looped():
            return {k: f.get_tensor(k, "cuda:0", torch.bfloat16)
                    for k in f.keys()}
        b_out, l_out = batched(), looped()
        assert all(torch.equal(b_out[k].view(torch.int16),
                               l_out[k].view(torch.int16)) for k in b_out)
        del b_out, l_out
        b, lp = _alternate([batched, looped], repeats=9, inner=2, warmup=2)
        results["file_300_tensors"] = {
            "file_bytes": len(blob), "batched_load": b,
            "get_tensor_loop": lp,
            "batched_over_loop": round(b["median_us"] / lp["median_us"], 3)}
        f.close()
        sf.shutdown()
    finally:
        smc.stop()


def main():
    assert native.gpu_available(), "needs a GPU"
    if "--safetensors-only" in sys.argv[1:]:
        results = {}
        bench_safetensors(results)
        print(json.dumps(results, indent=1))
        return
    if "--lz4-only" in sys.argv[1:]:
        a = native.Arena(0, (512 << 20) + (1 << 20), staging_bytes=16 << 20,
                         staging_count=8)
        results = {}
        bench_lz4(a, np.random.default_rng(1), results)
        print(json.dumps(results, indent=1))
        a.close()
        return
    GB = 1 << 30
    size = 4 * GB
    a = native.Arena(0, size + (1 << 20), staging_bytes=16 << 20,
                     staging_count=8)
    results = {}

    host = np.random.default_rng(0).integers(0, 256, 1 * GB, dtype=np.uint8)
    pin = native.PinnedBuffer(1 * GB)

    # H2D via staging ring (pageable source)
    dt = timeit(lambda: a.write(0, host, 0, len(host)))
    results["h2d_pageable_ring_GBps"] = round(len(host) / dt / 1e9, 2)

    # H2D from pinned (direct DMA)
    pin.view[:len(host)] = host.tobytes()
    dt = timeit(lambda: a.write_from_ptr(0, pin.ptr, len(host), False))
    results["h2d_pinned_GBps"] = round(len(host) / dt / 1e9, 2)

    # D2H via staging ring into pageable
    out = np.zeros(1 * GB, dtype=np.uint8)
    dt = timeit(lambda: a.read(0, out, 0, len(out)))
    results["d2h_pageable_ring_GBps"] = round(len(out) / dt / 1e9, 2)

    # D2H direct into pinned
    dt = timeit(lambda: a.read_to_ptr(0, pin.ptr, len(host), False))
    results["d2h_pinned_GBps"] = round(len(host) / dt / 1e9, 2)
    assert bytes(pin.view[:1 << 20]) == host[:1 << 20].tobytes()

    # device CRC32C kernel (1 GiB resident)
    crc_host = native.crc32c(host)
    dt = timeit(lambda: a.crc32c(0, len(host)))
    assert a.crc32c(0, len(host)) == crc_host
    results["crc32c_device_GBps"] = round(len(host) / dt / 1e9, 2)
    results["crc32c_matches_host"] = True

    # host CRC32C (SSE4.2) for comparison
    dt = timeit(lambda: native.crc32c(host))
    results["crc32c_host_sse42_GBps"] = round(len(host) / dt / 1e9, 2)

    # gather: pack 256 x 1 MiB scattered extents into pinned
    rng = np.random.default_rng(1)
    offs = sorted(rng.choice(range(0, 3 * GB // (1 << 20)), 256,
                             replace=False).tolist())
    extents = [(int(o) << 20, 1 << 20) for o in offs]
    total = sum(e[1] for e in extents)
    gout = np.zeros(total, dtype=np.uint8)
    dt = timeit(lambda: a.gather(extents, gout, 0))
    results["gather_256x1MiB_GBps"] = round(total / dt / 1e9, 2)

    # device fill
    dt = timeit(lambda: a.fill(0, 1 * GB, 0))
    results["fill_device_GBps"] = round(GB / dt / 1e9, 2)

    # D2D copy within arena (block move / promotion analog)
    dt = timeit(lambda: native.load().arena_copy(a.handle, 2 * GB, a.handle, 0, GB))
    results["d2d_copy_GBps"] = round(2 * GB / dt / 1e9, 2)  # rd+wr bytes

    # on-device sample gather (CurvineDeviceLoader hot path): 4096 x
    # 256 KiB scattered extents packed to a device destination
    mod = native.load()
    n_s, s_sz = 4096, 256 << 10
    src_offs = rng.choice(range(0, (2 * GB) // s_sz), n_s,
                          replace=False).tolist()
    triples = [(int(o) * s_sz, i * s_sz, s_sz)
               for i, o in enumerate(src_offs)]
    dst_ptr = a.base_ptr() + 3 * GB
    dt = timeit(lambda: mod.arena_gather_ptr(a.handle, triples, dst_ptr))
    results["gather_dev_4096x256KiB_GBps"] = round(
        2 * n_s * s_sz / dt / 1e9, 2)   # rd+wr bytes

    bench_lz4(a, rng, results)

    a.close()
    pin.close()
    bench_safetensors(results)
    print(json.dumps(results, indent=1))


if __name__ == "__main__":
    main()
