#!/usr/bin/env python3
"""FP8 checkpoints through the HBM tier: sdk.save_file(quantize="row")
(one absmax_segments_kernel launch, then the quantising store of every
block) against what a user had to do before it existed — scales and fp8
weights computed with torch on the GPU, then save_file of the results as
same-dtype copies — and load(dequantize=True, dtype=bf16) against the
unscaled fp8 -> bf16 load followed by a torch multiply.

Two files: one 64 Mi-element BF16 weight, and 300 tensors (20 BF16
matrices that are quantised, 280 F32 vectors that are not).  Every sample
is a host clock between torch.cuda.synchronize() calls; the compared
routes alternate inside one run; the median is over at least 10 repeats
after warm-up.  Each case runs in a fresh process under a time limit of
its own; this process only starts them and joins their results into one
JSON.  Needs a GPU: there is no CPU fallback.

    python scripts/safetensors_fp8_bench.py --out profiles/safetensors_fp8.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MiB = 1 << 20
CASES = ("save_big", "save_many", "load_big", "load_many")


def stats(samples_s):
    us = [s * 1e6 for s in samples_s]
    return {"median_us": round(statistics.median(us), 1),
            "mean_us": round(statistics.fmean(us), 1),
            "min_us": round(min(us), 1), "max_us": round(max(us), 1),
            "stdev_us": round(statistics.stdev(us), 1) if len(us) > 1 else 0.0,
            "repeats": len(us)}


def alternate(fns: dict, warmup: int, repeats: int):
    """{name: [seconds]}: the routes take turns inside every round"""
    import torch
    out = {k: [] for k in fns}
    for i in range(warmup + repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if i >= warmup:
                out[k].append(dt)
    return out


def tensors_of(case: str, elems: int):
    import torch
    if case.endswith("big"):
        side = int(elems ** 0.5)
        return {"w": torch.randn(side, elems // side, device="cuda:0")
                .to(torch.bfloat16)}
    many = {f"layer{i:03d}.weight": torch.randn(
        1024, 2048, device="cuda:0").to(torch.bfloat16) for i in range(20)}
    many.update({f"layer{i:03d}.norm": torch.randn(
        8192, dtype=torch.float32, device="cuda:0") for i in range(280)})
    return many


def torch_quantize(tensors: dict) -> dict:
    """the reference expression on the GPU, row scales, for the tensors
    save_file's default filter selects"""
    import torch
    out = {}
    for name, w in tensors.items():
        if w.ndim < 2:
            out[name] = w
            continue
        s = w.float().abs().nan_to_num(nan=0, posinf=0, neginf=0) \
            .reshape(w.shape[0], -1).amax(dim=1, keepdim=True) \
            .clamp(min=2 ** -40) / 448
        shape = [-1] + [1] * (w.ndim - 1)
        out[name] = (w.float() / s.reshape(shape)).clamp(-448, 448) \
            .to(torch.float8_e4m3fn)
        out[name + "_scale"] = s
    return out


def run_case(case: str, elems: int, warmup: int, repeats: int) -> dict:
    import torch

    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors, save_file
    from curvine_amd.testing import SyncMiniCluster, test_conf

    tmp = tempfile.mkdtemp(prefix="stfp8-bench-")
    smc = SyncMiniCluster(conf=test_conf(tmp), tmp_dir=tmp,
                          worker_dirs=[["[HBM:3GB:0]gpu0"]]).start()
    try:
        sf = SyncFs(smc.client_conf())
        tensors = tensors_of(case, elems)
        kw = dict(storage_tier="HBM", block_size=64 * MiB, overwrite=True)
        fused_path, torch_path = "/bench/fused.safetensors", \
            "/bench/torch.safetensors"

        def fused_save():
            save_file(sf, tensors, fused_path, quantize="row", **kw)

        def torch_save():
            save_file(sf, torch_quantize(tensors), torch_path, **kw)

        fused_save()
        torch_save()
        blob = sf.read_file(fused_path)
        res = {"file_bytes": len(blob),
               "files_identical": blob == sf.read_file(torch_path)}
        del blob
        if case.startswith("save"):
            # where the routes differ, and which of them is torch's CPU
            # result (the reference expression on cpu copies)
            with CurvineSafetensors(sf, fused_path) as ff, \
                    CurvineSafetensors(sf, torch_path) as ft:
                a, b = ff.load(device="cpu"), ft.load(device="cpu")
            ref = torch_quantize({k: v.cpu() for k, v in tensors.items()})

            def differ(x, y):
                return {kind: sum(int((x[n].view(iv) != y[n].view(iv)).sum())
                                  for n in x if n.endswith("_scale") == sc)
                        for kind, sc, iv in (("scale_elements", True,
                                              torch.int32),
                                             ("other_bytes", False,
                                              torch.uint8))}
            res["fused_vs_torch_cpu_reference"] = differ(a, ref)
            res["torch_gpu_route_vs_torch_cpu_reference"] = differ(b, ref)
            del a, b, ref
            t = alternate({"save_file_quantize_row": fused_save,
                           "torch_quantize_then_save_file": torch_save},
                          warmup, repeats)
        else:
            bf = torch.bfloat16
            f = CurvineSafetensors(sf, fused_path)
            weights = [n for n in tensors if tensors[n].ndim >= 2]
            others = [n for n in tensors if tensors[n].ndim < 2]
            scales = [n + "_scale" for n in weights]

            def fused_load():
                return f.load(device="cuda:0", dtype=bf, dequantize=True)

            def torch_load():
                out = f.load(device="cuda:0", dtype=bf,
                             names=weights + others)
                sc = f.load(device="cuda:0", names=scales)
                for n in weights:
                    s = sc[n + "_scale"]
                    out[n] = (out[n] * s.reshape(
                        [-1] + [1] * (out[n].ndim - 1))).to(bf)
                return out

            a, b = fused_load(), torch_load()
            res["results_identical"] = all(
                torch.equal(a[n].view(torch.int16), b[n].view(torch.int16))
                for n in weights)
            del a, b
            t = alternate({"load_dequantize": fused_load,
                           "load_then_torch_multiply": torch_load},
                          warmup, repeats)
            f.close()
        names = list(t)
        for k in names:
            res[k] = stats(t[k])
        res["fused_over_torch_route"] = round(
            res[names[0]]["median_us"] / res[names[1]]["median_us"], 3)
        sf.shutdown()
        return res
    finally:
        smc.stop()


WHAT = {
    "save_big": "one BF16 weight on cuda:0 into the HBM tier, 64 MiB "
                "blocks: save_file(quantize='row') against the reference "
                "expression in torch on the GPU + save_file of the fp8 and "
                "scale tensors",
    "save_many": "20 BF16 matrices of 1024x2048 (quantised) and 280 F32 "
                 "vectors of 8192 (kept) on cuda:0, the same two routes",
    "load_big": "the one-weight file from the HBM tier to cuda:0 as BF16: "
                "load(dequantize=True) against load(dtype=bf16) of the "
                "weights + load of the scales + (w * s).to(bf16) in torch",
    "load_many": "the 300-tensor file, the same two routes",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/safetensors_fp8.json")
    ap.add_argument("--elems", type=int, default=64 << 20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=CASES,
                    help="run one case in this process and print its JSON")
    ap.add_argument("--case-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.repeats < 10:
        raise SystemExit("at least 10 repeats")
    if args.case:
        from curvine_amd import native
        if not native.gpu_available():
            raise SystemExit("needs a GPU")
        print(json.dumps(run_case(args.case, args.elems, args.warmup,
                                  args.repeats)))
        return
    out = {"source": (
        "scripts/safetensors_fp8_bench.py, one run on one MI355X, each case "
        "in a fresh process.  Host clock between torch.cuda.synchronize() "
        "calls around whole save_file / load calls; the two routes "
        f"alternate inside the run; {args.warmup} warm-up rounds; median / "
        f"min / max / sample stdev over {args.repeats} repeats."),
        "elems_big": args.elems}
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(args.case_timeout), sys.executable,
               os.path.abspath(__file__), "--case", case,
               "--elems", str(args.elems), "--repeats", str(args.repeats),
               "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"{case}: exit status {p.returncode}; nothing "
                             "more is started")
        out[case] = dict(what=WHAT[case],
                         **json.loads(p.stdout.strip().splitlines()[-1]))
        sys.stderr.write(f"{case}: done\n")
        sys.stderr.flush()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
