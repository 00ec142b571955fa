#!/usr/bin/env python3
"""Block-scaled FP8 checkpoints (128 x 128 tiles, F32 `_scale_inv`) through
the HBM tier: sdk.save_file(quantize="block", quantize_block=(128, 128))
(one block_absmax_kernel
launch, then the block store of every file block) and
load(dequantize=True, dtype=bf16) of the files, each next to the
quantize="row" save and row-dequantising load of the same tensors, whose
code this change leaves as the parent commit has it.  The loads also run
next to torch on the GPU doing

    q.float() * s.repeat_interleave(128, 0).repeat_interleave(128, 1)

(trimmed to the shape, cast to bf16) around the unscaled load of the same
file, which is what a user had to write before.

Two files: one 64 Mi-element BF16 weight, and 300 tensors (20 BF16
matrices that are quantised, 280 F32 vectors that are not).  Every sample
is a host clock between torch.cuda.synchronize() calls; the routes
alternate inside one run; the median is over at least 10 repeats after
warm-up.  Each case runs in a fresh process under a time limit of its own;
this process only starts them and joins their results into one JSON.
Needs a GPU: there is no CPU fallback.

    python scripts/safetensors_block_bench.py \
        --out profiles/safetensors_block.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safetensors_fp8_bench import alternate, stats, tensors_of  # noqa: E402

MiB = 1 << 20
CASES = ("save_big", "save_many", "load_big", "load_many")
MODES = ("block", "row")
BLOCK = 128


def run_case(case: str, elems: int, warmup: int, repeats: int) -> dict:
    import torch

    from curvine_amd.client.filesystem import SyncFs
    from curvine_amd.sdk import CurvineSafetensors, save_file
    from curvine_amd.testing import SyncMiniCluster, test_conf

    tmp = tempfile.mkdtemp(prefix="stblk-bench-")
    smc = SyncMiniCluster(conf=test_conf(tmp), tmp_dir=tmp,
                          worker_dirs=[["[HBM:3GB:0]gpu0"]]).start()
    try:
        sf = SyncFs(smc.client_conf())
        tensors = tensors_of(case, elems)
        kw = dict(storage_tier="HBM", block_size=64 * MiB, overwrite=True)

        def saver(mode):
            geom = {"quantize_block": (BLOCK, BLOCK)} if mode == "block" \
                else {}
            return lambda: save_file(sf, tensors, f"/bench/{mode}.safetensors",
                                     quantize=mode, **geom, **kw)
        res = {}
        for mode in MODES:
            res[f"file_bytes_{mode}"] = saver(mode)().length
        if case.startswith("save"):
            t = alternate({f"save_{m}": saver(m) for m in MODES}, warmup,
                          repeats)
        else:
            files = {m: CurvineSafetensors(sf, f"/bench/{m}.safetensors")
                     for m in MODES}

            def loader(mode):
                return lambda: files[mode].load(
                    device="cuda:0", dtype=torch.bfloat16, dequantize=True)

            def torch_route():
                raw = files["block"].load(device="cuda:0")
                out = {}
                for name, q in raw.items():
                    if name.endswith("_scale_inv"):
                        continue
                    s = raw.get(name + "_scale_inv")
                    if s is None:
                        out[name] = q
                        continue
                    se = s.repeat_interleave(BLOCK, 0) \
                        .repeat_interleave(BLOCK, 1)[:q.shape[0], :q.shape[1]]
                    out[name] = (q.float() * se).to(torch.bfloat16)
                return out
            fns = {f"load_{m}": loader(m) for m in MODES}
            fns["load_torch_repeat_interleave"] = torch_route
            t = alternate(fns, warmup, repeats)
            for f in files.values():
                f.close()
        for k in t:
            res[k] = stats(t[k])
        base = [k for k in t if k.endswith("_row")][0]
        for k in t:
            if k != base:
                res[f"{k}_over_row"] = round(
                    res[k]["median_us"] / res[base]["median_us"], 3)
        if "load_torch_repeat_interleave" in t:
            res["load_block_over_torch"] = round(
                res["load_block"]["median_us"] /
                res["load_torch_repeat_interleave"]["median_us"], 3)
        sf.shutdown()
        return res
    finally:
        smc.stop()


WHAT = {
    "save_big": "one BF16 weight on cuda:0 into the HBM tier, 64 MiB blocks: "
                "save_file(quantize='block') and ('row')",
    "save_many": "20 BF16 matrices of 1024x2048 (quantised) and 280 F32 "
                 "vectors of 8192 (kept) on cuda:0, the same two routes",
    "load_big": "each one-weight file from the HBM tier to cuda:0 as BF16 "
                "with load(dequantize=True), and torch's repeat_interleave "
                "expression around the unscaled load of the block file",
    "load_many": "each 300-tensor file, the same",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/safetensors_block.json")
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
        "scripts/safetensors_block_bench.py, one run on one MI355X, each "
        "case in a fresh process.  Host clock between "
        "torch.cuda.synchronize() calls around whole save_file / load calls; "
        "the routes alternate inside the run; "
        f"{args.warmup} warm-up rounds; median / min / max / sample stdev "
        f"over {args.repeats} repeats.  The row route is the parent commit's "
        "code, unchanged."),
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
