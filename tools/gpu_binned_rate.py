"""Binned accumulation against evaluation with roots written and plain fused accumulation, on tile-major batches (fdg.h:
fdg_accumulate_device_binned).  parquet_sigma4 (the headline, L = 84, R = 4) at 1e8 samples: eval_device_tiled, accumulate_device_tiled and
accumulate_binned for n_bin in {1, 64, 4096} with uniform bins and for 90 % of the samples in one bin of 4096; parquet_ver4_4 (R = 180) at 1e7
samples with n_bin = 1024 (the root-slice loop).  Prints ONE JSON line: ms per call and the ratio of each binned call to eval_device_tiled.

    python tools/gpu_binned_rate.py [--samples 1e8] [--ver4-samples 1e7] [--reps 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, workloads  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def uniform_bins(B, n_bin, dev, skew=False):
    g = torch.Generator(device=dev).manual_seed(n_bin + 7 * skew)
    b = torch.randint(0, n_bin, (B,), generator=g, device=dev, dtype=torch.int32)
    if skew:
        b = torch.where(torch.rand(B, generator=g, device=dev, dtype=torch.float64) < 0.9, torch.zeros_like(b), b)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=float, default=1e8)
    ap.add_argument("--ver4-samples", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {"tool": "gpu_binned_rate", "device": torch.cuda.get_device_name(0)}

    t = workloads.get("parquet_sigma4")
    B = int(a.samples) // 64 * 64
    f = fd.compile_table(t, specialize="isa")
    T = B // 64
    leaf = torch.empty((T, t.n_leaf, 64), dtype=torch.float64, device=dev)
    capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 1234, 0, st)
    w = torch.rand(B, dtype=torch.float64, device=dev)
    root = torch.empty((T, t.n_root, 64), dtype=torch.float64, device=dev)
    rows = {"samples": B}
    rows["eval_device_tiled_ms"] = timed(lambda: f.eval_tiled(root, leaf, B), a.reps)
    del root
    rows["accumulate_device_tiled_ms"] = timed(lambda: f.accumulate_tiled(leaf, w, None, B), a.reps)
    for n_bin, skew in ((1, False), (64, False), (4096, False), (4096, True)):
        bins = uniform_bins(B, n_bin, dev, skew)
        acc = torch.zeros((n_bin, t.n_root), dtype=torch.float64, device=dev)
        key = f"binned_{n_bin}{'_skew90' if skew else ''}"
        rows[key + "_ms"] = timed(lambda: f.accumulate_binned(leaf, bins, n_bin, w, acc, n_sample=B), a.reps)
        rows[key + "_vs_eval"] = rows[key + "_ms"] / rows["eval_device_tiled_ms"]
        del bins, acc
    out["parquet_sigma4"] = rows
    del leaf, w
    torch.cuda.empty_cache()

    t = workloads.get("parquet_ver4_4")
    B = int(a.ver4_samples) // 64 * 64
    T = B // 64
    f = fd.compile_table(t, specialize="isa")
    leaf = torch.empty((T, t.n_leaf, 64), dtype=torch.float64, device=dev)
    capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 99, 0, st)
    w = torch.rand(B, dtype=torch.float64, device=dev)
    rows = {"samples": B}
    root = torch.empty((T, t.n_root, 64), dtype=torch.float64, device=dev)
    rows["eval_device_tiled_ms"] = timed(lambda: f.eval_tiled(root, leaf, B), max(1, a.reps // 2))
    del root
    bins = uniform_bins(B, 1024, dev)
    acc = torch.zeros((1024, t.n_root), dtype=torch.float64, device=dev)
    rows["binned_1024_ms"] = timed(lambda: f.accumulate_binned(leaf, bins, 1024, w, acc, n_sample=B), max(1, a.reps // 2))
    rows["binned_1024_vs_eval"] = rows["binned_1024_ms"] / rows["eval_device_tiled_ms"]
    out["parquet_ver4_4"] = rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
