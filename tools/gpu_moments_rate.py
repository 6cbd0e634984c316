"""Second-moment accumulation against binned accumulation and evaluation with roots written, on tile-major batches (fdg.h:
fdg_accumulate_device_moments).  parquet_sigma4 (the headline, L = 84, R = 4) at 1e8 samples: eval_device_tiled, and accumulate_moments /
accumulate_binned for n_bin = 1 (no bin vector for the moments call, an all-zero one for the binned call), 64, 4096 and FDG_BIN_MAX with
uniform bins; parquet_ver4_4 (R = 180) at 1e7 samples with n_bin = 1024 (the root-slice loop).  Prints ONE JSON line: ms per call, and the
ratio of each moments call to the binned call and to eval_device_tiled.

    python tools/gpu_moments_rate.py [--samples 1e8] [--ver4-samples 1e7] [--reps 5]
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


def uniform_bins(B, n_bin, dev):
    g = torch.Generator(device=dev).manual_seed(n_bin)
    return torch.randint(0, n_bin, (B,), generator=g, device=dev, dtype=torch.int32)


def case(rows, key, f, leaf, bins, n_bin, w, B, R, dev, reps):
    acc = torch.zeros((n_bin, R), dtype=torch.float64, device=dev)
    acc2 = torch.zeros_like(acc)
    tie = torch.zeros(B, dtype=torch.int32, device=dev) if bins is None else bins
    rows[key + "_moments_ms"] = timed(lambda: f.accumulate_moments(leaf, bins, n_bin, w, acc, acc2, n_sample=B), reps)
    rows[key + "_binned_ms"] = timed(lambda: f.accumulate_binned(leaf, tie, n_bin, w, acc, n_sample=B), reps)
    rows[key + "_moments_vs_binned"] = rows[key + "_moments_ms"] / rows[key + "_binned_ms"]
    rows[key + "_moments_vs_eval"] = rows[key + "_moments_ms"] / rows["eval_device_tiled_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=float, default=1e8)
    ap.add_argument("--ver4-samples", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {"tool": "gpu_moments_rate", "device": torch.cuda.get_device_name(0)}

    t = workloads.get("parquet_sigma4")
    B = int(a.samples) // 64 * 64
    T = B // 64
    f = fd.compile_table(t, specialize="isa")
    leaf = torch.empty((T, t.n_leaf, 64), dtype=torch.float64, device=dev)
    capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 1234, 0, st)
    w = torch.rand(B, dtype=torch.float64, device=dev)
    rows = {"samples": B}
    root = torch.empty((T, t.n_root, 64), dtype=torch.float64, device=dev)
    rows["eval_device_tiled_ms"] = timed(lambda: f.eval_tiled(root, leaf, B), a.reps)
    del root
    case(rows, "bins_1_null", f, leaf, None, 1, w, B, t.n_root, dev, a.reps)
    for n_bin in (64, 4096, capi.FDG_BIN_MAX):
        bins = uniform_bins(B, n_bin, dev)
        case(rows, f"bins_{n_bin}", f, leaf, bins, n_bin, w, B, t.n_root, dev, a.reps)
        del bins
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
    case(rows, "bins_1024", f, leaf, uniform_bins(B, 1024, dev), 1024, w, B, t.n_root, dev, max(1, a.reps // 2))
    out["parquet_ver4_4"] = rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
