"""The VEGAS accumulate step against the moments call it extends, and the sampler against the uniform fill (fdg.h:
fdg_accumulate_device_vegas, fdg_vegas_sample_device).  parquet_sigma4 (the headline, L = 84, R = 4), tile-major, 1e8 samples:
accumulate_moments with no bin vector, then accumulate_vegas at (n_dim, n_grid) = (17, 64), (17, 1024), (64, 1024), all in this one
run; the sampler alone at n_dim = 17 (n_grid 64 and 1024, component-major x) against fdg_fill_uniform_device for 17 columns.
Prints ONE JSON line: ms per call and the ratios.

    python tools/gpu_vegas_rate.py [--samples 1e8] [--reps 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {"tool": "gpu_vegas_rate", "device": torch.cuda.get_device_name(0)}

    t = workloads.get("parquet_sigma4")
    B = int(a.samples) // 64 * 64
    T, R = B // 64, t.n_root
    f = fd.compile_table(t, specialize="isa")
    leaf = torch.empty((T, t.n_leaf, 64), dtype=torch.float64, device=dev)
    capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 1234, 0, st)
    w = torch.rand(B, dtype=torch.float64, device=dev)
    rows = {"samples": B}
    acc = torch.zeros((1, R), dtype=torch.float64, device=dev)
    acc2 = torch.zeros_like(acc)
    rows["moments_ms"] = timed(lambda: f.accumulate_moments(leaf, None, 1, w, acc, acc2, n_sample=B), a.reps)
    for D, G in ((17, 64), (17, 1024), (64, 1024)):
        hist = torch.zeros((D, G), dtype=torch.float64, device=dev)
        key = f"vegas_d{D}_g{G}"
        rows[key + "_ms"] = timed(lambda: f.accumulate_vegas(leaf, w, hist, 7, 0, D, G, acc=acc, acc2=acc2, n_sample=B), a.reps)
        rows[key + "_vs_moments"] = rows[key + "_ms"] / rows["moments_ms"]
    rows["moments_again_ms"] = timed(lambda: f.accumulate_moments(leaf, None, 1, w, acc, acc2, n_sample=B), a.reps)
    del leaf, w
    torch.cuda.empty_cache()

    D = 17
    x = torch.empty((D, B), dtype=torch.float64, device=dev)
    jac = torch.empty(B, dtype=torch.float64, device=dev)
    rows["fill_uniform_17_ms"] = timed(lambda: capi.fill_uniform_device(x.data_ptr(), B, D, 1, B, 7, 0, st), a.reps)
    rng = np.random.default_rng(0)
    for G in (64, 1024):
        grid = capi.vegas_refine(vegas.uniform_grid([0.0] * D, [1.0] * D, G), rng.random((D, G)) + 0.1, 1.0)
        d_grid = torch.from_numpy(grid).to(dev)
        key = f"sample_d17_g{G}"
        rows[key + "_ms"] = timed(lambda: capi.vegas_sample_device(d_grid.data_ptr(), D, G, None, 7, 0, x.data_ptr(), 1, B, jac.data_ptr(), 0,
                                                                   B, st), a.reps)
        rows[key + "_vs_fill"] = rows[key + "_ms"] / rows["fill_uniform_17_ms"]
    out["parquet_sigma4"] = rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
