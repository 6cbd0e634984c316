"""The VEGAS accumulate step with a discrete variable against the two calls it replaces, and the discrete sampler against the continuous
one (fdg.h: fdg_accumulate_device_vegas_binned, fdg_vegas_sample_device_discrete).  parquet_sigma4 (the headline, L = 84, R = 4),
tile-major, 1e8 samples, a uniformly random bin vector: per (n_dim, n_grid) in (17, 64), (17, 1024) and n_bin in 64, 4096 the medians
over --reps calls of accumulate_vegas_binned, accumulate_vegas and accumulate_moments with the same bin vector, all in this one run;
the new call evaluates each chunk once where the pair evaluates it twice.  Then the sampler at n_dim = 17 (component-major x) with and
without the discrete variable (n_bin 64, 4096, 16384; a table of three columns).  Prints ONE JSON line: ms per call and the ratios.

    python tools/gpu_vegas_binned_rate.py [--samples 1e8] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402


def median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {"tool": "gpu_vegas_binned_rate", "device": torch.cuda.get_device_name(0)}

    t = workloads.get("parquet_sigma4")
    B = int(a.samples) // 64 * 64
    T, R = B // 64, t.n_root
    f = fd.compile_table(t, specialize="isa")
    leaf = torch.empty((T, t.n_leaf, 64), dtype=torch.float64, device=dev)
    capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 1234, 0, st)
    w = torch.rand(B, dtype=torch.float64, device=dev)
    rows = {"samples": B, "reps": a.reps}
    for n_bin in (64, 4096):
        bins = torch.randint(0, n_bin, (B,), dtype=torch.int32, device=dev)
        acc = torch.zeros((n_bin, R), dtype=torch.float64, device=dev)
        acc2 = torch.zeros_like(acc)
        acc1 = torch.zeros((1, R), dtype=torch.float64, device=dev)
        acc12 = torch.zeros_like(acc1)
        hb = torch.zeros(n_bin, dtype=torch.float64, device=dev)
        mom = median_ms(lambda: f.accumulate_moments(leaf, bins, n_bin, w, acc, acc2, n_sample=B), a.reps)
        rows[f"moments_b{n_bin}_ms"] = mom
        for D, G in ((17, 64), (17, 1024)):
            hist = torch.zeros((D, G), dtype=torch.float64, device=dev)
            key = f"d{D}_g{G}_b{n_bin}"
            veg = median_ms(lambda: f.accumulate_vegas(leaf, w, hist, 7, 0, D, G, acc=acc1, acc2=acc12, n_sample=B), a.reps)
            new = median_ms(lambda: f.accumulate_vegas_binned(leaf, bins, n_bin, w, hist, hb, 7, 0, D, G, acc=acc, acc2=acc2, n_sample=B), a.reps)
            rows["vegas_" + key + "_ms"] = veg
            rows["vegas_binned_" + key + "_ms"] = new
            rows["vegas_binned_" + key + "_vs_pair"] = new / (veg + mom)
        del bins
    del leaf, w
    torch.cuda.empty_cache()

    D = 17
    x = torch.empty((D + 3, B), dtype=torch.float64, device=dev)
    jac = torch.empty(B, dtype=torch.float64, device=dev)
    bins = torch.empty(B, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(0)
    for G in (64, 1024):
        grid = capi.vegas_refine(vegas.uniform_grid([0.0] * D, [1.0] * D, G), rng.random((D, G)) + 0.1, 1.0)
        d_grid = torch.from_numpy(grid).to(dev)
        base = median_ms(lambda: capi.vegas_sample_device(d_grid.data_ptr(), D, G, None, 7, 0, x.data_ptr(), 1, B, jac.data_ptr(), 0, B, st),
                         a.reps)
        rows[f"sample_d17_g{G}_ms"] = base
        for n_bin in (64, 4096, 16384):
            dm = vegas.DiscreteMap(capi.vegas_refine_discrete(vegas.uniform_cdf(n_bin), rng.random(n_bin) + 0.1, 1.0, 0.05),
                                   ext=rng.random((n_bin, 3)), ext_col=[D, D + 1, D + 2], device=dev)
            key = f"sample_discrete_d17_g{G}_b{n_bin}"
            rows[key + "_ms"] = median_ms(lambda: capi.vegas_sample_device_discrete(
                d_grid.data_ptr(), D, G, None, dm.d_cdf.data_ptr(), n_bin, 0, dm.d_ext.data_ptr(), dm.ext_col, 7, 0, x.data_ptr(), 1, B,
                jac.data_ptr(), bins.data_ptr(), 0, B, st), a.reps)
            rows[key + "_vs_sample"] = rows[key + "_ms"] / base
    out["parquet_sigma4"] = rows
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
