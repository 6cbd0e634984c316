"""The observables pass against the moments call, on a tile-major batch (fdg.h: fdg_accumulate_device_observables).  parquet_sigma4
(the headline, L = 84, R = 4) at 1e8 samples in one box; n_obs = 2 and 16 dense random rows, n_bin = 1 (no bin vector) and 64 (uniform
bins).  Per n_bin, in one process: accumulate_moments (the yardstick), the grouped call with one group and no observables (the same
call without ob: the ungrouped kernels on the ungrouped plan), the observables call alone (no per-root moments), and the observables
call beside the per-root moments; then the frequency-observables call alone (fdg_accumulate_device_freq_observables, no per-root sums;
external times (1,1) (1,2) (1,3) (1,4)) for M = 2 and 8 dense random rows at n_freq = 1 and 8.  One warm-up call, then the median of
--reps timed calls (events around each call).  Prints ONE JSON line: ms per call, their spread, the ratios to the moments call.

    python tools/gpu_observables_rate.py [--samples 1e8] [--reps 7]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, workloads  # noqa: E402
from gpu_groups_rate import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    name = "parquet_sigma4"
    t = workloads.get(name)
    R = t.n_root
    B = int(a.samples) // 64 * 64
    f = fd.compile_table(t, specialize="isa")
    leaf = torch.empty((B // 64, t.n_leaf, 64), dtype=torch.float64, device=dev)
    capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 1234, 0, st)
    w = torch.rand(B, dtype=torch.float64, device=dev)
    beta = 3.0
    tin, tout = workloads.root_times(name)
    T = torch.rand((4, B), dtype=torch.float64, device=dev).mul_(beta).t()           # component-major, as the sampler writes it
    T[:, 0] = 0.0
    rng = np.random.default_rng(1)
    rows = {"samples": B}
    wg, _keep = capi.make_weight_groups([0] * R, [(0,)], B)
    for n_bin in (1, 64):
        bins = None if n_bin == 1 else torch.randint(0, n_bin, (B,), dtype=torch.int32, device=dev)
        d_bin = 0 if bins is None else bins.data_ptr()
        acc = torch.zeros((n_bin, R), dtype=torch.float64, device=dev)
        acc2 = torch.zeros_like(acc)

        def put(key, fn):
            med, lo, hi = timed(fn, a.reps)
            k = f"bins{n_bin}_{key}"
            rows[k + "_ms"], rows[k + "_ms_min"], rows[k + "_ms_max"] = med, lo, hi
            rows[k + "_vs_moments"] = med / rows[f"bins{n_bin}_moments_ms"]

        put("moments", lambda: f.accumulate_moments(leaf, bins, n_bin, w, acc, acc2, n_sample=B))
        put("grouped_no_obs", lambda: f.handle.accumulate_device_grouped(leaf.data_ptr(), 1, 64, 64 * t.n_leaf, d_bin, 0, n_bin, w.data_ptr(), wg,
                                                                         d_acc=acc.data_ptr(), d_acc2=acc2.data_ptr(), B=B, stream=st))
        for n_obs in (2, 16):
            obs = torch.zeros((n_bin, n_obs), dtype=torch.float64, device=dev)
            cov = torch.zeros((n_bin, n_obs, n_obs), dtype=torch.float64, device=dev)
            coef = rng.uniform(-1.0, 1.0, size=(n_obs, R))
            put(f"obs{n_obs}", lambda: f.accumulate_observables(leaf, coef, bins, n_bin, w, obs, cov, n_sample=B))
            put(f"obs{n_obs}_and_moments", lambda: f.accumulate_observables(leaf, coef, bins, n_bin, w, obs, cov, acc, acc2, n_sample=B))
        for M, n_freq in ((2, 1), (2, 8), (8, 1), (8, 8)):
            freq = list(range(-(n_freq // 2), n_freq - n_freq // 2))
            fobs = torch.zeros((n_bin, n_freq, 2 * M), dtype=torch.float64, device=dev)
            fcov = torch.zeros((n_bin, n_freq, 2 * M, 2 * M), dtype=torch.float64, device=dev)
            coef = rng.uniform(-1.0, 1.0, size=(M, R))
            put(f"fobs{M}_freq{n_freq}", lambda: f.accumulate_freq_observables(leaf, T, freq, tin, tout, beta, coef, True, bins, n_bin, w, fobs, fcov,
                                                                               n_sample=B))
    print(json.dumps({"tool": "gpu_observables_rate", "device": torch.cuda.get_device_name(0), name: rows}), flush=True)


if __name__ == "__main__":
    main()
