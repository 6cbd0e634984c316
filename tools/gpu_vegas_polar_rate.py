"""The polar VEGAS sampler against the sampler it extends (fdg.h: fdg_vegas_sample_device_polar, fdg_vegas_sample_device), in one process.
n_dim = 17 over the 19 columns of parquet_sigma4's Monte-Carlo variables (five loop momenta of three components, four times), 1e8
samples, component-major x, n_grid 64 and 1024, a refined map:
  plain       fdg_vegas_sample_device, variables 0 .. 16 -> columns 0 .. 16
  polar0      fdg_vegas_sample_device_polar with no group: the same bits through the new kernel
  polar5      five groups of three (the five loop momenta: variables 0 .. 14 -> columns 0 .. 14) and two plain variables (two times)
  polar4      four groups of three (loop momenta 2 .. 5; variables 0 .. 11 -> columns 3 .. 14) and five plain variables
Prints ONE JSON line: ms per call (medians of --reps calls) and the ratios to `plain`.

    python tools/gpu_vegas_polar_rate.py [--samples 1e8] [--reps 5]
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402


def timed(fn, reps):
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
    z = workloads.leafstates("parquet_sigma4")
    n_loop, n_tau, D = int(z["basis"].shape[1]), int(z["n_tau"]), 17
    C = 3 * n_loop + n_tau
    assert 3 * n_loop <= D <= C
    B = int(a.samples) // 64 * 64
    x = torch.empty((C, B), dtype=torch.float64, device=dev)
    jac = torch.empty(B, dtype=torch.float64, device=dev)
    rows = {"samples": B, "n_dim": D, "columns": C}
    rng = np.random.default_rng(0)
    configs = {
        "polar0": ([], list(range(D))),
        "polar5": ([(3 * g, (3 * g, 3 * g + 1, 3 * g + 2)) for g in range(n_loop)], [None] * (3 * n_loop) + list(range(3 * n_loop, D))),
        "polar4": ([(3 * g, (3 * g + 3, 3 * g + 4, 3 * g + 5)) for g in range(n_loop - 1)],
                   [None] * (3 * n_loop - 3) + [0, 1, 2] + list(range(3 * n_loop, D))),
    }
    for G in (64, 1024):
        for name, (groups, col) in [("plain", ([], list(range(D))))] + list(configs.items()):
            lo, hi = [0.0] * D, [1.0] * D
            for var, cols in groups:
                lo[var:var + 3], hi[var:var + 3] = vegas.ball(10.0 * 1.919, 3, k_min=0.0)
            grid = capi.vegas_refine(vegas.uniform_grid(lo, hi, G), rng.random((D, G)) + 0.1, 1.0)
            assert all(grid[v + 1, -1] == math.pi and grid[v + 2, -1] == 2.0 * math.pi for v, _ in groups)
            d_grid = torch.from_numpy(grid).to(dev)
            if name == "plain":
                def call():
                    capi.vegas_sample_device(d_grid.data_ptr(), D, G, col, 7, 0, x.data_ptr(), 1, B, jac.data_ptr(), 0, B, st)
            else:
                def call():
                    capi.vegas_sample_device_polar(d_grid.data_ptr(), D, G, col, 0, 0, 0, 0, None, groups, 7, 0, x.data_ptr(), 1, B,
                                                   jac.data_ptr(), 0, 0, B, st)
            key = f"{name}_g{G}"
            rows[key + "_ms"] = timed(call, a.reps)
            if name != "plain":
                rows[key + "_vs_plain"] = rows[key + "_ms"] / rows[f"plain_g{G}_ms"]
    print(json.dumps({"tool": "gpu_vegas_polar_rate", "device": torch.cuda.get_device_name(0), "parquet_sigma4": rows}), flush=True)


if __name__ == "__main__":
    main()
