"""The frequency-observables pass against the per-root projection and the moments call, on a tile-major batch (fdg.h:
fdg_accumulate_device_freq_observables).  parquet_sigma4 (the headline, L = 84, R = 4, external times (1,1) (1,2) (1,3) (1,4)) at 1e8
samples in one box; (M, n_freq) = (2, 1), (2, 16), (8, 16) dense random rows, n_bin = 1 (no bin vector) and 64 (uniform bins).  Per
n_bin, in one process: accumulate_moments (the yardstick), accumulate_matsubara with the same frequencies (what a caller had before:
one mean and error bar per root), and the frequency-observables call alone (no per-root sums).  One warm-up call, then the median of
--reps timed calls (events around each call).  Prints ONE JSON line: ms per call, their spread, the ratios to the moments call and to
the projection with the same frequencies.

    python tools/gpu_freq_observables_rate.py [--samples 1e8] [--reps 7]
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
from gpu_matsubara_rate import timed  # noqa: E402


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
    beta, n_tau = 3.0, 4
    tin, tout = workloads.root_times(name)
    T = torch.rand((n_tau, B), dtype=torch.float64, device=dev).mul_(beta).t()       # component-major, as the sampler writes it
    T[:, 0] = 0.0
    rng = np.random.default_rng(1)
    rows = {"samples": B}
    for n_bin in (1, 64):
        bins = None if n_bin == 1 else torch.randint(0, n_bin, (B,), generator=torch.Generator(device=dev).manual_seed(n_bin), device=dev,
                                                     dtype=torch.int32)
        acc = torch.zeros((n_bin, R), dtype=torch.float64, device=dev)
        acc2 = torch.zeros_like(acc)

        def put(key, fn, against=()):
            med, lo, hi = timed(fn, a.reps)
            k = f"bins{n_bin}_{key}"
            rows[k + "_ms"], rows[k + "_ms_min"], rows[k + "_ms_max"] = med, lo, hi
            for other in against:
                rows[f"{k}_vs_{other}"] = med / rows[f"bins{n_bin}_{other}_ms"]
            print(k, med, flush=True, file=sys.stderr)

        put("moments", lambda: f.accumulate_moments(leaf, bins, n_bin, w, acc, acc2, n_sample=B))
        for n_freq in (1, 16):
            freq = list(range(-(n_freq // 2), n_freq - n_freq // 2))
            sums = torch.zeros((4, n_bin, n_freq, R), dtype=torch.float64, device=dev)
            put(f"matsubara_freq{n_freq}", lambda: f.accumulate_matsubara(leaf, T, freq, tin, tout, beta, True, bins, n_bin, w, sums=sums, n_sample=B),
                ("moments",))
        for M, n_freq in ((2, 1), (2, 16), (8, 16)):
            freq = list(range(-(n_freq // 2), n_freq - n_freq // 2))
            fobs = torch.zeros((n_bin, n_freq, 2 * M), dtype=torch.float64, device=dev)
            fcov = torch.zeros((n_bin, n_freq, 2 * M, 2 * M), dtype=torch.float64, device=dev)
            coef = rng.uniform(-1.0, 1.0, size=(M, R))
            put(f"fobs{M}_freq{n_freq}", lambda: f.accumulate_freq_observables(leaf, T, freq, tin, tout, beta, coef, True, bins, n_bin, w, fobs, fcov,
                                                                               n_sample=B), ("moments", f"matsubara_freq{n_freq}"))
    print(json.dumps({"tool": "gpu_freq_observables_rate", "device": torch.cuda.get_device_name(0), name: rows}), flush=True)


if __name__ == "__main__":
    main()
