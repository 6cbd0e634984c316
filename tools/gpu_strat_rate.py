"""Adaptive stratified sampling against the plain VEGAS step, on a tile-major batch (fdg.h: fdg_vegas_sample_device_strat,
fdg_accumulate_device_strat).  parquet_sigma4 (the headline, L = 84, R = 4) at 1e8 samples in one box, D = 17 variables, G = 64.
Two steps, each a process of its own:

  accumulate   accumulate_vegas (the yardstick: the code of the commit before stratification, untouched), then
               fdg_accumulate_device_strat with H = 1 (one stratum per variable, every sample in hypercube 0: one run of 1e8 samples
               through every level of the stitch) and with H = 2^17 (two strata per variable, the uniform allocation);
  sample       fdg_vegas_sample_device, then the stratified sampler with H = 1 and H = 2^17.

One warm-up call, then the median of --reps timed calls (events around each call).  A step merges its figures into the JSON file
--out (and prints them as one JSON line), so the whole measurement is

    timeout -k 10 600 python tools/gpu_strat_rate.py --step accumulate --out profiles/strat_rate_parquet_sigma4.json && \\
    timeout -k 10 300 python tools/gpu_strat_rate.py --step sample --out profiles/strat_rate_parquet_sigma4.json
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

D, G = 17, 64
CASES = (("strat_h1", (1,) * D), ("strat_h2p17", (2,) * D))


def timed(fn, reps):
    """(median, min, max) ms of ``reps`` calls after one warm-up"""
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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("accumulate", "sample"), required=True)
    ap.add_argument("--samples", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    name = "parquet_sigma4"
    t = workloads.get(name)
    R = t.n_root
    B = int(a.samples) // 64 * 64
    rows = {}

    def put(key, fn, base=None):
        med, lo, hi = timed(fn, a.reps)
        rows[key + "_ms"], rows[key + "_ms_min"], rows[key + "_ms_max"] = med, lo, hi
        if base:
            rows[key + "_vs_" + base] = med / rows[base + "_ms"]

    starts = {key: capi.strat_allocate(None, None, 0, None, int(np.prod(sv)), B) for key, sv in CASES}
    if a.step == "accumulate":
        f = fd.compile_table(t, specialize="isa")
        leaf = torch.empty((B // 64, t.n_leaf, 64), dtype=torch.float64, device=dev)
        capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 1234, 0, st)
        w = torch.rand(B, dtype=torch.float64, device=dev)
        acc = torch.zeros((1, R), dtype=torch.float64, device=dev)
        acc2, hist = torch.zeros_like(acc), torch.zeros((D, G), dtype=torch.float64, device=dev)
        put("vegas", lambda: f.accumulate_vegas(leaf, w, hist, 7, 0, D, G, acc=acc, acc2=acc2, n_sample=B))
        for key, sv in CASES:
            H = int(np.prod(sv))
            counts = torch.from_numpy(np.diff(starts[key])).to(dev)
            cube = torch.repeat_interleave(torch.arange(H, dtype=torch.int32, device=dev), counts)
            cs = torch.zeros((2, H, R + 1), dtype=torch.float64, device=dev)
            put(key, lambda: f.handle.accumulate_device_strat(leaf.data_ptr(), 1, 64, 64 * t.n_leaf, w.data_ptr(), None, 7, 0, D, G, acc.data_ptr(),
                                                              acc2.data_ptr(), hist.data_ptr(), sv, cube.data_ptr(), cs[0].data_ptr(),
                                                              cs[1].data_ptr(), B, st), "vegas")
            del cube
    else:
        grid = torch.from_numpy(vegas.uniform_grid([0.0] * D, [1.0] * D, G)).to(dev)
        x = torch.empty((D, B), dtype=torch.float64, device=dev)
        jac = torch.empty(B, dtype=torch.float64, device=dev)
        cube = torch.empty(B, dtype=torch.int32, device=dev)
        put("sample", lambda: capi.vegas_sample_device(grid.data_ptr(), D, G, None, 7, 0, x.data_ptr(), 1, B, jac.data_ptr(), 0, B, st))
        for key, sv in CASES:
            d_start = torch.from_numpy(starts[key]).to(dev)
            put("sample_" + key, lambda: capi.vegas_sample_device_strat(grid.data_ptr(), D, G, None, sv, d_start.data_ptr(), 7, 0, x.data_ptr(), 1, B,
                                                                        jac.data_ptr(), cube.data_ptr(), 0, B, st), "sample")
    out = {"tool": "gpu_strat_rate", "device": torch.cuda.get_device_name(0), name: {"samples": B, "n_dim": D, "n_grid": G}}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)
    out[name].update(rows)
    out.setdefault("command", "python tools/gpu_strat_rate.py --step accumulate --reps %d && ... --step sample --reps %d" % (a.reps, a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps({"tool": "gpu_strat_rate", "step": a.step, name: rows}), flush=True)


if __name__ == "__main__":
    main()
