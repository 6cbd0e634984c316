"""The stratified grouped calls against the calls they combine, on a tile-major batch (fdg.h: fdg_vegas_sample_device_strat_grouped,
fdg_accumulate_device_strat_grouped).  parquet_sigma4 (the headline, L = 84, R = 4) at 1e8 samples in one box, D = 17 variables, G = 64,
H = 1 (one stratum per variable, every sample in hypercube 0) and H = 2^17 (two strata per variable, the uniform allocation), with one
group (a full mask: the ungrouped kernels on the same plan), four groups (root k in group k, nested masks: 8 columns, one column group of
the per-hypercube pass) and eight groups (the same four and four without a root: 12 columns, two column groups).
Two steps, each a process of its own; within a step everything is timed in the same process:

  accumulate   fdg_accumulate_device_grouped with 1, 4 and 8 groups and fdg_accumulate_device_strat at both H (the yardsticks, untouched
               code), then fdg_accumulate_device_strat_grouped at every (H, groups);
  sample       fdg_vegas_sample_device_grouped with 1 and 4 groups and the stratified sampler at both H, then
               fdg_vegas_sample_device_strat_grouped at every (H, groups), the last with five polar groups of three variables too.

One warm-up call, then the median of --reps timed calls (events around each call).  A step merges its figures into the JSON file --out
(and prints them as one JSON line), so the whole measurement is

    timeout -k 10 600 python tools/gpu_strat_grouped_rate.py --step accumulate --out profiles/strat_grouped_rate_parquet_sigma4.json && \\
    timeout -k 10 300 python tools/gpu_strat_grouped_rate.py --step sample --out profiles/strat_grouped_rate_parquet_sigma4.json

Under ``rocprofv3 --kernel-trace --stats -- python tools/gpu_strat_grouped_rate.py --step accumulate --reps 1 --only sg_h2p17_g4`` the
kernel statistics give the split of one configuration's time between the training pass (fdg_vegas_partials) and the per-hypercube
pass (fdg_strat_partials, fdg_strat_stitch).
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

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402

D, G = 17, 64
STRATA = (("h1", (1,) * D), ("h2p17", (2,) * D))


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
    ap.add_argument("--only", default=None, help="time this one row (and nothing it is compared with): for a profiler pass")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    name = "parquet_sigma4"
    t = workloads.get(name)
    R = t.n_root
    B = int(a.samples) // 64 * 64
    rows = {}

    def put(key, fn, *bases):
        if a.only and key != a.only:
            return
        med, lo, hi = timed(fn, a.reps)
        rows[key + "_ms"], rows[key + "_ms_min"], rows[key + "_ms_max"] = med, lo, hi
        for base in bases:
            if base + "_ms" in rows:
                rows[key + "_vs_" + base] = med / rows[base + "_ms"]

    nested = [tuple(range(D - 4 * (R - 1 - k))) for k in range(R)]             # 5, 9, 13, 17 variables
    groups = (("g1", [0] * R, [tuple(range(D))]), ("g4", list(range(R)), nested), ("g8", list(range(R)), nested + nested))
    starts = {key: capi.strat_allocate(None, None, 0, None, int(np.prod(sv)), B) for key, sv in STRATA}
    if a.step == "accumulate":
        f = fd.compile_table(t, specialize="isa")
        leaf = torch.empty((B // 64, t.n_leaf, 64), dtype=torch.float64, device=dev)
        capi.fill_uniform_device_tiled(leaf.data_ptr(), B, t.n_leaf, 1, 64, 64 * t.n_leaf, 1234, 0, st)
        w = torch.rand((8, B), dtype=torch.float64, device=dev)
        acc = torch.zeros((1, R), dtype=torch.float64, device=dev)
        acc2, hist = torch.zeros_like(acc), torch.zeros((D, G), dtype=torch.float64, device=dev)
        lf = (leaf.data_ptr(), 1, 64, 64 * t.n_leaf)
        wgs = {gk: capi.make_weight_groups(rg, sets, B) for gk, rg, sets in groups}
        for gk, _, _ in groups:
            put("grouped_" + gk, lambda: f.handle.accumulate_device_grouped(*lf, 0, 0, 1, w.data_ptr(), wgs[gk][0], None, None, 7, 0, D, G,
                                                                            acc.data_ptr(), acc2.data_ptr(), hist.data_ptr(), 0, B, st))
        for hk, sv in STRATA:
            H = int(np.prod(sv))
            counts = torch.from_numpy(np.diff(starts[hk])).to(dev)
            cube = torch.repeat_interleave(torch.arange(H, dtype=torch.int32, device=dev), counts)
            cs = torch.zeros((2, H, R + 8), dtype=torch.float64, device=dev)
            put("strat_" + hk, lambda: f.handle.accumulate_device_strat(*lf, w.data_ptr(), None, 7, 0, D, G, acc.data_ptr(), acc2.data_ptr(),
                                                                        hist.data_ptr(), sv, cube.data_ptr(), cs[0].data_ptr(),
                                                                        cs[1].data_ptr(), B, st))
            for gk, _, _ in groups:
                put("sg_%s_%s" % (hk, gk),
                    lambda: f.handle.accumulate_device_strat_grouped(*lf, w.data_ptr(), None, 7, 0, D, G, acc.data_ptr(), acc2.data_ptr(),
                                                                     hist.data_ptr(), sv, cube.data_ptr(), cs[0].data_ptr(), cs[1].data_ptr(),
                                                                     wgs[gk][0], B, st), "grouped_" + gk, "strat_" + hk)
            del cube, cs
    else:
        grid = torch.from_numpy(vegas.uniform_grid([0.0] * D, [1.0] * D, G)).to(dev)
        x = torch.empty((D, B), dtype=torch.float64, device=dev)
        jac = torch.empty((R, B), dtype=torch.float64, device=dev)
        cube = torch.empty(B, dtype=torch.int32, device=dev)
        sample_groups = groups[:2]
        for gk, _, sets in sample_groups:
            put("sample_grouped_" + gk, lambda: capi.vegas_sample_device_grouped(grid.data_ptr(), D, G, None, 0, 1, 0, 0, None, None, sets, B, 7,
                                                                                 0, x.data_ptr(), 1, B, jac.data_ptr(), 0, 0, B, st))
        # five balls: variables 3 g .. 3 g + 2 are (k, theta, phi) -> the same three columns; variables 15, 16 stay free
        pgrid = torch.from_numpy(vegas.uniform_grid([0.0] * D, ([1.0, math.pi, 2.0 * math.pi] * 5) + [1.0, 1.0], G)).to(dev)
        balls = [(3 * g, (3 * g, 3 * g + 1, 3 * g + 2)) for g in range(5)]
        pcol = [None] * 15 + [15, 16]
        pmasks = [tuple(range(3 * (k + 2))) for k in range(R - 1)] + [tuple(range(D))]       # 2, 3, 4 balls, then everything
        put("sample_grouped_g4_polar5", lambda: capi.vegas_sample_device_grouped(pgrid.data_ptr(), D, G, pcol, 0, 1, 0, 0, None, balls, pmasks, B,
                                                                                 7, 0, x.data_ptr(), 1, B, jac.data_ptr(), 0, 0, B, st))
        for hk, sv in STRATA:
            d_start = torch.from_numpy(starts[hk]).to(dev)
            put("sample_strat_" + hk, lambda: capi.vegas_sample_device_strat(grid.data_ptr(), D, G, None, sv, d_start.data_ptr(), 7, 0,
                                                                             x.data_ptr(), 1, B, jac.data_ptr(), cube.data_ptr(), 0, B, st))
            for gk, _, sets in sample_groups:
                put("sample_sg_%s_%s" % (hk, gk),
                    lambda: capi.vegas_sample_device_strat_grouped(grid.data_ptr(), D, G, None, None, sets, B, sv, d_start.data_ptr(), 7, 0,
                                                                   x.data_ptr(), 1, B, jac.data_ptr(), cube.data_ptr(), 0, B, st),
                    "sample_grouped_" + gk, "sample_strat_" + hk)
            put("sample_sg_%s_g4_polar5" % hk,
                lambda: capi.vegas_sample_device_strat_grouped(pgrid.data_ptr(), D, G, pcol, balls, pmasks, B, sv, d_start.data_ptr(), 7, 0,
                                                               x.data_ptr(), 1, B, jac.data_ptr(), cube.data_ptr(), 0, B, st),
                "sample_grouped_g4_polar5")
    out = {"tool": "gpu_strat_grouped_rate", "device": torch.cuda.get_device_name(0), name: {"samples": B, "n_dim": D, "n_grid": G}}
    if a.out and os.path.exists(a.out):
        with open(a.out) as fh:
            out = json.load(fh)
    out[name].update(rows)
    out.setdefault("command", "python tools/gpu_strat_grouped_rate.py --step accumulate --reps %d && ... --step sample --reps %d" % (a.reps, a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps({"tool": "gpu_strat_grouped_rate", "step": a.step, name: rows}), flush=True)


if __name__ == "__main__":
    main()
