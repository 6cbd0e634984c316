"""Weight groups against the ungrouped VEGAS accumulate call, on a tile-major batch (fdg.h: fdg_accumulate_device_grouped,
fdg_vegas_sample_device_grouped).  parquet_sigma4 (the headline, L = 84, R = 4) at 1e8 samples in one box, D = 17 variables, G = 64:
accumulate_vegas (the yardstick), the grouped call with one group and a full mask (the same kernels on the same plan: any gap beyond
the run's own min-max spread is to be explained), and the grouped call with four groups, root k in group k, nested masks.  Then the
samplers: fdg_vegas_sample_device against the grouped sampler with one and with four groups.  One warm-up call, then the median of
--reps timed calls (events around each call), all in one process.  Prints ONE JSON line: ms per call, their spread, the ratios.

    python tools/gpu_groups_rate.py [--samples 1e8] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402

D, G = 17, 64


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
    w = torch.rand((R, B), dtype=torch.float64, device=dev)
    rows = {"samples": B, "n_dim": D, "n_grid": G}

    def put(key, fn):
        med, lo, hi = timed(fn, a.reps)
        rows[key + "_ms"], rows[key + "_ms_min"], rows[key + "_ms_max"] = med, lo, hi

    acc = torch.zeros((1, R), dtype=torch.float64, device=dev)
    acc2, hist = torch.zeros_like(acc), torch.zeros((D, G), dtype=torch.float64, device=dev)
    put("vegas", lambda: f.accumulate_vegas(leaf, w[0], hist, 7, 0, D, G, acc=acc, acc2=acc2, n_sample=B))
    nested = [tuple(range(D - 4 * (R - 1 - k))) for k in range(R)]             # 5, 9, 13, 17 variables
    for key, rg, sets in (("grouped_1", [0] * R, [tuple(range(D))]), ("grouped_4", list(range(R)), nested)):
        wg, _keep = capi.make_weight_groups(rg, sets, B)
        put(key, lambda: f.handle.accumulate_device_grouped(leaf.data_ptr(), 1, 64, 64 * t.n_leaf, 0, 0, 1, w.data_ptr(), wg, None, None, 7, 0, D, G,
                                                            acc.data_ptr(), acc2.data_ptr(), hist.data_ptr(), 0, B, st))
        rows[key + "_vs_vegas"] = rows[key + "_ms"] / rows["vegas_ms"]
    del leaf
    # the samplers: D columns component-major, as the driver lays them out
    grid = torch.from_numpy(vegas.uniform_grid([0.0] * D, [1.0] * D, G)).to(dev)
    x = torch.empty((D, B), dtype=torch.float64, device=dev)
    jac = torch.empty((R, B), dtype=torch.float64, device=dev)
    put("sample", lambda: capi.vegas_sample_device(grid.data_ptr(), D, G, None, 7, 0, x.data_ptr(), 1, B, jac.data_ptr(), 0, B, st))
    for key, sets in (("sample_grouped_1", [tuple(range(D))]), ("sample_grouped_4", nested)):
        put(key, lambda: capi.vegas_sample_device_grouped(grid.data_ptr(), D, G, None, 0, 1, 0, 0, None, None, sets, B, 7, 0, x.data_ptr(), 1, B,
                                                          jac.data_ptr(), 0, 0, B, st))
        rows[key + "_vs_sample"] = rows[key + "_ms"] / rows["sample_ms"]
    print(json.dumps({"tool": "gpu_groups_rate", "device": torch.cuda.get_device_name(0), name: rows}), flush=True)


if __name__ == "__main__":
    main()
