"""The chain's reduction with observables against the existing one (fdg.h: fdg_chain_reduce_device_observables against
fdg_chain_reduce_device, which is the yardstick and unchanged code).  parquet_sigma4 (R = 4), the Monte-Carlo form, the walkers' sums
[R + 1][n_walker] of a chain set up as tools/gpu_chain_rate.py sets it up (the placement and two measured steps fill them), 1e8
walkers when the state fits the device and 1e7 otherwise.  One warm-up call, then the median of --reps timed calls (events around
each call), everything in one process:

  reduce        fdg_chain_reduce_device: 3 R + 2 workgroups, every column read three times
  obs_unit      the new entry, one unit row per root: S, Q and X of the yardstick and the cross moments between the roots beside them
  obs_sum       the new entry, one row that sums all roots
  obs_dense8    the new entry, eight dense rows (the instance of nine slots)
  obs_dense16   the new entry, sixteen dense rows (the instance whose pairs are split over three workgroups)

    timeout -k 10 600 python tools/gpu_chain_reduce_rate.py --out profiles/chain_reduce_rate_parquet_sigma4.json

Under ``rocprofv3 --kernel-trace --stats -- python tools/gpu_chain_reduce_rate.py --only obs_unit --reps 3`` the kernel statistics give
the split between fdg_chain_obs_partial and fdg_chain_obs_final (a run of its own, no counters with it).  ``*_gbs`` is the rate at
which the columns a call must read once, (live columns + 1) * 8 bytes per walker, go by."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402
from gpu_chain_rate import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="time this one row: for a profiler pass")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    name = "parquet_sigma4"
    t, z = workloads.get(name), workloads.leafstates(name)
    R, dim, n_loop, n_tau = t.n_root, 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam = 1.919, 3.0, 1.2
    nk, C = n_loop * dim, n_loop * dim + n_tau
    col = list(range(dim, nk)) + list(range(nk + 1, C))
    D, G = len(col), 64
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    grid = torch.from_numpy(vegas.uniform_grid([-2.0] * (nk - dim) + [0.0] * (n_tau - 1), [2.0] * (nk - dim) + [beta] * (n_tau - 1), G)).to(dev)
    B = int(a.walkers) // 64 * 64
    per_walker = 8 * (2 * C + 2 * D + R + 1 + R + 1) + 4                 # x, xp, fac, facp, root, a, sum, n_accept
    free, _total = torch.cuda.mem_get_info(dev)
    if per_walker * B > 0.8 * free:
        B = int(1e7) // 64 * 64
    f64 = dict(dtype=torch.float64, device=dev)
    x, xp = torch.zeros((C, B), **f64), torch.empty((C, B), **f64)
    x[0] = kF
    fac, facp = torch.ones((D, B), **f64), torch.empty((D, B), **f64)
    root, av, total = torch.zeros((R, B), **f64), torch.zeros(B, **f64), torch.zeros((R + 1, B), **f64)
    n_acc = torch.zeros(B, dtype=torch.int32, device=dev)
    xp.copy_(x)
    gamma = 1.0
    for i, flags in enumerate((capi.FDG_CHAIN_INIT, capi.FDG_CHAIN_MEASURE, capi.FDG_CHAIN_MEASURE)):
        capi.chain_propose_device(grid.data_ptr(), D, G, col, C, (1 << D) - 1, 7, i * B, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B,
                                  facp.data_ptr(), B, st)
        f.handle.mc_chain_step_device(xp.data_ptr(), B, kF, beta, lam, facp.data_ptr(), C, D, None, gamma, 7, i * B, flags, x.data_ptr(), B,
                                      fac.data_ptr(), root.data_ptr(), av.data_ptr(), total.data_ptr(), n_acc.data_ptr(), B, st)
        if i == 0:
            torch.cuda.synchronize()
            gamma = float(av.mean().item())
    torch.cuda.synchronize()
    del x, xp, fac, facp, root, av, n_acc
    rows = {"walkers": B, "n_root": R, "gamma": gamma, "groups": capi.FDG_CHAIN_OBS_GROUPS}
    out_old = torch.zeros(3 * R + 2, **f64)
    dense = np.random.default_rng(0).uniform(0.5, 2.0, size=(capi.FDG_CHAIN_OBS_MAX, R))
    cases = {"obs_unit": np.eye(R), "obs_sum": np.ones((1, R)), "obs_dense8": dense[:8], "obs_dense16": dense}
    work = torch.empty(capi.chain_reduce_observables_work_bytes(capi.FDG_CHAIN_OBS_MAX, R), dtype=torch.uint8, device=dev)

    def put(key, fn, columns):
        if a.only and key != a.only:
            return
        med, lo, hi = timed(fn, a.reps)
        rows[key + "_ms"], rows[key + "_ms_min"], rows[key + "_ms_max"] = med, lo, hi
        rows[key + "_gbs"] = 8.0 * columns * B / (med * 1e6)
        if key != "reduce" and "reduce_ms" in rows:
            rows[key + "_vs_reduce"] = med / rows["reduce_ms"]

    put("reduce", lambda: capi.chain_reduce_device(total.data_ptr(), R, B, out_old.data_ptr(), st), R + 1)
    for key, coef in cases.items():
        M = coef.shape[0]
        out = torch.zeros((M + 1) + (M + 1) * (M + 2) // 2, **f64)
        put(key, lambda: capi.chain_reduce_observables_device(total.data_ptr(), B, 0, R, R, coef, out.data_ptr(), work.data_ptr(), st), R + 1)
        if key == "obs_unit" and "reduce_ms" in rows and key + "_ms" in rows:
            # the same figures by both entries (each was called reps + 1 times into its output): S_R and X_0
            n = a.reps + 1
            o, u = out_old.cpu().numpy() / n, out.cpu().numpy() / n
            rows["check_S_R"] = [float(o[R]), float(u[R])]
            rows["check_X_0"] = [float(o[2 * R + 2]), float(u[R + 1 + R])]
    res = {"tool": "gpu_chain_reduce_rate", "device": torch.cuda.get_device_name(0), name: rows,
           "command": "python tools/gpu_chain_reduce_rate.py --reps %d" % a.reps}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
