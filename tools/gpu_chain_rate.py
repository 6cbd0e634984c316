"""One step of the Markov chain on the VEGAS map against the plain iteration on the same number of evaluations (fdg.h:
fdg_chain_propose_device + fdg_mc_chain_step_device against fdg_vegas_sample_device + fdg_mc_accumulate_device_vegas, the calls the
plain driver makes and this change does not touch).  parquet_sigma4 (the headline, R = 4), the Monte-Carlo form, the uniform map over
the internal momenta and times (D = 15 variables, G = 64), 1e8 walkers when the state fits the device and 1e7 otherwise.
One warm-up call, then the median of --reps timed calls (events around each call), everything in one process:

  plain         fdg_vegas_sample_device + fdg_mc_accumulate_device_vegas
  step_all      propose with every variable + step with FDG_CHAIN_MEASURE
  step_one      propose with one variable + step with FDG_CHAIN_MEASURE
  reduce        fdg_chain_reduce_device

and, with --variance, the variance per evaluation of chain_integrate against vegas_integrate on the GV self-energy of
tests/test_chain_accumulate.py (printed and recorded, not asserted).

    timeout -k 10 600 python tools/gpu_chain_rate.py --variance --out profiles/chain_rate_parquet_sigma4.json

Under ``rocprofv3 --kernel-trace --stats -- python tools/gpu_chain_rate.py --only step_all --reps 3 --walkers 1e7`` the kernel statistics
give the split of a step between the evaluation, fdg_chain_propose and fdg_chain_select (a run of its own, no counters with it).
``select_bytes_per_walker`` is what the select kernel must move per walker at the measured acceptance: it reads x', fac', the R
proposal roots, a and the R + 1 sums, and writes the R + 1 sums and, where the proposal is accepted, x, fac, root and a."""
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


def variance_on_gv(dev):
    """chain_integrate against vegas_integrate on gv_sigma4 at the sizes of the test: (stderr^2 * evaluations) of each"""
    z = dict(np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    dim, n_loop, n_tau = 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam = 1.919, 3.0, 1.2
    nk, C = n_loop * dim, n_loop * dim + n_tau
    col = list(range(dim, nk)) + list(range(nk + 1, C))
    lo, hi = [-2.0] * (nk - dim) + [0.0] * (n_tau - 1), [2.0] * (nk - dim) + [beta] * (n_tau - 1)
    fixed = np.zeros(C)
    fixed[0] = kF
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    f = fd.compile_table(t, specialize="isa")
    ref = vegas.vegas_integrate(f, tab, lo, hi, col, kF, beta, lam, n_iter=6, n_discard=3, n_sample=200_000, n_grid=16, seed=999, fixed=fixed,
                                device=dev)
    rows = {"vegas_mean": ref.mean.tolist(), "vegas_stderr": ref.stderr.tolist(), "vegas_evaluations": 600_000}
    for grel in (1.0, 4.0, 16.0):
        res = vegas.chain_integrate(f, tab, lo, hi, col, kF, beta, lam, n_walker=20_000, n_step=40, n_therm=16, gamma_rel=grel, n_warm=3,
                                    n_warm_sample=100_000, n_grid=16, seed=0, fixed=fixed, device=dev)
        n_eval = 20_000 * 41
        rows["chain_gamma_rel_%g" % grel] = {
            "mean": res.mean.tolist(), "stderr": res.stderr.tolist(), "acceptance": res.acceptance, "evaluations": n_eval,
            "variance_per_evaluation_vs_vegas": ((res.stderr ** 2 * n_eval) / (ref.stderr ** 2 * 600_000)).tolist()}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="time this one row: for a profiler pass")
    ap.add_argument("--variance", action="store_true")
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
    acc, acc2, hist = torch.zeros(R, **f64), torch.zeros(R, **f64), torch.zeros((D, G), **f64)
    out9 = torch.zeros(3 * R + 2, **f64)
    off = [0]

    def step(mask, flags, gamma):
        off[0] += B
        capi.chain_propose_device(grid.data_ptr(), D, G, col, C, mask, 7, off[0], x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B,
                                  facp.data_ptr(), B, st)
        f.handle.mc_chain_step_device(xp.data_ptr(), B, kF, beta, lam, facp.data_ptr(), C, D, None, gamma, 7, off[0], flags, x.data_ptr(), B,
                                      fac.data_ptr(), root.data_ptr(), av.data_ptr(), total.data_ptr(), n_acc.data_ptr(), B, st)

    def plain():
        off[0] += B
        capi.vegas_sample_device(grid.data_ptr(), D, G, col, 7, off[0], xp.data_ptr(), 1, B, av.data_ptr(), 0, B, st)
        f.handle.mc_accumulate_device_vegas(xp.data_ptr(), 1, B, xp.data_ptr() + 8 * nk * B, 1, B, kF, beta, lam, av.data_ptr(), None, 7, off[0],
                                            D, G, acc.data_ptr(), acc2.data_ptr(), hist.data_ptr(), B, st)

    rows = {"walkers": B, "n_dim": D, "n_grid": G, "n_col": C, "state_bytes_per_walker": per_walker}
    xp.copy_(x)

    def put(key, fn, base=None):
        if a.only and key != a.only:
            return
        med, lo, hi = timed(fn, a.reps)
        rows[key + "_ms"], rows[key + "_ms_min"], rows[key + "_ms_max"] = med, lo, hi
        if base and base + "_ms" in rows:
            rows[key + "_vs_" + base] = med / rows[base + "_ms"]

    put("plain", plain)
    step((1 << D) - 1, capi.FDG_CHAIN_INIT, 1.0)
    torch.cuda.synchronize()
    gamma = float(av.mean().item())
    rows["gamma"] = gamma
    before = int(n_acc.sum(dtype=torch.int64).item())
    put("step_all", lambda: step((1 << D) - 1, capi.FDG_CHAIN_MEASURE, gamma), "plain")
    if "step_all_ms" in rows:
        rate = (int(n_acc.sum(dtype=torch.int64).item()) - before) / (B * (a.reps + 1))
        rows["step_all_acceptance"] = rate
        rows["select_bytes_per_walker"] = 8 * ((C + D + R + 1 + R + 1) + (R + 1) + rate * (C + D + R + 1)) + 4 * rate
    put("step_one", lambda: step(1, capi.FDG_CHAIN_MEASURE, gamma), "plain")
    put("reduce", lambda: capi.chain_reduce_device(total.data_ptr(), R, B, out9.data_ptr(), st))
    del x, xp, fac, facp, root, av, total, n_acc
    out = {"tool": "gpu_chain_rate", "device": torch.cuda.get_device_name(0), name: rows,
           "command": "python tools/gpu_chain_rate.py --variance --reps %d" % a.reps}
    if a.variance:
        out["gv_sigma4_variance"] = variance_on_gv(dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
