"""One step of the Markov chain with a discrete external variable against the plain chain step in the same session (fdg.h:
fdg_chain_propose_device_discrete + fdg_mc_chain_step_device_binned against fdg_chain_propose_device + fdg_mc_chain_step_device).  The
workload of tools/gpu_chain_rate.py: parquet_sigma4 (R = 4), the Monte-Carlo form, the uniform map over the internal momenta and times
(D = 15, G = 64); the discrete variable writes the external momentum (columns 0 .. 2) from a table of n_bin rows of length kF, drawn
uniformly.  1e8 walkers when the state with the n_bin = 8 sum fits the device and the largest of 5e7, 2e7, 1e7 otherwise (``walkers``
in the output says which).  One process; per row one first placement (FDG_CHAIN_INIT) of its own kind, one warm-up call, then the median
and min - max of --reps timed calls (events around each call), every variable redrawn, FDG_CHAIN_MEASURE set:

  plain_step     propose + the plain step: the yardstick
  bin1_step      the discrete propose + the binned step with one value (the plain step's bits)
  bin8_step      ... with 8 values, the discrete variable redrawn too

    timeout -k 10 600 python tools/gpu_chain_binned_rate.py --out profiles/chain_binned_rate_parquet_sigma4.json

Nothing is asserted: there is no bar on this kernel's speed."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402
from gpu_chain_rate import timed  # noqa: E402

N_BIN = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
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
    n_sum = N_BIN * R + 1
    per_walker = 8 * (2 * C + 2 * (D + 1) + R + 1 + n_sum + 2) + 12      # x, xp, fac, facp, root, a, the largest sum, two temporaries, n_accept, bin, binp
    free, _total = torch.cuda.mem_get_info(dev)
    B = next((int(n) // 64 * 64 for n in (a.walkers, 5e7, 2e7, 1e7) if n <= a.walkers and per_walker * int(n) <= 0.8 * free), int(1e7) // 64 * 64)
    f64 = dict(dtype=torch.float64, device=dev)
    x, xp = torch.zeros((C, B), **f64), torch.empty((C, B), **f64)
    fac, facp = torch.ones((D + 1, B), **f64), torch.empty((D + 1, B), **f64)
    root, av, total = torch.zeros((R, B), **f64), torch.zeros(B, **f64), torch.zeros((n_sum, B), **f64)
    n_acc = torch.zeros(B, dtype=torch.int32, device=dev)
    bins, binp = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    off, full = [0], (1 << D) - 1

    def table(n_bin):
        """n_bin external momenta of length kF: the first along x (the plain rows' fixed one), the others turned in the x-y plane"""
        phi = 2.0 * np.pi * np.arange(n_bin) / n_bin
        ext = np.stack([kF * np.cos(phi), kF * np.sin(phi), np.zeros(n_bin)], axis=1)
        ext[0] = (kF, 0.0, 0.0)
        return torch.from_numpy(vegas.uniform_cdf(n_bin)).to(dev), torch.from_numpy(np.ascontiguousarray(ext)).to(dev)

    def step(flags, gamma, disc, offset=None):
        if offset is None:
            off[0] += B
            offset = off[0]
        tail = (facp.data_ptr(), C, D, None, gamma, 7, offset, flags, x.data_ptr(), B, fac.data_ptr(), root.data_ptr(), av.data_ptr(),
                total.data_ptr(), n_acc.data_ptr())
        if disc is None:
            capi.chain_propose_device(grid.data_ptr(), D, G, col, C, full, 7, offset, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B,
                                      facp.data_ptr(), B, st)
            f.handle.mc_chain_step_device(xp.data_ptr(), B, kF, beta, lam, *tail, B, st)
        else:
            n_bin, d_cdf, d_ext = disc
            capi.chain_propose_device_discrete(grid.data_ptr(), D, G, col, C, full, 7, offset, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B,
                                               facp.data_ptr(), True, d_cdf.data_ptr(), n_bin, d_ext.data_ptr(), [0, 1, 2], bins.data_ptr(),
                                               binp.data_ptr(), B, st)
            f.handle.mc_chain_step_device_binned(xp.data_ptr(), B, kF, beta, lam, *tail, None, None, n_bin, binp.data_ptr(), bins.data_ptr(), B, st)

    rows = {"walkers": B, "n_dim": D, "n_grid": G, "n_col": C, "n_root": R, "state_bytes_per_walker": per_walker}

    def put(key, n_bin):
        disc = None if n_bin == 0 else (n_bin,) + table(n_bin)
        x.zero_()
        x[0] = kF
        fac.fill_(1.0)
        bins.zero_()
        off[0] += B
        step(capi.FDG_CHAIN_INIT, 1.0, disc, off[0])
        torch.cuda.synchronize()
        gamma = float(av.mean().item())
        total.zero_()
        before = int(n_acc.sum(dtype=torch.int64).item())
        med, lo, hi = timed(lambda: step(capi.FDG_CHAIN_MEASURE, gamma, disc), a.reps)
        rate = (int(n_acc.sum(dtype=torch.int64).item()) - before) / (B * (a.reps + 1))
        scale = 1e8 / B
        rows[key] = {"n_bin": n_bin, "gamma": gamma, "acceptance": rate, "ms_per_1e8": med * scale, "ms_per_1e8_min": lo * scale,
                     "ms_per_1e8_max": hi * scale, "sum_columns": max(n_bin, 1) * R + 1}
        if "plain_step" in rows and key != "plain_step":
            rows[key]["vs_plain_step"] = med * scale / rows["plain_step"]["ms_per_1e8"]

    put("plain_step", 0)
    put("bin1_step", 1)
    put("bin%d_step" % N_BIN, N_BIN)
    out = {"tool": "gpu_chain_binned_rate", "device": torch.cuda.get_device_name(0), name: rows,
           "command": "python tools/gpu_chain_binned_rate.py --reps %d" % a.reps}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
