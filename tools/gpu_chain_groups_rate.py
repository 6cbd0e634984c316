"""One step of the Markov chain with weight groups against the plain chain step in the same session (fdg.h:
fdg_chain_propose_device + fdg_mc_chain_step_device_grouped against fdg_chain_propose_device + fdg_mc_chain_step_device).  The
workload of tools/gpu_chain_rate.py: parquet_sigma4 (R = 4, the pairs of times (1, 1) .. (1, 4)), the Monte-Carlo form, the uniform
map over the internal momenta and times (D = 15, G = 64), 1e8 walkers when the state with the largest sum fits the device and the
largest of 5e7, 2e7, 1e7 otherwise (``walkers`` in the output says which).  One process; per row one first placement
(FDG_CHAIN_INIT) of its own kind, one warm-up call, then the median and min - max of --reps timed calls (events around each call),
every variable redrawn, FDG_CHAIN_MEASURE set:

  plain_step     propose + the plain step: the yardstick
  grp1_step      propose + the grouped step with one group, a full mask and no factors (the plain step's bits)
  grp4_step      propose + the grouped step with 4 groups, root k in group k, nested masks of 3, 7, 11 and 15 variables, and the
                 factors rho_g = 1 / mean |jac_g s_g| of the first placement
  grp1_step_f8   the two grouped rows with the Matsubara projection at n_freq = 8
  grp4_step_f8

    timeout -k 10 600 python tools/gpu_chain_groups_rate.py --out profiles/chain_groups_rate_parquet_sigma4.json

Nothing is asserted: there is no bar on this kernel's speed."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import feynmandiagram_jl_amd as fd  # noqa: E402
from feynmandiagram_jl_amd import capi, vegas, workloads  # noqa: E402
from gpu_chain_rate import timed  # noqa: E402

N_FREQ = 8


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
    tin, tout = workloads.root_times(name)
    cin, cout = [nk + int(i) - 1 for i in tin], [nk + int(i) - 1 for i in tout]
    n_sum = 2 * N_FREQ * R + 1
    per_walker = 8 * (2 * C + 2 * D + R + 1 + n_sum + 2) + 4             # x, xp, fac, facp, root, a, the largest sum, two temporaries, n_accept
    free, _total = torch.cuda.mem_get_info(dev)
    B = next((int(n) // 64 * 64 for n in (a.walkers, 5e7, 2e7, 1e7) if n <= a.walkers and per_walker * int(n) <= 0.8 * free), int(1e7) // 64 * 64)
    f64 = dict(dtype=torch.float64, device=dev)
    x, xp = torch.zeros((C, B), **f64), torch.empty((C, B), **f64)
    x[0] = kF
    fac, facp = torch.ones((D, B), **f64), torch.empty((D, B), **f64)
    root, av, total = torch.zeros((R, B), **f64), torch.zeros(B, **f64), torch.zeros((n_sum, B), **f64)
    n_acc = torch.zeros(B, dtype=torch.int32, device=dev)
    off, full = [0], (1 << D) - 1
    layouts = {1: ([0] * R, [tuple(range(D))]), 4: (list(range(R)), [tuple(range((g + 1) * D // 4)) for g in range(4)])}
    assert R == 4 and layouts[4][1][-1] == tuple(range(D))

    def step(flags, gamma, desc, groups, offset=None):
        if offset is None:
            off[0] += B
            offset = off[0]
        capi.chain_propose_device(grid.data_ptr(), D, G, col, C, full, 7, offset, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B,
                                  facp.data_ptr(), B, st)
        tail = (facp.data_ptr(), C, D, None, gamma, 7, offset, flags, x.data_ptr(), B, fac.data_ptr(), root.data_ptr(), av.data_ptr(),
                total.data_ptr(), n_acc.data_ptr())
        if groups is None:
            f.handle.mc_chain_step_device(xp.data_ptr(), B, kF, beta, lam, *tail, B, st)
        else:
            f.handle.mc_chain_step_device_grouped(xp.data_ptr(), B, kF, beta, lam, *tail, desc, groups, B, st)

    rows = {"walkers": B, "n_dim": D, "n_grid": G, "n_col": C, "n_root": R, "state_bytes_per_walker": per_walker}

    def put(key, n_group, n_freq):
        desc, keep = (None, None) if n_freq == 0 else capi.make_chain_matsubara(list(range(-(n_freq // 2), n_freq - n_freq // 2)), True, 0, cin,
                                                                                cout, beta)
        groups, gkeep, rho = None, None, None
        if n_group:
            root_group, var_sets = layouts[n_group]
            groups, gkeep = capi.make_chain_groups(root_group, var_sets, None)
        off[0] += B
        step(capi.FDG_CHAIN_INIT, 1.0, desc, groups, off[0])
        if n_group > 1:                                       # the driver's factors, then the placement again on the same counters
            rho = []
            for g in range(n_group):
                jg = fac[var_sets[g][0]].clone()
                for d in var_sets[g][1:]:
                    jg *= fac[d]
                rho.append(1.0 / float(jg.mul_(root[g]).abs_().mean().item()))
            del jg
            groups, gkeep = capi.make_chain_groups(root_group, var_sets, rho)
            step(capi.FDG_CHAIN_INIT, 1.0, desc, groups, off[0])
        torch.cuda.synchronize()
        gamma = float(av.mean().item())
        total.zero_()
        before = int(n_acc.sum(dtype=torch.int64).item())
        med, lo, hi = timed(lambda: step(capi.FDG_CHAIN_MEASURE, gamma, desc, groups), a.reps)
        rate = (int(n_acc.sum(dtype=torch.int64).item()) - before) / (B * (a.reps + 1))
        scale = 1e8 / B
        rows[key] = {"n_group": n_group, "n_freq": n_freq, "reweight": rho, "gamma": gamma, "acceptance": rate, "ms_per_1e8": med * scale,
                     "ms_per_1e8_min": lo * scale, "ms_per_1e8_max": hi * scale, "sum_columns": 2 * n_freq * R + 1 if n_freq else R + 1}
        if "plain_step" in rows and key != "plain_step":
            rows[key]["vs_plain_step"] = med * scale / rows["plain_step"]["ms_per_1e8"]

    put("plain_step", 0, 0)
    put("grp1_step", 1, 0)
    put("grp4_step", 4, 0)
    put("grp1_step_f%d" % N_FREQ, 1, N_FREQ)
    put("grp4_step_f%d" % N_FREQ, 4, N_FREQ)
    out = {"tool": "gpu_chain_groups_rate", "device": torch.cuda.get_device_name(0), name: rows,
           "command": "python tools/gpu_chain_groups_rate.py --reps %d" % a.reps}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
