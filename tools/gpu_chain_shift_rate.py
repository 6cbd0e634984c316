"""One step of the Markov chain with a local shift move against the same step with a redraw, in the same session (fdg.h:
fdg_chain_propose_device_local with a one-variable shift mask + fdg_mc_chain_step_device against fdg_chain_propose_device with the same
mask as a redraw + fdg_mc_chain_step_device).  The workload of tools/gpu_chain_rate.py: parquet_sigma4 (R = 4), the Monte-Carlo form,
the uniform map with G = 64, D = 15 Cartesian variables.  1e8 walkers when the state fits the device and the largest of 5e7, 2e7, 1e7
otherwise (``walkers`` in the output says which).  One process; per row one first placement (FDG_CHAIN_INIT, every variable redrawn),
one warm-up call, then the median and min - max of --reps timed calls (events around each call), FDG_CHAIN_MEASURE set; and the same
for the propose call alone:

  redraw_step    fdg_chain_propose_device, mask = 1 << --var, + the plain step: the yardstick
  shift_step     fdg_chain_propose_device_local, local_mask = 1 << --var, width --width, + the plain step
  shift0_step    fdg_chain_propose_device_local with local_mask = 0 and mask = 1 << --var (the plain propose's bits) + the plain step

    timeout -k 10 600 python tools/gpu_chain_shift_rate.py --out profiles/chain_shift_rate_parquet_sigma4.json

Nothing is asserted: there is no bar on this kernel's speed.  Not measured here: more than one shifted variable, a trained map, a
larger G, whether shifts lower the error of any workload, more than one GPU."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--var", type=int, default=0)
    ap.add_argument("--width", type=float, default=0.1)
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
    box = torch.from_numpy(vegas.uniform_grid([-2.0] * (nk - dim) + [0.0] * (n_tau - 1), [2.0] * (nk - dim) + [beta] * (n_tau - 1), G)).to(dev)
    per_walker = 8 * (2 * C + 2 * D + R + 1 + R + 1 + 2) + 4            # x, xp, fac, facp, root, a, sum, two temporaries, n_accept
    free, _total = torch.cuda.mem_get_info(dev)
    B = next((int(n) // 64 * 64 for n in (a.walkers, 5e7, 2e7, 1e7) if n <= a.walkers and per_walker * int(n) <= 0.8 * free), int(1e7) // 64 * 64)
    f64 = dict(dtype=torch.float64, device=dev)
    x, xp = torch.zeros((C, B), **f64), torch.empty((C, B), **f64)
    fac, facp = torch.ones((D, B), **f64), torch.empty((D, B), **f64)
    root, av, total = torch.zeros((R, B), **f64), torch.zeros(B, **f64), torch.zeros((R + 1, B), **f64)
    n_acc = torch.zeros(B, dtype=torch.int32, device=dev)
    off, full, one = [0], (1 << D) - 1, 1 << a.var

    def propose(kind, offset, place=False):
        head = (box.data_ptr(), D, G, col, C)
        tail = (7, offset, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B, facp.data_ptr())
        if place or kind == "redraw":
            capi.chain_propose_device(*head, full if place else one, *tail, B, st)
        elif kind == "shift":
            capi.chain_propose_device_local(*head, 0, one, a.width, *tail, B=B, stream=st)
        else:
            capi.chain_propose_device_local(*head, one, 0, None, *tail, B=B, stream=st)

    def step(kind, flags, gamma, offset=None):
        if offset is None:
            off[0] += B
            offset = off[0]
        propose(kind, offset, bool(flags & capi.FDG_CHAIN_INIT))
        f.handle.mc_chain_step_device(xp.data_ptr(), B, kF, beta, lam, facp.data_ptr(), C, D, None, gamma, 7, offset, flags, x.data_ptr(), B,
                                      fac.data_ptr(), root.data_ptr(), av.data_ptr(), total.data_ptr(), n_acc.data_ptr(), B, st)

    rows = {"walkers": B, "n_dim": D, "n_grid": G, "n_col": C, "n_root": R, "var": a.var, "width": a.width, "state_bytes_per_walker": per_walker}

    def put(key, kind):
        x.zero_()
        x[0] = kF
        fac.fill_(1.0)
        off[0] += B
        step(kind, capi.FDG_CHAIN_INIT, 1.0, off[0])
        torch.cuda.synchronize()
        gamma = float(av.mean().item())
        total.zero_()
        before = int(n_acc.sum(dtype=torch.int64).item())
        med, lo, hi = timed(lambda: step(kind, capi.FDG_CHAIN_MEASURE, gamma), a.reps)
        rate = (int(n_acc.sum(dtype=torch.int64).item()) - before) / (B * (a.reps + 1))
        pmed, plo, phi = timed(lambda: propose(kind, off[0]), a.reps)
        scale = 1e8 / B
        rows[key] = {"gamma": gamma, "acceptance": rate, "ms_per_1e8": med * scale, "ms_per_1e8_min": lo * scale, "ms_per_1e8_max": hi * scale,
                     "propose_ms_per_1e8": pmed * scale, "propose_ms_per_1e8_min": plo * scale, "propose_ms_per_1e8_max": phi * scale}
        if "redraw_step" in rows and key != "redraw_step":
            rows[key]["vs_redraw_step"] = med * scale / rows["redraw_step"]["ms_per_1e8"]
            rows[key]["propose_vs_redraw"] = pmed / (rows["redraw_step"]["propose_ms_per_1e8"] / scale)

    put("redraw_step", "redraw")
    put("shift_step", "shift")
    put("shift0_step", "shift0")
    out = {"tool": "gpu_chain_shift_rate", "device": torch.cuda.get_device_name(0), name: rows,
           "not_measured": ["more than one shifted variable", "a trained map", "a larger G", "the error of any workload", "more than one GPU"],
           "command": "python tools/gpu_chain_shift_rate.py --reps %d" % a.reps}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
