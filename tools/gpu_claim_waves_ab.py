"""GPU dev tool: from how many resident waves per CU does the claimed one-wave evaluator stream best, and what could prefetching the next tile's
leaves add?  ONE process, ONE allocation (the allocation lottery): the headline batch (tile-major, fdg_batch_alloc_pair or
torch.empty) is evaluated with FDG_ISA_TILE_CLAIM=1 at each FDG_ISA_MEM_WAVES of `waves` ("-": the option unset, the library's rule) by the
library's kernel and, with `nohead`, by the same kernel assembled with FDG_ISA_DEBUG=nohead (a wave never waits for the loads at the head of
its tile: a timing experiment, its results are garbage by design; the best such leg bounds a cross-tile prefetch from above).  Every
alternation times all legs, `warm` untimed launches and `timed` launches with a HIP event between them on the launch stream.  Prints every
leg, then per leg the gain over the first one (median and min over the leg's launches) per alternation, how many alternations agree in
sign, and the median.  Handle options only: works with the product build.
usage: gpu_claim_waves_ab.py [workload] [B] [paired|plain] [alternations] [warm] [timed] [waves, e.g. 4,3,2] [nohead|-]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import workloads, capi

dev = torch.device("cuda:0")
name = sys.argv[1] if len(sys.argv) > 1 else "parquet_sigma4"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
kind = sys.argv[3] if len(sys.argv) > 3 else "paired"
n_alt = int(sys.argv[4]) if len(sys.argv) > 4 else 5
warm = int(sys.argv[5]) if len(sys.argv) > 5 else 60
timed = int(sys.argv[6]) if len(sys.argv) > 6 else 20
waves = (sys.argv[7] if len(sys.argv) > 7 else "4,3,2").split(",")
nohead = len(sys.argv) > 8 and sys.argv[8] == "nohead"
t = workloads.get(name); L, R = t.n_leaf, t.n_root
fs = {"wait": fd.compile_table(t, specialize="isa")}
if nohead: fs["nohead"] = fd.compile_table(t, specialize="isa", options={"FDG_ISA_DEBUG": "nohead"})
T = (B + 63) // 64
st = torch.cuda.current_stream().cuda_stream

if kind == "paired":
    pb = fs["wait"].tile_major_pair(B, dev, calibrate=True)
    leaf, root = pb.leaf, pb.root
    print("paired: " + ", ".join(f"{k} = {pb.info[k]}" for k in ("n_chunk", "chunk_tiles", "n_matched", "gbs_fast", "gbs_slow")), flush=True)
else:
    leaf = torch.empty((T, L, 64), dtype=torch.float64, device=dev)
    root = torch.empty((T, R, 64), dtype=torch.float64, device=dev)
capi.fill_uniform_device_tiled(leaf.data_ptr(), B, L, 1, 64, 64 * L, 1234, 0, st)
for f in fs.values(): f.handle.set_option("FDG_ISA_TILE_CLAIM", "1")


def frac(ms): return 8 * (L + R) * B / ms / 1e6 / 8000


def med(x): return sorted(x)[len(x) // 2]


def label(l): return ("the rule's" if l[1] == "-" else l[1]) + " waves per CU" + (", nohead (garbage results)" if l[0] == "nohead" else "")


def leg(which, n_waves):
    f = fs[which]
    f.handle.set_option("FDG_ISA_MEM_WAVES", None if n_waves == "-" else n_waves)
    for _ in range(warm): f.eval_tiled(root, leaf, B)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(timed + 1)]
    ev[0].record()
    for k in range(timed):
        f.eval_tiled(root, leaf, B); ev[k + 1].record()
    torch.cuda.synchronize()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(timed)]
    ki = f.kernel_info()
    return ms, ki["last_kernel"] + ("_cl" if ki["tile_walk"] == "claimed" else ""), ki["last_grid"]


if not nohead and len(waves) > 1:      # the same bits from every wave count (a sample of the tiles and the last ones)
    pick = torch.cat([torch.randint(0, T, (4096,), device=dev), torch.arange(T - 8, T, device=dev)])
    got = []
    for n_waves in waves:
        fs["wait"].handle.set_option("FDG_ISA_MEM_WAVES", None if n_waves == "-" else n_waves)
        root[pick] = float("nan"); fs["wait"].eval_tiled(root, leaf, B); torch.cuda.synchronize()
        got.append(root[pick].clone().view(torch.int64))
    print("roots of the legs on %d tiles: %s" % (len(pick), "bit-equal" if all(torch.equal(g, got[0]) for g in got) else "DIFFERENT"), flush=True)

legs = [(w, n) for n in waves for w in fs]
base = legs[0]
gains = {l: [] for l in legs[1:]}
for a in range(n_alt):
    res = {}
    for l in legs:
        ms, k, n = leg(*l)
        res[l] = ms
        print(f"alternation {a} {label(l)} {k} x {n}: median {med(ms):.3f} ms ({frac(med(ms)):.3f}) min {min(ms):.3f} ms ({frac(min(ms)):.3f}) max {max(ms):.3f} ms", flush=True)
    for l in gains:
        gains[l].append((med(res[base]) / med(res[l]) - 1, min(res[base]) / min(res[l]) - 1))
print(f"{kind} {name} B = {B}: gain over {label(base)} per alternation (median | min of the leg's launches)")
for l, g_ in gains.items():
    print(f"   {label(l)}: " + " ".join(f"{100 * g:+.2f}|{100 * m:+.2f}%" for g, m in g_))
    print(f"      alternations faster: {sum(g > 0 for g, _ in g_)}/{n_alt} (median), {sum(m > 0 for _, m in g_)}/{n_alt} (min); median gain {100 * med([g for g, _ in g_]):+.2f} %")
if nohead:
    best = max((l for l in gains if l[0] == "nohead"), key=lambda l: med([g for g, _ in gains[l]]))
    print(f"upper bound of a cross-tile prefetch: {label(best)}, {100 * med([g for g, _ in gains[best]]):+.2f} % (median of {n_alt} alternations)")
if kind == "paired":
    pb.free()
