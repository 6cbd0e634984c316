"""GPU dev tool: the claimed tile walk (option FDG_ISA_TILE_CLAIM) against the static one, in ONE process on ONE allocation -- the only
comparison the allocation lottery allows.  The headline batch (tile-major, fdg_batch_alloc_pair or torch.empty) is evaluated
with the option alternating 0 / 1; every leg is `warm` untimed launches and `timed` launches with a HIP event between them on the launch
stream.  Prints every leg, then per alternation the gain of the claimed walk (median and min over the leg's launches) and how many
alternations agree in sign.  With `leg=0` / `leg=1` only that walk runs (one leg: for a kernel trace under a profiler).  `runs`: tiles per
claim (FDG_ISA_CLAIM_RUN, a handle each), several separated by commas: every alternation then times the static walk and each of them.
usage: gpu_tile_claim_ab.py [workload] [B] [paired|plain] [alternations] [warm] [timed] [leg|-] [runs]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import workloads, capi

dev = torch.device("cuda:0")
name = sys.argv[1] if len(sys.argv) > 1 else "parquet_sigma4"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
kind = sys.argv[3] if len(sys.argv) > 3 else "paired"
n_alt = int(sys.argv[4]) if len(sys.argv) > 4 else 10
warm = int(sys.argv[5]) if len(sys.argv) > 5 else 60
timed = int(sys.argv[6]) if len(sys.argv) > 6 else 20
only = sys.argv[7] if len(sys.argv) > 7 and sys.argv[7] != "-" else ""
runs = (sys.argv[8] if len(sys.argv) > 8 else "4").split(",")
t = workloads.get(name); L, R = t.n_leaf, t.n_root
fs = {r: fd.compile_table(t, specialize="isa", options={"FDG_ISA_CLAIM_RUN": r}) for r in runs}
f = fs[runs[0]]
T = (B + 63) // 64
st = torch.cuda.current_stream().cuda_stream

if kind == "paired":
    pb = f.tile_major_pair(B, dev, calibrate=True)
    leaf, root = pb.leaf, pb.root
    print("paired: " + ", ".join(f"{k} = {pb.info[k]}" for k in ("n_chunk", "chunk_tiles", "n_matched", "gbs_fast", "gbs_slow")), flush=True)
else:
    leaf = torch.empty((T, L, 64), dtype=torch.float64, device=dev)
    root = torch.empty((T, R, 64), dtype=torch.float64, device=dev)
capi.fill_uniform_device_tiled(leaf.data_ptr(), B, L, 1, 64, 64 * L, 1234, 0, st)


def frac(ms): return 8 * (L + R) * B / ms / 1e6 / 8000


def med(x): return sorted(x)[len(x) // 2]


def leg(claim, f=f):
    f.handle.set_option("FDG_ISA_TILE_CLAIM", claim)
    for _ in range(warm): f.eval_tiled(root, leaf, B)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(timed + 1)]
    ev[0].record()
    for k in range(timed):
        f.eval_tiled(root, leaf, B); ev[k + 1].record()
    torch.cuda.synchronize()
    ms = [ev[k].elapsed_time(ev[k + 1]) for k in range(timed)]
    ki = f.kernel_info()
    return ms, ki["last_kernel"] + ("_cl" if ki["tile_walk"] == "claimed" else ""), ki["last_grid"]


if only:
    ms, k, n = leg(only)
    print(f"{kind} {name} B = {B}: FDG_ISA_TILE_CLAIM={only} {k} x {n}: median {med(ms):.3f} ms ({frac(med(ms)):.3f}) min {min(ms):.3f} ms ({frac(min(ms)):.3f})")
    sys.exit(0)

# the same bits from both walks (a sample of the tiles and the last ones)
f.handle.set_option("FDG_ISA_TILE_CLAIM", "0"); f.eval_tiled(root, leaf, B); torch.cuda.synchronize()
pick = torch.cat([torch.randint(0, T, (4096,), device=dev), torch.arange(T - 8, T, device=dev)])
want = root[pick].clone()
f.handle.set_option("FDG_ISA_TILE_CLAIM", "1"); root[pick] = float("nan"); f.eval_tiled(root, leaf, B); torch.cuda.synchronize()
print("roots of the two walks on %d tiles: %s" % (len(pick), "bit-equal" if torch.equal(root[pick].view(torch.int64), want.view(torch.int64)) else "DIFFERENT"), flush=True)

gains = {r: [] for r in runs}
for a in range(n_alt):
    res = {}
    for r in ["static"] + runs:
        ms, k, n = leg("0" if r == "static" else "1", fs[runs[0] if r == "static" else r])
        res[r] = ms
        print(f"alternation {a} {'static walk' if r == 'static' else 'claimed, ' + r + ' tiles per claim'} {k} x {n}: median {med(ms):.3f} ms ({frac(med(ms)):.3f}) min {min(ms):.3f} ms ({frac(min(ms)):.3f}) max {max(ms):.3f} ms", flush=True)
    for r in runs:
        gains[r].append((med(res["static"]) / med(res[r]) - 1, min(res["static"]) / min(res[r]) - 1))
for r in runs:
    g_ = gains[r]
    print(f"{kind} {name} B = {B}, {r} tiles per claim: gain of the claimed walk per alternation (median | min): " + " ".join(f"{100 * g:+.2f}|{100 * m:+.2f}%" for g, m in g_))
    print(f"   alternations with the claimed walk faster: {sum(g > 0 for g, _ in g_)}/{n_alt} (median), {sum(m > 0 for _, m in g_)}/{n_alt} (min); "
          f"median gain {100 * med([g for g, _ in g_]):+.2f} %")
if kind == "paired":
    pb.free()
