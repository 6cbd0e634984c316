"""GPU dev tool: does the headline evaluation lose rate because the launch is LONG?  One launch over the whole tile-major batch runs
a few per cent below the mean of its own 2 GB pieces (gpu_chunk_probe.py), but those pieces were timed five times in a row each, so
their pages were warm.  Here the batch is walked once per pass in every form, so nothing is warm that the whole launch does not have:
  (a) the whole batch in one launch;
  (b) the same batch as K back-to-back launches over consecutive ranges of tiles, K = 4, 8, 16, 32: timed as one pass, and again
      with an event after every launch (the time of each range INSIDE the pass);
  (c) the ranges of (b) timed one at a time, each repeated (warm, as gpu_chunk_probe.py times its segments).
The launch gap is measured as the time of K back-to-back launches over one tile.  If (b) minus K gaps sits at (c)'s level and clearly
under (a), short launches are faster because they are short (the persistent waves drift apart in a long one); if (b) is at (a)'s
level, the pieces of (c) only looked faster because they were repeated.
usage: gpu_split_pass_probe.py [workload] [B] [batches: paired,plain] [Ks: 4,8,16,32] [passes]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import workloads, capi

dev = torch.device("cuda:0")
name = sys.argv[1] if len(sys.argv) > 1 else "parquet_sigma4"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
batches = (sys.argv[3] if len(sys.argv) > 3 else "paired,plain").split(",")
Ks = [int(k) for k in (sys.argv[4] if len(sys.argv) > 4 else "4,8,16,32").split(",")]
passes = int(sys.argv[5]) if len(sys.argv) > 5 else 8
t = workloads.get(name); L, R = t.n_leaf, t.n_root
f = fd.compile_table(t, specialize="isa")
h = f.handle
T = (B + 63) // 64
st = torch.cuda.current_stream().cuda_stream


def frac(ms, n): return 8 * (L + R) * n / ms / 1e6 / 8000


def med(x): return sorted(x)[len(x) // 2]


def run(lp, rp, lo, hi):
    """tiles [lo, hi) of the batch (the last range ends at sample B)"""
    h.eval_device_tiled(lp + lo * 512 * L, 1, 64, 64 * L, rp + lo * 512 * R, 1, 64, 64 * R, min(B, 64 * hi) - 64 * lo, st)


def time_pass(fn, n, warm):
    """n timed calls of fn after `warm` untimed ones: list of ms"""
    for _ in range(warm): fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for k in range(n):
        fn(); ev[k + 1].record()
    torch.cuda.synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(n)]


def probe(kind, lp, rp, unit):
    print(f"== {kind} batch: {name}, B = {B} ({T} tiles), leaves @ {lp:#x}, roots @ {rp:#x}, ranges cut at multiples of {unit} tiles", flush=True)
    a = time_pass(lambda: run(lp, rp, 0, T), passes, 5)
    print(f"(a) one launch: min {min(a):.3f} ms ({frac(min(a), B):.3f}), median {med(a):.3f} ms ({frac(med(a), B):.3f})", flush=True)
    for K in Ks:
        cut = [min(T, round(i * T / K / unit) * unit) for i in range(K)] + [T]
        rng = [(cut[i], cut[i + 1]) for i in range(K) if cut[i + 1] > cut[i]]
        gap = min(time_pass(lambda: [run(lp, rp, 0, 1) for _ in rng], passes, 2)) / len(rng)

        def whole_pass():
            for lo, hi in rng: run(lp, rp, lo, hi)
        b = time_pass(whole_pass, passes, 2)
        # the same pass with an event after every launch: each range's time inside the pass
        inside = [[] for _ in rng]
        for p in range(passes):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(rng) + 1)]
            ev[0].record()
            for i, (lo, hi) in enumerate(rng):
                run(lp, rp, lo, hi); ev[i + 1].record()
            torch.cuda.synchronize()
            for i in range(len(rng)): inside[i].append(ev[i].elapsed_time(ev[i + 1]))
        b_in = [min(x) for x in inside]
        # (c) one at a time, repeated
        c = [min(time_pass(lambda: run(lp, rp, lo, hi), 5, 1)) for lo, hi in rng]
        net = min(b) - gap * len(rng)
        print(f"K = {len(rng):2d}: launch gap {1e3 * gap:.1f} us | (b) pass min {min(b):.3f} median {med(b):.3f} ms; minus {len(rng)} gaps {net:.3f} ms "
              f"({frac(net, B):.3f}) | (b) sum of the ranges' times inside the pass {sum(b_in):.3f} ms ({frac(sum(b_in), B):.3f}) "
              f"| (c) sum of the ranges alone, repeated {sum(c):.3f} ms ({frac(sum(c), B):.3f}) | (a) {min(a):.3f} ms ({frac(min(a), B):.3f})", flush=True)
        n_of = [min(B, 64 * hi) - 64 * lo for lo, hi in rng]
        print("   inside the pass: " + " ".join(f"{frac(x, n):.3f}" for x, n in zip(b_in, n_of)))
        print("   alone, repeated: " + " ".join(f"{frac(x, n):.3f}" for x, n in zip(c, n_of)), flush=True)
    a = time_pass(lambda: run(lp, rp, 0, T), passes, 2)
    print(f"(a) again: min {min(a):.3f} ms ({frac(min(a), B):.3f}), median {med(a):.3f} ms ({frac(med(a), B):.3f})", flush=True)


for kind in batches:
    if kind == "paired":
        pb = f.tile_major_pair(B, dev, calibrate=True)
        lp, rp, unit = pb.leaf.data_ptr(), pb.root.data_ptr(), int(pb.info["chunk_tiles"])
        print("paired: " + ", ".join(f"{k} = {pb.info[k]}" for k in ("n_chunk", "chunk_tiles", "n_matched", "gbs_fast", "gbs_slow")), flush=True)
    else:
        leaf = torch.empty((T, L, 64), dtype=torch.float64, device=dev)
        root = torch.empty((T, R, 64), dtype=torch.float64, device=dev)
        lp, rp, unit = leaf.data_ptr(), root.data_ptr(), 1
    capi.fill_uniform_device_tiled(lp, B, L, 1, 64, 64 * L, 1234, 0, st)
    probe(kind, lp, rp, unit)
    if kind == "paired":
        pb.free()
    else:
        del leaf, root
    torch.cuda.empty_cache()
