"""GPU dev tool: rate of the fused typed accumulation (fdg_accumulate_device_typed) next to what there was before it --
fdg_eval_device_typed into a [B, R] root matrix of the element type followed by torch's weighted column sum --, in one process, for
ComplexF64 (leaf-major and row-major) and Float32 leaves.  Warm-up, then many launches between two device events.
python tools/gpu_typed_accumulate_rate.py [--workload parquet_sigma4] [--samples 10000000] [--out profiles/typed_accumulate_rates.txt]"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import workloads

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="parquet_sigma4")
ap.add_argument("--samples", type=int, default=10_000_000)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "typed_accumulate_rates.txt"))
a = ap.parse_args()
dev = torch.device("cuda:0")
t = workloads.get(a.workload)
f = fd.compile_table(t, specialize="isa")
B, L, R = a.samples, t.n_leaf, t.n_root
lines = [f"# {a.workload}: L={L} R={R}, {B} samples, {a.launches} launches after 5 warm-up calls, device events; {torch.cuda.get_device_name(0)}"]


def timed(call):
    for _ in range(5): call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.launches): call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.launches


w = torch.rand(B, dtype=torch.float64, device=dev) - 0.25
for dtype, td, layout in (("ComplexF64", torch.complex128, "leaf-major"), ("ComplexF64", torch.complex128, "row-major"), ("Float32", torch.float32, "leaf-major")):
    x = torch.rand((L, B), dtype=torch.float64, device=dev) - 0.3
    leaf = (torch.complex(x, torch.rand_like(x) - 0.6) if td.is_complex else x).to(td).t()
    del x
    if layout == "row-major":
        leaf = leaf.contiguous()
    adt = torch.complex128 if td.is_complex else torch.float64
    acc = torch.zeros(R, dtype=adt, device=dev)
    ms_fused = timed(lambda: f.accumulate(leaf, w, acc))
    k_fused = f.last_typed_kernel
    # the sum against the typed twin on the first samples
    n = 2048
    got = f.accumulate(leaf[:n], w[:n]).cpu().numpy()
    h = np.ascontiguousarray(leaf[:n].cpu().numpy())
    terms = oracle.eval_static_typed(t, h, dtype).astype(np.complex128 if td.is_complex else np.float64) * w[:n].cpu().numpy()[:, None]
    ok = all(np.all(np.abs(g - c.sum(0)) <= 1e-12 * np.maximum(1.0, np.abs(c).sum(0)))
             for g, c in ((got.real, terms.real), (got.imag, terms.imag)))
    # before: the roots of the element type in memory, then torch's weighted column sum in that type
    root = torch.empty((B, R), dtype=td, device=dev) if layout == "row-major" else torch.empty((R, B), dtype=td, device=dev).t()
    wt = w.to(td)
    def two_pass():
        f(root, leaf)
        return wt @ root
    ms_two = timed(two_pass)
    k_eval = f.last_typed_kernel
    ms_eval = timed(lambda: f(root, leaf))
    root_bytes = B * R * root.element_size()
    lines.append(f"{dtype:10s} {layout:10s} fused {ms_fused:8.3f} ms {B / ms_fused * 1e3:.3e} samples/s [{k_fused}] {'sum within 1e-12' if ok else 'SUM OFF'} | "
                 f"eval + torch sum {ms_two:8.3f} ms {B / ms_two * 1e3:.3e} samples/s (eval alone {ms_eval:.3f} ms) [{k_eval}] | "
                 f"root matrix no longer allocated: {root_bytes} bytes")
    print(lines[-1], flush=True)
    del leaf, root, wt
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
