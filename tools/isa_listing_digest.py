"""(no GPU) The assembly listings of a fixed corpus, as digests: every entry is specialised into a fresh cache directory with
FDG_SPEC_KEEP_SOURCE and the name and SHA-256 of each `.s` file left there is printed.  A listing's file name is the hash of its text, so
two commits that print the same lines print the same kernels.  The corpus is the one profiles/isa_variant_meta_equal.txt describes:

  tuned:NAME / untuned:NAME        every name in workloads.PREBUILT, with and without the remembered configurations (FDG_IGNORE_TUNED)
  tuned:mc:NAME / untuned:mc:NAME  every name in workloads.PREBUILT_MC, the one-kernel Monte-Carlo step behind the evaluator's code object
  FDG_ISA_COOP=1:G, FDG_ISA_POOL=1:G, FDG_ISA_W2=1:G   the graphs of tests/test_random_graphs.py (fuzz_table 1000..1055,
                                   random_table 0..39, power_table 0..5) with that variant forced on

    python tools/isa_listing_digest.py [--jobs N] > listings.txt       # the last line counts code objects and kernels
"""
import argparse
import glob
import hashlib
import multiprocessing
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def corpus():
    from feynmandiagram_jl_amd import workloads
    for tuned in ("tuned", "untuned"):
        for name in workloads.PREBUILT:
            yield f"{tuned}:{name}"
        for name in workloads.PREBUILT_MC:
            yield f"{tuned}:mc:{name}"
    graphs = [f"fuzz_{s}" for s in range(1000, 1056)] + [f"random_{s}" for s in range(40)] + [f"power_{s}" for s in range(6)]
    for variant in ("FDG_ISA_COOP", "FDG_ISA_POOL", "FDG_ISA_W2"):
        for g in graphs:
            yield f"{variant}=1:{g}"


def digest(entry):
    """(entry, [(file name, sha256, kernels)]) of one corpus entry"""
    import feynmandiagram_jl_amd as fd
    from feynmandiagram_jl_amd import capi, workloads
    head, _, name = entry.rpartition(":")
    options = {}
    if head.startswith("untuned"):
        options["FDG_IGNORE_TUNED"] = "1"
    if head.startswith("FDG_"):
        options[head.split("=")[0]] = "1"
        import test_random_graphs as T
        kind, seed = name.split("_")
        table = {"fuzz": lambda s: T.fuzz_table(s)[0], "random": T.random_table, "power": T.power_table}[kind](int(seed))
    else:
        table = workloads.get(name)
    with tempfile.TemporaryDirectory() as d:
        f = fd.compile_table(table, specialize="isa", cache_dir=d, flags=capi.FDG_SPEC_KEEP_SOURCE, options=options)
        if head.endswith(":mc"):
            z = workloads.leafstates(name)
            tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], 3, int(z["n_tau"]))
            before = set(glob.glob(d + "/*.s"))
            f.handle.specialize_fused(tab, cache_dir=d, flags=capi.FDG_SPEC_KEEP_SOURCE)
            files = sorted(set(glob.glob(d + "/*.s")) - before)         # (the evaluator's own listing is the entry without `mc:`)
        else:
            files = sorted(glob.glob(d + "/*.s"))
        out = []
        for path in files:
            text = open(path, "rb").read()
            out.append((os.path.basename(path), hashlib.sha256(text).hexdigest(), text.count(b"\t.protected\t")))
    return entry, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--jobs", type=int, default=min(16, len(os.sched_getaffinity(0))))
    args = ap.parse_args()
    n_file = n_kernel = 0
    with multiprocessing.get_context("spawn").Pool(args.jobs) as pool:
        for entry, files in pool.imap(digest, list(corpus())):
            print(entry)
            for name, sha, kernels in files:
                print(f"  {name}  sha256 {sha}  {kernels} kernels", flush=True)
                n_file += 1
                n_kernel += kernels
    print(f"{n_file} code objects, {n_kernel} kernels")


if __name__ == "__main__":
    main()
