"""FDG_ISA_NO_RM: the way off the chunked row-major variant (fdg_isa_eval_rm / _rm_acc), the counterpart of FDG_ISA_NO_RL and
FDG_ISA_NO_POOL.  Set before fdg_graph_specialize the code object is assembled without the two kernels (csrc/fdg_runtime.hip:
build_rm_program); set on a handle that has them, the next call leaves them alone (IsaRun::wants_rm) and the rows go through the
transposition in front of the plain kernels.

The graph is the smallest prebuilt workload whose default code object holds fdg_isa_eval_rm: parquet_sigma3, 27 leaves, 3 roots.  It has
the linear variant for contiguous rows too, so the device test pads its rows (pitch L + 3): padded rows are the chunked variant's."""
import glob
import os
import re

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, workloads

NAME = "parquet_sigma3"
RM = ("fdg_isa_eval_rm", "fdg_isa_eval_rm_acc")


def kernels(text):
    """name -> (text of the kernel, its entry in the code object's metadata), cut as tests/test_tile_claim.py cuts a listing"""
    body, meta = {}, {}
    for part in text.split("\t.text\n"):
        m = re.match(r"\t\.protected\t(\S+)\n", part)
        if m:
            body[m.group(1)] = part.split("\t.amdgpu_metadata")[0]
        if "\t.amdgpu_metadata" in part:
            for e in part.split("\t.amdgpu_metadata")[1].split("  - .agpr_count")[1:]:
                entry = e.partition("amdhsa.target:")[0]
                meta[re.search(r"\.name: +(\S+)\n", entry).group(1)] = entry
    assert body and set(body) == set(meta)
    return {k: (body[k], meta[k]) for k in body}


def specialise(tmp, **options):
    d = os.path.join(str(tmp), "_".join(options) or "default")
    os.makedirs(d, mode=0o700)
    f = fd.compile_table(workloads.get(NAME), specialize="isa", cache_dir=d, flags=capi.FDG_SPEC_KEEP_SOURCE, options=options)
    (src,) = glob.glob(d + "/fdg_isa_*.s")
    return f, kernels(open(src).read())


def test_the_option_takes_the_two_kernels_out_and_leaves_every_other_as_it_was(libfdg, tmp_path):
    # (what the choice of NAME rests on: every smaller prebuilt graph has fewer than 16 leaves, so no such kernel)
    smaller = [n for n in workloads.PREBUILT if workloads.get(n).n_node < workloads.get(NAME).n_node]
    assert smaller and all(workloads.get(n).n_leaf < 16 for n in smaller)
    f0, k0 = specialise(tmp_path)
    f1, k1 = specialise(tmp_path, FDG_ISA_NO_RM="1")
    assert set(RM) <= set(k0) and f0.kernel_info()["has_rm"] == 1 and f0.kernel_info()["rm_bufs"] > 0
    assert not any(n.endswith(("_rm", "_rm_acc")) for n in k1)
    ki = f1.kernel_info()
    assert ki["has_rm"] == 0 and ki["rm_bufs"] == 0 and ki["n_valu"][2] == 0, ki
    assert set(k1) == set(k0) - set(RM)
    for name in k1:
        assert k1[name] == k0[name], name


@pytest.mark.gpu
def test_set_on_a_handle_that_has_the_kernels_the_rows_take_another_road_to_the_same_bits(libfdg, cuda):
    """65 padded rows, one full tile and a ragged one.  By default the full tile runs fdg_isa_eval_rm / _rm_acc; with the option set after
    specialisation neither call launches them (kernel_info: the name of the kernel and the workgroups of the launch), the roots are the
    oracle's bit for bit and the weighted sums are the exact sums of the oracle's terms to within the roundings of any order of summation:
    B products and B additions, each within 2^-53 of a partial sum that the sum of |terms| bounds -- |d| <= (B + 2) 2^-53 sum |w root|."""
    import fractions
    import torch
    t = workloads.get(NAME)
    L, R, B = t.n_leaf, t.n_root, 65
    f = fd.compile_table(t, specialize="isa")
    assert f.kernel_info()["has_rm"] == 1
    h_leaf = oracle.philox_uniform(B, L, 65) * 2 - 0.5
    want = oracle.eval_static(t, h_leaf)
    h_w = np.random.default_rng(65).uniform(0.5, 1.5, B)
    exact = [sum(fractions.Fraction(float(h_w[b])) * fractions.Fraction(float(want[b, k])) for b in range(B)) for k in range(R)]
    bound = (B + 2) * 2.0 ** -53 * np.abs(want * h_w[:, None]).sum(0)
    pad = torch.full((B, L + 3), float("nan"), dtype=torch.float64, device=cuda)
    pad[:, :L] = torch.from_numpy(h_leaf).to(cuda)
    leaf, w = pad[:, :L], torch.from_numpy(h_w).to(cuda)

    def run():
        root = torch.full((B, R), 9.0, dtype=torch.float64, device=cuda)
        f(root, leaf)
        torch.cuda.synchronize()
        ki_eval = f.kernel_info()
        acc = f.accumulate(leaf, w)
        torch.cuda.synchronize()
        ki_acc = f.kernel_info()
        got, sums = root.cpu().numpy(), acc.cpu().numpy()
        d = np.array([abs(float(fractions.Fraction(float(sums[k])) - exact[k])) for k in range(R)])
        print("last kernels", ki_eval["last_kernel"], ki_acc["last_kernel"], "grids", ki_eval["last_grid"], ki_acc["last_grid"], "|d| / bound", d / bound)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), ki_eval["last_kernel"]
        assert np.all(d <= bound), (ki_acc["last_kernel"], d / bound)
        return ki_eval, ki_acc

    ki_eval, ki_acc = run()
    assert (ki_eval["last_kernel"], ki_acc["last_kernel"]) == RM, "padded rows of a full tile are the chunked variant's by default"
    f.handle.set_option("FDG_ISA_NO_RM", "1")
    ki_eval, ki_acc = run()
    for ki in (ki_eval, ki_acc):
        assert ki["last_kernel"].startswith("fdg_isa_eval") and ki["last_kernel"] not in RM and ki["last_grid"] > 0, ki
