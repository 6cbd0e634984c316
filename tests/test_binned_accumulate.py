"""Binned accumulation on the device (include/fdg.h: fdg_accumulate_device_binned, fdg_mc_accumulate_device_binned):
acc[j, k] += w[b] root_k(b) for the samples whose bin j = bins[b] - bin_base lies in [0, n_bin).  The expected value is the oracle's roots
binned on the host; the bar is the accumulate tests' own, |d| <= 1e-12 max(1, sum over the bin of |w root|) per (bin, root)."""
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, workloads
from feynmandiagram_jl_amd.lowering import lower
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-12
SPECS = {"interp": False, "hip": True, "isa": "isa"}


def host_binned(roots, bins, n_bin, w=None, base=0):
    """(sum, sum of |terms|) per (bin, root) of the samples whose bin is in range"""
    j = bins.astype(np.int64) - base
    ok = (j >= 0) & (j < n_bin)
    terms = roots[ok] if w is None else roots[ok] * w[ok, None]
    want = np.zeros((n_bin, roots.shape[1]))
    scale = np.zeros_like(want)
    np.add.at(want, j[ok], terms)
    np.add.at(scale, j[ok], np.abs(terms))
    return want, scale


def assert_close(got, want, scale, what):
    bad = np.abs(got - want) > TOL * np.maximum(1.0, scale)
    assert not bad.any(), (what, np.argwhere(bad)[:4], np.abs(got - want).max())


def make_bins(rng, B, n_bin, base=0, skew=False):
    """uniform bins in [base, base + n_bin) (or 90 % in the first bin), with a few out of range on both sides"""
    b = rng.integers(0, n_bin, size=B)
    if skew:
        b = np.where(rng.random(B) < 0.9, 0, b)
    out = rng.random(B)
    b = np.where(out < 0.01, -1, np.where(out < 0.02, n_bin, b))
    return (b + base).astype(np.int32)


def to_tiles(x):
    B, C = x.shape
    T = (B + 63) // 64
    full = np.full((T * 64, C), np.nan)
    full[:B] = x
    return np.ascontiguousarray(full.reshape(T, 64, C).transpose(0, 2, 1))


def leaves(cuda, h_leaf, layout):
    import torch
    if layout == "row":
        return torch.from_numpy(h_leaf).to(cuda)
    if layout == "leaf_major":
        return torch.from_numpy(np.ascontiguousarray(h_leaf.T)).to(cuda).t()
    return torch.from_numpy(to_tiles(h_leaf)).to(cuda)


@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("name", ["sigma2", "gv_sigma4", "parquet_sigma4"])
def test_binned_parity(libfdg, cuda, name, spec):
    import torch
    t = workloads.get(name)
    L, R, B = t.n_leaf, t.n_root, 200_003
    f = fd.compile_table(t, specialize=SPECS[spec])
    h_leaf = oracle.philox_uniform(B, L, 31)
    roots = oracle.eval_static(t, h_leaf)
    rng = np.random.default_rng(7)
    h_w = rng.uniform(-1.0, 2.0, size=B)
    w = torch.from_numpy(h_w).to(cuda)
    layouts = ["row", "leaf_major"] + (["tiled"] if spec == "isa" else [])
    cases = [(1, None, 0), (7, h_w, 1), (64, h_w, 0), (4096, None, 1), (capi.FDG_BIN_MAX, h_w, 0)]
    for layout in layouts:
        leaf = leaves(cuda, h_leaf, layout)
        for n_bin, hw, base in cases:
            h_bins = make_bins(rng, B, n_bin, base)
            want, scale = host_binned(roots, h_bins, n_bin, hw, base)
            acc = f.accumulate_binned(leaf, torch.from_numpy(h_bins).to(cuda), n_bin, None if hw is None else w, bin_base=base, n_sample=B)
            torch.cuda.synchronize()
            assert acc.shape == (n_bin, R)
            assert_close(acc.cpu().numpy(), want, scale, (layout, n_bin, base, hw is None))


def test_adds_on_top_is_bitwise_repeatable_and_matches_accumulate(libfdg, cuda):
    import torch
    t = workloads.get("parquet_sigma4")
    L, R, B = t.n_leaf, t.n_root, 100_001
    f = fd.compile_table(t, specialize="isa")
    h_leaf = oracle.philox_uniform(B, L, 5)
    roots = oracle.eval_static(t, h_leaf)
    leaf = torch.from_numpy(to_tiles(h_leaf)).to(cuda)
    rng = np.random.default_rng(3)
    h_w = rng.uniform(0.5, 1.5, size=B)
    w = torch.from_numpy(h_w).to(cuda)
    n_bin = 64
    bins = torch.from_numpy(make_bins(rng, B, n_bin)).to(cuda)
    acc0 = torch.from_numpy(rng.uniform(-3.0, 3.0, size=(n_bin, R))).to(cuda)
    a1 = f.accumulate_binned(leaf, bins, n_bin, w, acc0.clone(), n_sample=B)
    a2 = f.accumulate_binned(leaf, bins, n_bin, w, acc0.clone(), n_sample=B)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2)                                    # no atomics: the same arguments give the same bits
    want, scale = host_binned(roots, bins.cpu().numpy(), n_bin, h_w)
    assert_close(a1.cpu().numpy(), acc0.cpu().numpy() + want, scale + np.abs(acc0.cpu().numpy()), "on top")
    f.accumulate_binned(leaf, bins, n_bin, w, a1, n_sample=B)     # a second call adds again
    assert_close(a1.cpu().numpy(), acc0.cpu().numpy() + 2 * want, 2 * scale + np.abs(acc0.cpu().numpy()), "twice")
    # one bin that holds every sample is the plain accumulation, and the bins of any binning add up to it
    plain = f.accumulate_tiled(leaf, w, None, B)
    one = f.accumulate_binned(leaf, torch.zeros(B, dtype=torch.int32, device=cuda), 1, w, n_sample=B)
    all_in = torch.from_numpy(rng.integers(0, 4096, size=B).astype(np.int32)).to(cuda)
    many = f.accumulate_binned(leaf, all_in, 4096, w, n_sample=B)
    torch.cuda.synchronize()
    ref = (roots * h_w[:, None]).sum(0)
    tot = (np.abs(roots) * h_w[:, None]).sum(0)
    assert_close(one.cpu().numpy()[0], plain.cpu().numpy(), tot, "one bin")
    assert_close(many.cpu().numpy().sum(0), ref, tot, "sum over bins")


@pytest.mark.parametrize("spec", list(SPECS))
def test_missing_root_column_is_left_alone(libfdg, cuda, spec):
    import torch
    a, b, c = fd.Graph([]), fd.Graph([]), fd.Graph([])
    s = a + b
    p = fd.Graph([s, c, a], subgraph_factors=[1.0, -0.5, 2.0], operator=fd.Prod())
    t, _, _ = lower([s, p], root=[s.id, 424242, p.id])
    assert int(t.root_slot[1]) == FDG_NO_ROOT
    f = fd.compile_table(t, specialize=SPECS[spec])
    B, n_bin = 5_000, 9
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 9) + 0.25
    roots = oracle.eval_static(t, h_leaf)
    h_bins = make_bins(np.random.default_rng(1), B, n_bin)
    acc = torch.full((n_bin, t.n_root), -7.0, dtype=torch.float64, device=cuda)
    f.accumulate_binned(torch.from_numpy(h_leaf).to(cuda), torch.from_numpy(h_bins).to(cuda), n_bin, None, acc)
    got = acc.cpu().numpy()
    assert np.array_equal(got[:, 1], np.full(n_bin, -7.0))
    live = [0, 2]
    want, scale = host_binned(roots[:, live], h_bins, n_bin)
    assert_close(got[:, live], want - 7.0, scale + 7.0, spec)


def test_many_roots_skewed_bins_small_chunks_and_poisoned_samples(libfdg, cuda):
    """parquet_ver4_4 (R = 180): n_bin = 1024 takes the root-slice loop; 90 % of the samples in bin 0; FDG_ROOT_SCRATCH_MB=1 cuts the
    batch into about thirty chunks; inf leaves on samples whose bin is out of range reach no bin."""
    import torch
    t = workloads.get("parquet_ver4_4")
    L, R, B, n_bin = t.n_leaf, t.n_root, 20_011, 1024
    f = fd.compile_table(t, specialize="isa", options={"FDG_ROOT_SCRATCH_MB": "1"})
    h_leaf = oracle.philox_uniform(B, L, 17)
    rng = np.random.default_rng(23)
    h_bins = make_bins(rng, B, n_bin, skew=True)
    poisoned = rng.choice(B, size=40, replace=False)
    h_bins[poisoned[:20]] = -1
    h_bins[poisoned[20:]] = n_bin
    h_leaf[poisoned] = np.inf
    roots = oracle.eval_static(t, h_leaf)
    h_w = rng.uniform(0.0, 1.0, size=B)
    acc = f.accumulate_binned(leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_bins).to(cuda), n_bin, torch.from_numpy(h_w).to(cuda),
                              n_sample=B)
    got = acc.cpu().numpy()
    assert np.isfinite(got).all()
    want, scale = host_binned(roots, h_bins, n_bin, h_w)
    assert_close(got, want, scale, "parquet_ver4_4")


@pytest.mark.parametrize("route", ["split", "fused", None])
def test_mc_binned_routes(libfdg, cuda, fdgopt, route):
    import torch
    z = dict(np.load(os.path.join(GOLD, "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    R = t.n_root
    B, dim, n_loop, n_tau = 50_001, 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam = 1.919, 3.0, 1.2
    rng = np.random.default_rng(13)
    dK = torch.from_numpy(rng.uniform(-2.0, 2.0, size=(n_loop * dim, B))).to(cuda)
    dT = torch.from_numpy(rng.uniform(0.0, beta, size=(n_tau, B))).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    if route:
        fdgopt.set("FDG_MC_ROUTE", route)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    root = torch.zeros((B, R), dtype=torch.float64, device=cuda)
    f.handle.mc_eval_device(dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, kF, beta, lam, root.data_ptr(), R, 1, B, st)
    n_bin = 33
    h_bins = make_bins(rng, B, n_bin, base=1)
    bins = torch.from_numpy(h_bins).to(cuda)
    w = torch.from_numpy(rng.uniform(0.0, 1.0, size=B)).to(cuda)
    acc = torch.zeros((n_bin, R), dtype=torch.float64, device=cuda)
    f.handle.mc_accumulate_device_binned(dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, kF, beta, lam, bins.data_ptr(), 1, n_bin, w.data_ptr(),
                                         acc.data_ptr(), B, st)
    torch.cuda.synchronize()
    want, scale = host_binned(root.cpu().numpy(), h_bins, n_bin, w.cpu().numpy(), base=1)
    assert_close(acc.cpu().numpy(), want, scale, route)


def test_two_shards_add_up_to_the_batch(libfdg, cuda):
    import torch
    t = workloads.get("gv_sigma4")
    B, n_bin = 70_000, 100
    f = fd.compile_table(t, specialize="isa")
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 2)
    rng = np.random.default_rng(4)
    h_bins = make_bins(rng, B, n_bin)
    h_w = rng.uniform(-1.0, 1.0, size=B)
    leaf, bins, w = torch.from_numpy(h_leaf).to(cuda), torch.from_numpy(h_bins).to(cuda), torch.from_numpy(h_w).to(cuda)
    whole = f.accumulate_binned(leaf, bins, n_bin, w)
    acc = torch.zeros((n_bin, t.n_root), dtype=torch.float64, device=cuda)
    h = B // 2
    f.accumulate_binned(leaf[:h], bins[:h], n_bin, w[:h], acc)
    f.accumulate_binned(leaf[h:], bins[h:], n_bin, w[h:], acc)
    torch.cuda.synchronize()
    want, scale = host_binned(oracle.eval_static(t, h_leaf), h_bins, n_bin, h_w)
    assert_close(whole.cpu().numpy(), want, scale, "whole")
    assert_close(acc.cpu().numpy(), whole.cpu().numpy(), scale, "shards")


def test_accumulate_binned_validates_its_arguments(libfdg, cuda):
    import torch
    t = workloads.get("sigma2")
    f = fd.compile_table(t, specialize="isa")
    B = 1000
    leaf = torch.rand((B, t.n_leaf), dtype=torch.float64, device=cuda)
    bins = torch.zeros(B, dtype=torch.int32, device=cuda)
    with pytest.raises(TypeError):
        f.accumulate_binned(leaf, bins.double(), 4)
    with pytest.raises(ValueError):
        f.accumulate_binned(leaf, bins[:B - 1], 4)
    with pytest.raises(ValueError):
        f.accumulate_binned(leaf, bins, 4, torch.ones(B - 1, dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        f.accumulate_binned(leaf, bins, 4, None, torch.zeros((t.n_root, 4), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        f.accumulate_binned(leaf, bins, 0)
    assert f.accumulate_binned(leaf, bins, 4).shape == (4, t.n_root)
