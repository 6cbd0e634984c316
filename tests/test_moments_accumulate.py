"""Second-moment accumulation on the device (include/fdg.h: fdg_accumulate_device_moments, fdg_mc_accumulate_device_moments): with
t = w[b] root_k(b), acc[j, k] += t and acc2[j, k] += t * t for the samples whose bin j = bins[b] - bin_base lies in [0, n_bin).  acc must
carry the bits of fdg_accumulate_device_binned for the same arguments; acc2 is checked against the oracle's roots squared and binned on the
host, |d| <= 1e-12 max(1, sum over the bin of t * t) per (bin, root).  The helpers are copies of tests/test_binned_accumulate.py's."""
import math
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


def host_moments(roots, bins, n_bin, w=None, base=0):
    """(sum of t, sum of |t|, sum of t * t) per (bin, root) of the samples whose bin is in range; bins None: all in bin 0"""
    j = np.zeros(roots.shape[0], dtype=np.int64) if bins is None else bins.astype(np.int64) - base
    ok = (j >= 0) & (j < n_bin)
    terms = roots[ok] if w is None else roots[ok] * w[ok, None]
    s1 = np.zeros((n_bin, roots.shape[1]))
    a1 = np.zeros_like(s1)
    s2 = np.zeros_like(s1)
    np.add.at(s1, j[ok], terms)
    np.add.at(a1, j[ok], np.abs(terms))
    np.add.at(s2, j[ok], terms * terms)
    return s1, a1, s2


def assert_close(got, want, scale, what):
    bad = np.abs(got - want) > TOL * np.maximum(1.0, scale)
    assert not bad.any(), (what, np.argwhere(bad)[:4], np.abs(got - want).max())


def assert_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, np.argwhere(a.view(np.uint64) != b.view(np.uint64))[:4])


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
def test_moments_parity_and_bitwise_tie(libfdg, cuda, name, spec):
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
    # (n_bin, weight, base); bins None: the NULL-bins call, tied to an all-zero bin vector
    cases = [(1, None, None), (7, h_w, 1), (64, h_w, 0), (4096, None, 0), (capi.FDG_BIN_MAX, h_w, 0)]
    for layout in layouts:
        leaf = leaves(cuda, h_leaf, layout)
        for n_bin, hw, base in cases:
            h_bins = None if base is None else make_bins(rng, B, n_bin, base)
            d_bins = None if h_bins is None else torch.from_numpy(h_bins).to(cuda)
            ww = None if hw is None else w
            acc, acc2 = f.accumulate_moments(leaf, d_bins, n_bin, ww, bin_base=base or 0, n_sample=B)
            tie_bins = torch.zeros(B, dtype=torch.int32, device=cuda) if d_bins is None else d_bins
            ref = f.accumulate_binned(leaf, tie_bins, n_bin, ww, bin_base=base or 0, n_sample=B)
            torch.cuda.synchronize()
            what = (layout, n_bin, base, hw is None)
            assert acc.shape == acc2.shape == (n_bin, R)
            assert_bits(acc.cpu().numpy(), ref.cpu().numpy(), what)
            s1, a1, s2 = host_moments(roots, h_bins, n_bin, hw, base or 0)
            assert_close(acc.cpu().numpy(), s1, a1, what)
            assert_close(acc2.cpu().numpy(), s2, s2, what)


def test_repeatable_and_adds_on_top(libfdg, cuda):
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
    h_bins = make_bins(rng, B, n_bin)
    bins = torch.from_numpy(h_bins).to(cuda)
    p1 = torch.from_numpy(rng.uniform(-3.0, 3.0, size=(n_bin, R))).to(cuda)
    p2 = torch.from_numpy(rng.uniform(0.0, 3.0, size=(n_bin, R))).to(cuda)
    a1, q1 = f.accumulate_moments(leaf, bins, n_bin, w, p1.clone(), p2.clone(), n_sample=B)
    a2, q2 = f.accumulate_moments(leaf, bins, n_bin, w, p1.clone(), p2.clone(), n_sample=B)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and torch.equal(q1, q2)           # no atomics: the same arguments give the same bits
    assert_bits(a1.cpu().numpy(), f.accumulate_binned(leaf, bins, n_bin, w, p1.clone(), n_sample=B).cpu().numpy(), "on top")
    s1, a_1, s2 = host_moments(roots, h_bins, n_bin, h_w)
    h1, h2 = p1.cpu().numpy(), p2.cpu().numpy()
    assert_close(a1.cpu().numpy(), h1 + s1, a_1 + np.abs(h1), "acc on top")
    assert_close(q1.cpu().numpy(), h2 + s2, s2 + h2, "acc2 on top")
    f.accumulate_moments(leaf, bins, n_bin, w, a1, q1, n_sample=B)   # a second call adds again
    assert_close(a1.cpu().numpy(), h1 + 2 * s1, 2 * a_1 + np.abs(h1), "acc twice")
    assert_close(q1.cpu().numpy(), h2 + 2 * s2, 2 * s2 + h2, "acc2 twice")


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
    acc2 = torch.full((n_bin, t.n_root), 5.0, dtype=torch.float64, device=cuda)
    f.accumulate_moments(torch.from_numpy(h_leaf).to(cuda), torch.from_numpy(h_bins).to(cuda), n_bin, None, acc, acc2)
    got, got2 = acc.cpu().numpy(), acc2.cpu().numpy()
    assert np.array_equal(got[:, 1], np.full(n_bin, -7.0))
    assert np.array_equal(got2[:, 1], np.full(n_bin, 5.0))
    live = [0, 2]
    s1, a1, s2 = host_moments(roots[:, live], h_bins, n_bin)
    assert_close(got[:, live], s1 - 7.0, a1 + 7.0, spec)
    assert_close(got2[:, live], s2 + 5.0, s2 + 5.0, spec)


def test_many_roots_skewed_bins_small_chunks_and_poisoned_samples(libfdg, cuda):
    """parquet_ver4_4 (R = 180): n_bin = 1024 takes the root-slice loop; 90 % of the samples in bin 0; FDG_ROOT_SCRATCH_MB=1 cuts the
    batch into about thirty chunks; inf leaves on samples whose bin is out of range reach neither moment."""
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
    leaf, bins, w = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_bins).to(cuda), torch.from_numpy(h_w).to(cuda)
    acc, acc2 = f.accumulate_moments(leaf, bins, n_bin, w, n_sample=B)
    ref = f.accumulate_binned(leaf, bins, n_bin, w, n_sample=B)
    got, got2 = acc.cpu().numpy(), acc2.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(got2).all()
    assert_bits(got, ref.cpu().numpy(), "parquet_ver4_4")
    s1, a1, s2 = host_moments(roots, h_bins, n_bin, h_w)
    assert_close(got, s1, a1, "parquet_ver4_4")
    assert_close(got2, s2, s2, "parquet_ver4_4")


@pytest.mark.parametrize("route", ["split", "fused", None])
def test_mc_moments_routes(libfdg, cuda, fdgopt, route):
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
    w = torch.from_numpy(rng.uniform(0.0, 1.0, size=B)).to(cuda)
    for n_bin, h_bins in ((33, make_bins(rng, B, 33, base=1)), (1, None)):
        bins = None if h_bins is None else torch.from_numpy(h_bins).to(cuda)
        tie = torch.ones(B, dtype=torch.int32, device=cuda) if bins is None else bins
        acc = torch.zeros((n_bin, R), dtype=torch.float64, device=cuda)
        acc2 = torch.zeros_like(acc)
        ref = torch.zeros_like(acc)
        f.handle.mc_accumulate_device_moments(dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, kF, beta, lam, 0 if bins is None else bins.data_ptr(),
                                              1, n_bin, w.data_ptr(), acc.data_ptr(), acc2.data_ptr(), B, st)
        f.handle.mc_accumulate_device_binned(dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, kF, beta, lam, tie.data_ptr(), 1, n_bin, w.data_ptr(),
                                             ref.data_ptr(), B, st)
        torch.cuda.synchronize()
        assert_bits(acc.cpu().numpy(), ref.cpu().numpy(), (route, n_bin))
        s1, a1, s2 = host_moments(root.cpu().numpy(), h_bins, n_bin, w.cpu().numpy(), base=1)
        assert_close(acc.cpu().numpy(), s1, a1, (route, n_bin))
        assert_close(acc2.cpu().numpy(), s2, s2, (route, n_bin))


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
    whole, whole2 = f.accumulate_moments(leaf, bins, n_bin, w)
    m = torch.zeros((2, n_bin, t.n_root), dtype=torch.float64, device=cuda)      # acc, acc2 as halves of one reducible tensor
    h = B // 2
    f.accumulate_moments(leaf[:h], bins[:h], n_bin, w[:h], m[0], m[1])
    f.accumulate_moments(leaf[h:], bins[h:], n_bin, w[h:], m[0], m[1])
    torch.cuda.synchronize()
    s1, a1, s2 = host_moments(oracle.eval_static(t, h_leaf), h_bins, n_bin, h_w)
    assert_close(whole.cpu().numpy(), s1, a1, "whole")
    assert_close(whole2.cpu().numpy(), s2, s2, "whole2")
    assert_close(m[0].cpu().numpy(), whole.cpu().numpy(), a1, "shards")
    assert_close(m[1].cpu().numpy(), whole2.cpu().numpy(), s2, "shards2")


def test_estimator_recovers_the_standard_error(libfdg, cuda):
    """root = leaf, leaves uniform in (0, 1): mean 1/2, standard error sqrt(1/12 / N).  N = 2^20: the sample standard deviation of a
    uniform variable has a relative standard deviation of sqrt((9/5 - 1) / (4 N)) = 4.4e-4, so a 1 % bound on the error bar is over 20 of
    them; the mean must lie within 6 standard errors of 1/2.  Against the host's own numbers on the same leaves the bar is 1e-9 (the
    difference of sums, not statistics)."""
    import torch
    a = fd.Graph([])
    t, _, _ = lower([fd.Graph([a], subgraph_factors=[1.0])])
    assert t.n_leaf == 1 and t.n_root == 1
    f = fd.compile_table(t, specialize="isa")
    N = 1 << 20
    h_leaf = oracle.philox_uniform(N, 1, 11)
    assert np.array_equal(oracle.eval_static(t, h_leaf)[:, 0], h_leaf[:, 0])
    acc, acc2 = f.accumulate_moments(torch.from_numpy(h_leaf).to(cuda))
    mean, err = fd.mc_estimate(acc, acc2, N)
    mean, err = mean.item(), err.item()
    exact = math.sqrt(1.0 / 12.0 / N)
    assert abs(err / exact - 1.0) < 0.01, (err, exact)
    assert abs(mean - 0.5) < 6 * exact, (mean, exact)
    x = h_leaf[:, 0]
    assert abs(mean - x.mean()) <= 1e-12
    assert abs(err / (x.std(ddof=1) / math.sqrt(N)) - 1.0) < 1e-9


def test_accumulate_moments_validates_its_arguments(libfdg, cuda):
    import torch
    t = workloads.get("sigma2")
    f = fd.compile_table(t, specialize="isa")
    B = 1000
    leaf = torch.rand((B, t.n_leaf), dtype=torch.float64, device=cuda)
    bins = torch.zeros(B, dtype=torch.int32, device=cuda)
    with pytest.raises(ValueError):
        f.accumulate_moments(leaf, None, 4)
    with pytest.raises(TypeError):
        f.accumulate_moments(leaf, bins.double(), 4)
    with pytest.raises(ValueError):
        f.accumulate_moments(leaf, bins[:B - 1], 4)
    with pytest.raises(ValueError):
        f.accumulate_moments(leaf, bins, 0)
    acc = torch.zeros((4, t.n_root), dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        f.accumulate_moments(leaf, bins, 4, None, acc, acc)
    with pytest.raises(ValueError):
        f.accumulate_moments(leaf, bins, 4, None, acc, torch.zeros((t.n_root, 4), dtype=torch.float64, device=cuda))
    a, a2 = f.accumulate_moments(leaf)
    assert a.shape == a2.shape == (1, t.n_root)
    assert f.accumulate_moments(leaf, bins, 4)[1].shape == (4, t.n_root)
