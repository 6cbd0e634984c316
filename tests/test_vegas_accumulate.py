"""VEGAS importance sampling on the device (include/fdg.h: fdg_vegas_sample_device, fdg_accumulate_device_vegas,
fdg_mc_accumulate_device_vegas; feynmandiagram.jl_amd/vegas.py).  The sampler is compared bit for bit with the numpy mirror of
tests/test_vegas_host.py; acc / acc2 of the accumulate calls must carry the bits of the moments calls with no bin vector; the training
histogram is compared with a host histogram of the oracle's roots, |d| <= 1e-12 max(1, sum) per (variable, cell) -- every term is a
square, so an entry is its own scale."""
import math
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT
from feynmandiagram_jl_amd.sharding import shard_range
from test_vegas_host import mirror_cells, mirror_map, mirror_refine, mirror_sample

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-12
SPECS = {"interp": False, "hip": True, "isa": "isa"}


def assert_close(got, want, scale, what):
    bad = ~(np.abs(got - want) <= TOL * np.maximum(1.0, scale))
    print(what, "max |d| / max(1, scale) =", float((np.abs(got - want) / np.maximum(1.0, scale)).max()))
    assert not bad.any(), (what, np.argwhere(bad)[:4], np.abs(got - want).max())


def assert_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, np.argwhere(a.view(np.uint64) != b.view(np.uint64))[:4])


def to_tiles(x):
    B, C = x.shape
    T = (B + 63) // 64
    full = np.full((T * 64, C), np.nan)                 # the lanes past n_sample hold nan: they must poison nothing
    full[:B] = x
    return np.ascontiguousarray(full.reshape(T, 64, C).transpose(0, 2, 1))


def leaves(cuda, h_leaf, layout):
    import torch
    if layout == "row":
        return torch.from_numpy(h_leaf).to(cuda)
    if layout == "leaf_major":
        return torch.from_numpy(np.ascontiguousarray(h_leaf.T)).to(cuda).t()
    return torch.from_numpy(to_tiles(h_leaf)).to(cuda)


def host_hist(roots, w, coef, seed, offset, D, G, live=None):
    """(hist [D, G], sum of t, sum of |t|, sum of t * t) from the roots [B, R]: s the left fold of (coef_k * root_k) over the live roots"""
    B, R = roots.shape
    ks = list(range(R)) if live is None else list(live)
    s = None
    for k in ks:
        term = roots[:, k] if coef is None else coef[k] * roots[:, k]
        s = term if s is None else s + term
    t = s if w is None else w * s
    v = t * t
    _, c = mirror_cells(oracle.philox_uniform(B, D, seed, offset), G)
    return np.stack([np.bincount(c[:, d], weights=v, minlength=G) for d in range(D)])


def host_moments(roots, w):
    t = roots if w is None else roots * w[:, None]
    return t.sum(axis=0)[None, :], np.abs(t).sum(axis=0)[None, :], (t * t).sum(axis=0)[None, :]


def refined_grid(rng, D, G):
    """a non-uniform map: a uniform one refined by a random histogram (G = 1 has nothing to refine)"""
    lo = rng.uniform(-3.0, 1.0, size=D)
    g = vegas.uniform_grid(lo, lo + rng.uniform(0.5, 4.0, size=D), G)
    return capi.vegas_refine(g, rng.random((D, G)) ** 3 + 1e-3, 1.0)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("G", [1, 64, 1000, 1024])
@pytest.mark.parametrize("D", [1, 17, 64])
def test_sampler_matches_the_numpy_mirror_bit_for_bit(libfdg, cuda, D, G):
    import torch
    rng = np.random.default_rng(100 * D + G)
    grid = refined_grid(rng, D, G)
    if G > 1:
        assert not np.allclose(np.diff(grid, axis=1), np.diff(grid, axis=1)[:, :1])
    d_grid = torch.from_numpy(grid).to(cuda)
    B, seed, off, C = 10_003, 0x1234_5678_9ABC, 3_000_000_011, D + 3
    col = rng.permutation(C)[:D]                                            # not the identity, three columns left alone
    want_x, want_jac, want_c = mirror_sample(grid, seed, off, B)
    st = torch.cuda.current_stream().cuda_stream
    for major in ("component", "sample"):
        x = torch.full((C, B) if major == "component" else (B, C), -77.0, dtype=torch.float64, device=cuda)
        xs, xc = (1, B) if major == "component" else (C, 1)
        jac = torch.zeros(B, dtype=torch.float64, device=cuda)
        cell = torch.full((D, B), -1, dtype=torch.int32, device=cuda)
        capi.vegas_sample_device(d_grid.data_ptr(), D, G, col, seed, off, x.data_ptr(), xs, xc, jac.data_ptr(), cell.data_ptr(), B, st)
        torch.cuda.synchronize()
        hx = x.cpu().numpy().T if major == "component" else x.cpu().numpy()
        assert_bits(hx[:, col], want_x, ("x", major))
        untouched = [c for c in range(C) if c not in set(col.tolist())]
        assert (hx[:, untouched] == -77.0).all()
        assert_bits(jac.cpu().numpy(), want_jac, ("jac", major))
        assert np.array_equal(cell.cpu().numpy().T, want_c)
    # two halves with offsets are one call; no cell array; the default columns
    x1 = torch.zeros((D, B), dtype=torch.float64, device=cuda)
    j1 = torch.zeros(B, dtype=torch.float64, device=cuda)
    h = 4_097
    capi.vegas_sample_device(d_grid.data_ptr(), D, G, None, seed, off, x1.data_ptr(), 1, B, j1.data_ptr(), 0, h, st)
    capi.vegas_sample_device(d_grid.data_ptr(), D, G, None, seed, off + h, x1.data_ptr() + 8 * h, 1, B, j1.data_ptr() + 8 * h, 0, B - h, st)
    torch.cuda.synchronize()
    assert_bits(x1.cpu().numpy().T, want_x, "halves")
    assert_bits(j1.cpu().numpy(), want_jac, "halves jac")


def test_one_cell_on_the_unit_interval_is_fill_uniform(libfdg, cuda):
    import torch
    D, B, seed, off = 17, 5_001, 99, 123_456_789_012
    d_grid = torch.from_numpy(vegas.uniform_grid([0.0] * D, [1.0] * D, 1)).to(cuda)
    x = torch.zeros((B, D), dtype=torch.float64, device=cuda)
    u = torch.zeros((B, D), dtype=torch.float64, device=cuda)
    jac = torch.zeros(B, dtype=torch.float64, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    capi.vegas_sample_device(d_grid.data_ptr(), D, 1, None, seed, off, x.data_ptr(), D, 1, jac.data_ptr(), 0, B, st)
    capi.fill_uniform_device(u.data_ptr(), B, D, D, 1, seed, off, st)
    torch.cuda.synchronize()
    assert_bits(x.cpu().numpy(), u.cpu().numpy(), "G = 1")
    assert_bits(x.cpu().numpy(), oracle.philox_uniform(B, D, seed, off), "G = 1 against the oracle")
    assert (jac.cpu().numpy() == 1.0).all()


# ---- the accumulate step, leaf form ----------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("name", ["sigma2", "gv_sigma4", "parquet_sigma4"])
def test_accumulate_ties_to_the_moments_call_and_to_the_host_histogram(libfdg, cuda, name, spec):
    import torch
    t = workloads.get(name)
    L, R, B = t.n_leaf, t.n_root, 200_003
    f = fd.compile_table(t, specialize=SPECS[spec])
    h_leaf = oracle.philox_uniform(B, L, 31)
    roots = oracle.eval_static(t, h_leaf)
    rng = np.random.default_rng(7)
    h_w = rng.uniform(-1.0, 2.0, size=B)
    w = torch.from_numpy(h_w).to(cuda)
    h_coef = rng.uniform(-1.0, 1.0, size=R)
    layouts = ["row", "leaf_major"] + (["tiled"] if spec == "isa" else [])
    cases = [(h_w, None, 5, 64, 11, 0), (None, h_coef, 17, 1000, 12, 777_000_000_001), (h_w, h_coef, 1, 1, 13, 5)]
    for layout in layouts:
        leaf = leaves(cuda, h_leaf, layout)
        for hw, coef, D, G, seed, off in cases:
            ww = None if hw is None else w
            acc, acc2, hist = f.accumulate_vegas(leaf, ww, None, seed, off, D, G, coef=coef, n_sample=B)
            ref, ref2 = f.accumulate_moments(leaf, None, 1, ww, n_sample=B)
            again = f.accumulate_vegas(leaf, ww, None, seed, off, D, G, coef=coef, n_sample=B)
            torch.cuda.synchronize()
            what = (name, spec, layout, D, G)
            assert hist.shape == (D, G)
            assert_bits(acc.cpu().numpy(), ref.cpu().numpy(), what)
            assert_bits(acc2.cpu().numpy(), ref2.cpu().numpy(), what)
            for a, b in zip(again, (acc, acc2, hist)):
                assert_bits(a.cpu().numpy(), b.cpu().numpy(), ("twice",) + what)
            want = host_hist(roots, hw, coef, seed, off, D, G)
            assert_close(hist.cpu().numpy(), want, want, what)
            s1, a1, s2 = host_moments(roots, hw)
            assert_close(acc.cpu().numpy(), s1, a1, what)
            assert_close(acc2.cpu().numpy(), s2, s2, what)


def test_a_second_call_adds_on_top(libfdg, cuda):
    import torch
    t = workloads.get("parquet_sigma4")
    L, R, B, D, G, seed, off = t.n_leaf, t.n_root, 100_001, 6, 128, 3, 1 << 40
    f = fd.compile_table(t, specialize="isa")
    h_leaf = oracle.philox_uniform(B, L, 5)
    roots = oracle.eval_static(t, h_leaf)
    leaf = torch.from_numpy(to_tiles(h_leaf)).to(cuda)
    rng = np.random.default_rng(3)
    h_w = rng.uniform(0.5, 1.5, size=B)
    w = torch.from_numpy(h_w).to(cuda)
    p1 = torch.from_numpy(rng.uniform(-3.0, 3.0, size=(1, R))).to(cuda)
    p2 = torch.from_numpy(rng.uniform(0.0, 3.0, size=(1, R))).to(cuda)
    ph = torch.from_numpy(rng.uniform(0.0, 3.0, size=(D, G))).to(cuda)
    a1, q1, g1 = f.accumulate_vegas(leaf, w, ph.clone(), seed, off, D, G, acc=p1.clone(), acc2=p2.clone(), n_sample=B)
    a2, q2, g2 = f.accumulate_vegas(leaf, w, ph.clone(), seed, off, D, G, acc=p1.clone(), acc2=p2.clone(), n_sample=B)
    m1, m2 = f.accumulate_moments(leaf, None, 1, w, p1.clone(), p2.clone(), n_sample=B)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and torch.equal(q1, q2) and torch.equal(g1, g2)
    assert torch.equal(a1, m1) and torch.equal(q1, m2)
    want = host_hist(roots, h_w, None, seed, off, D, G)
    assert_close(g1.cpu().numpy(), ph.cpu().numpy() + want, ph.cpu().numpy() + want, "hist on top")
    f.accumulate_vegas(leaf, w, g1, seed, off, D, G, acc=a1, acc2=q1, n_sample=B)
    assert_close(g1.cpu().numpy(), ph.cpu().numpy() + 2 * want, ph.cpu().numpy() + 2 * want, "hist twice")
    s1, a_1, s2 = host_moments(roots, h_w)
    assert_close(a1.cpu().numpy(), p1.cpu().numpy() + 2 * s1, 2 * a_1 + np.abs(p1.cpu().numpy()), "acc twice")
    assert_close(q1.cpu().numpy(), p2.cpu().numpy() + 2 * s2, 2 * s2 + p2.cpu().numpy(), "acc2 twice")


@pytest.mark.parametrize("spec", list(SPECS))
def test_missing_root_is_skipped(libfdg, cuda, spec):
    """A root that does not exist (FDG_NO_ROOT) enters neither moment nor the histogram, whatever its factor says."""
    import torch
    a, b, c = fd.Graph([]), fd.Graph([]), fd.Graph([])
    s = a + b
    p = fd.Graph([s, c, a], subgraph_factors=[1.0, -0.5, 2.0], operator=fd.Prod())
    t, _, _ = lower([s, p], root=[s.id, 424242, p.id])
    assert int(t.root_slot[1]) == FDG_NO_ROOT
    f = fd.compile_table(t, specialize=SPECS[spec])
    B, D, G, seed, off = 5_000, 4, 32, 8, 100
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 9) + 0.25
    roots = oracle.eval_static(t, h_leaf)
    leaf = torch.from_numpy(h_leaf).to(cuda)
    for coef in (None, np.array([0.5, float("nan"), -2.0])):
        acc = torch.full((1, t.n_root), -7.0, dtype=torch.float64, device=cuda)
        acc2 = torch.full((1, t.n_root), 5.0, dtype=torch.float64, device=cuda)
        _, _, hist = f.accumulate_vegas(leaf, None, None, seed, off, D, G, coef=coef, acc=acc, acc2=acc2)
        got, got2 = acc.cpu().numpy(), acc2.cpu().numpy()
        assert got[0, 1] == -7.0 and got2[0, 1] == 5.0
        want = host_hist(roots, None, coef, seed, off, D, G, live=[0, 2])
        assert np.isfinite(hist.cpu().numpy()).all()
        assert_close(hist.cpu().numpy(), want, want, (spec, coef is None))


def test_many_roots_small_chunks_many_slices_and_poisoned_lanes(libfdg, cuda):
    """parquet_ver4_4 (R = 180) with FDG_ROOT_SCRATCH_MB=1: about thirty chunks; D = 64, G = 1024: eight slices of the variables per
    segment; the tile-major batch holds nan in the lanes past n_sample."""
    import torch
    t = workloads.get("parquet_ver4_4")
    L, R, B, D, G, seed, off = t.n_leaf, t.n_root, 20_011, capi.FDG_VEGAS_DIM_MAX, capi.FDG_VEGAS_GRID_MAX, 21, 9_999_999_937
    f = fd.compile_table(t, specialize="isa", options={"FDG_ROOT_SCRATCH_MB": "1"})
    h_leaf = oracle.philox_uniform(B, L, 17)
    roots = oracle.eval_static(t, h_leaf)
    rng = np.random.default_rng(23)
    h_w = rng.uniform(0.0, 1.0, size=B)
    h_coef = rng.uniform(-1.0, 1.0, size=R)
    tiles = to_tiles(h_leaf)
    assert np.isnan(tiles[-1, :, B % 64:]).all()
    leaf, w = torch.from_numpy(tiles).to(cuda), torch.from_numpy(h_w).to(cuda)
    acc, acc2, hist = f.accumulate_vegas(leaf, w, None, seed, off, D, G, coef=h_coef, n_sample=B)
    ref, ref2 = f.accumulate_moments(leaf, None, 1, w, n_sample=B)
    again = f.accumulate_vegas(leaf, w, None, seed, off, D, G, coef=h_coef, n_sample=B)
    torch.cuda.synchronize()
    got = hist.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(acc.cpu().numpy()).all()
    assert_bits(acc.cpu().numpy(), ref.cpu().numpy(), "acc")
    assert_bits(acc2.cpu().numpy(), ref2.cpu().numpy(), "acc2")
    assert_bits(again[2].cpu().numpy(), got, "twice")
    want = host_hist(roots, h_w, h_coef, seed, off, D, G)
    assert_close(got, want, want, "parquet_ver4_4")
    # every variable's histogram holds the whole sum once
    assert np.allclose(got.sum(axis=1), want[0].sum(), rtol=1e-10)


# ---- the accumulate step, Monte-Carlo form ---------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("route", ["split", "fused", None])
def test_mc_vegas_routes(libfdg, cuda, fdgopt, route):
    import torch
    z = dict(np.load(os.path.join(GOLD, "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    R = t.n_root
    B, dim, n_loop, n_tau = 50_001, 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam = 1.919, 3.0, 1.2
    nk, C = n_loop * dim, n_loop * dim + n_tau
    col = list(range(dim, nk)) + list(range(nk + 1, C))                     # the external momentum and T[1] stay fixed
    D, G, seed, off = len(col), 48, 77, 12_345_678_901
    rng = np.random.default_rng(13)
    lo = np.array([-2.0] * (nk - dim) + [0.0] * (n_tau - 1))
    hi = np.array([2.0] * (nk - dim) + [beta] * (n_tau - 1))
    grid = capi.vegas_refine(vegas.uniform_grid(lo, hi, G), rng.random((D, G)) + 0.05, 1.0)
    d_grid = torch.from_numpy(grid).to(cuda)
    fixed = np.zeros(C)
    fixed[0] = kF
    x = torch.from_numpy(fixed).to(cuda)[:, None].repeat(1, B).contiguous()
    jac = torch.zeros(B, dtype=torch.float64, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    capi.vegas_sample_device(d_grid.data_ptr(), D, G, col, seed, off, x.data_ptr(), 1, B, jac.data_ptr(), 0, B, st)
    want_x, want_jac, _ = mirror_sample(grid, seed, off, B)
    torch.cuda.synchronize()
    assert_bits(x.cpu().numpy()[col].T, want_x, "x")
    assert (x.cpu().numpy()[0] == kF).all() and (x.cpu().numpy()[nk] == 0.0).all()
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    if route:
        fdgopt.set("FDG_MC_ROUTE", route)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    dK, dT = x.data_ptr(), x.data_ptr() + 8 * nk * B
    root = torch.zeros((B, R), dtype=torch.float64, device=cuda)
    f.handle.mc_eval_device(dK, 1, B, dT, 1, B, kF, beta, lam, root.data_ptr(), R, 1, B, st)
    h_coef = rng.uniform(-1.0, 1.0, size=R)
    for coef in (None, h_coef):
        m = torch.zeros((2, 2, R), dtype=torch.float64, device=cuda)        # [call][moment][root]
        ref = torch.zeros((2, R), dtype=torch.float64, device=cuda)
        hist = torch.zeros((2, D, G), dtype=torch.float64, device=cuda)
        for i in range(2):
            f.handle.mc_accumulate_device_vegas(dK, 1, B, dT, 1, B, kF, beta, lam, jac.data_ptr(), coef, seed, off, D, G, m[i, 0].data_ptr(),
                                                m[i, 1].data_ptr(), hist[i].data_ptr(), B, st)
        f.handle.mc_accumulate_device_moments(dK, 1, B, dT, 1, B, kF, beta, lam, 0, 0, 1, jac.data_ptr(), ref[0].data_ptr(), ref[1].data_ptr(), B, st)
        torch.cuda.synchronize()
        what = (route, coef is None)
        assert_bits(m[0].cpu().numpy(), ref.cpu().numpy(), what)
        assert_bits(m[1].cpu().numpy(), m[0].cpu().numpy(), ("twice",) + what)
        assert_bits(hist[1].cpu().numpy(), hist[0].cpu().numpy(), ("twice",) + what)
        h_root, h_jac = root.cpu().numpy(), jac.cpu().numpy()
        want = host_hist(h_root, h_jac, coef, seed, off, D, G)
        assert_close(hist[0].cpu().numpy(), want, want, what)
        s1, a1, s2 = host_moments(h_root, h_jac)
        assert_close(m[0, 0].cpu().numpy()[None, :], s1, a1, what)
        assert_close(m[0, 1].cpu().numpy()[None, :], s2, s2, what)


def one_bosonic_leaf(order):
    """a one-root graph over one leaf, and the tables that make the leaf 8 pi (|K_1|^2 + lambda) (lambda / (|K_1|^2 + lambda))^order"""
    a = fd.Graph([])
    t, _, _ = lower([fd.Graph([a], subgraph_factors=[1.0])])
    assert t.n_leaf == 1 and t.n_root == 1
    tab, keep = capi.make_leaf_tables([2], [order], [1], [1], [1], np.array([[1.0]]), 3, 1)
    return t, tab, keep


def test_known_answer(libfdg, cuda):
    """The integral of 8 pi (|K|^2 + lambda) over [-L, L]^3 is 64 pi L^3 (lambda + L^2) = 6514.4 at L = 2, lambda = 0.05.  The Philox-driven
    numpy mirror at this seed gives 6511.8 +- 7.4 in the first iteration and stays within 1.5 reported errors in each of six."""
    t, tab, _keep = one_bosonic_leaf(0)
    f = fd.compile_table(t, specialize="isa")
    L, lam = 2.0, 0.05
    res = vegas.vegas_integrate(f, tab, [-L] * 3, [L] * 3, [0, 1, 2], 0.0, 1.0, lam, n_iter=4, n_sample=200_000, n_grid=64, alpha=0.5,
                                seed=2024, device=cuda)
    exact = 64.0 * math.pi * L ** 3 * (lam + L * L)
    print("known answer:", res.mean, res.stderr, res.chi2_dof, exact, res.iterations)
    assert res.mean.shape == res.stderr.shape == (1,) and len(res.iterations) == 4
    assert res.stderr[0] > 0 and abs(res.mean[0] - exact) < 5.0 * res.stderr[0]
    m0, e0 = res.iterations[0]
    assert abs(m0[0] - exact) < 5.0 * e0[0] and 5.0 < e0[0] < 10.0       # a flat map over 2e5 samples: 7.4 on the CPU
    assert res.map.grid.shape == (3, 65) and (np.diff(res.map.grid, axis=1) > 0).all()


def test_adaptation_on_a_peaked_integrand(libfdg, cuda):
    """8 pi lambda^2 / (|K|^2 + lambda), lambda = 0.05, over [-2, 2]^3; G = 64, 2e5 samples, 6 iterations, alpha = 0.5.  The Philox-driven
    numpy mirror on the CPU with this seed (2024) gives standard errors 5.79e-3, 3.82e-3, 2.70e-3, 2.14e-3, 1.84e-3, 1.68e-3: the last
    is 0.2905 of the first (the condition below is one half).  Per iteration acc, acc2 and hist are checked against host sums over the
    roots mc_eval_device gives on the same samples, and the refined grid against the numpy mirror of the refinement."""
    import torch
    t, tab, _keep = one_bosonic_leaf(2)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    L, lam, G, B, n_iter, seed, D = 2.0, 0.05, 64, 200_000, 6, 2024, 3
    vm = vegas.VegasMap(vegas.uniform_grid([-L] * 3, [L] * 3, G), cuda)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros((4, B), dtype=torch.float64, device=cuda)                # three momentum components, one time
    jac = torch.zeros(B, dtype=torch.float64, device=cuda)
    root = torch.zeros((B, 1), dtype=torch.float64, device=cuda)
    dK, dT = x.data_ptr(), x.data_ptr() + 8 * 3 * B
    errs, means = [], []
    for it in range(n_iter):
        off = it * B
        capi.vegas_sample_device(vm.d_grid.data_ptr(), D, G, [0, 1, 2], seed, off, dK, 1, B, jac.data_ptr(), 0, B, st)
        m = torch.zeros((2, 1, 1), dtype=torch.float64, device=cuda)
        hist = torch.zeros((D, G), dtype=torch.float64, device=cuda)
        f.handle.mc_accumulate_device_vegas(dK, 1, B, dT, 1, B, 0.0, 1.0, lam, jac.data_ptr(), None, seed, off, D, G, m[0].data_ptr(),
                                            m[1].data_ptr(), hist.data_ptr(), B, st)
        f.handle.mc_eval_device(dK, 1, B, dT, 1, B, 0.0, 1.0, lam, root.data_ptr(), 1, 1, B, st)
        torch.cuda.synchronize()
        want_x, want_jac, _ = mirror_map(vm.grid, oracle.philox_uniform(B, D, seed, off))
        assert_bits(x.cpu().numpy()[:3].T, want_x, ("x", it))
        assert_bits(jac.cpu().numpy(), want_jac, ("jac", it))
        h_root = root.cpu().numpy()
        q2 = (want_x * want_x).sum(axis=1)
        assert np.allclose(h_root[:, 0], 8 * math.pi * lam * lam / (q2 + lam), rtol=1e-12)
        s1, a1, s2 = host_moments(h_root, want_jac)
        assert_close(m[0].cpu().numpy(), s1, a1, ("acc", it))
        assert_close(m[1].cpu().numpy(), s2, s2, ("acc2", it))
        want_h = host_hist(h_root, want_jac, None, seed, off, D, G)
        h = hist.cpu().numpy()
        assert_close(h, want_h, want_h, ("hist", it))
        mean, err = fd.mc_estimate(m[0], m[1], B)
        means.append(mean.item())
        errs.append(err.item())
        before = vm.grid.copy()
        vm.refine(hist, 0.5)
        assert np.abs(vm.grid - mirror_refine(before, h, 0.5)).max() <= 1e-12 * 2 * L, it
        assert_bits(vm.d_grid.cpu().numpy(), vm.grid, ("uploaded", it))
        assert (np.diff(vm.grid, axis=1) > 0).all()
    print("adaptation: means", means, "errors", errs, "ratio", errs[-1] / errs[0])
    assert errs[-1] < 0.5 * errs[0], errs
    # the driver walks the same iterations: the same bits
    res = vegas.vegas_integrate(f, tab, [-L] * 3, [L] * 3, [0, 1, 2], 0.0, 1.0, lam, n_iter=n_iter, n_sample=B, n_grid=G, alpha=0.5, seed=seed,
                                device=cuda, n_discard=1, specialize_fused=False)
    assert [a[0] for a, _ in res.iterations] == means and [b[0] for _, b in res.iterations] == errs
    assert_bits(res.map.grid, vm.grid, "the driver's map")
    mean, err, chi2 = vegas.combine([(np.array([a]), np.array([b])) for a, b in zip(means[1:], errs[1:])])
    assert res.mean[0] == mean[0] and res.stderr[0] == err[0] and res.stderr[0] < min(errs)


def test_two_shards_add_up_to_the_batch(libfdg, cuda):
    import torch
    t = workloads.get("gv_sigma4")
    B, D, G, seed, base = 70_001, 9, 100, 4, 1_000_000
    f = fd.compile_table(t, specialize="isa")
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 2)
    rng = np.random.default_rng(4)
    h_w = rng.uniform(-1.0, 1.0, size=B)
    leaf, w = torch.from_numpy(h_leaf).to(cuda), torch.from_numpy(h_w).to(cuda)
    whole = f.accumulate_vegas(leaf, w, None, seed, base, D, G)
    m = torch.zeros((2, 1, t.n_root), dtype=torch.float64, device=cuda)
    hist = torch.zeros((D, G), dtype=torch.float64, device=cuda)
    for rank in range(2):
        s, n = shard_range(B, rank, 2)
        f.accumulate_vegas(leaf[s:s + n], w[s:s + n], hist, seed, base + s, D, G, acc=m[0], acc2=m[1])
        one = f.accumulate_vegas(leaf[s:s + n], w[s:s + n], None, seed, base + s, D, G)
        two = f.accumulate_vegas(leaf[s:s + n], w[s:s + n], None, seed, base + s, D, G)
        for a, b in zip(one, two):
            assert torch.equal(a, b), rank                                  # each shard is bitwise repeatable
    torch.cuda.synchronize()
    roots = oracle.eval_static(t, h_leaf)
    s1, a1, s2 = host_moments(roots, h_w)
    want = host_hist(roots, h_w, None, seed, base, D, G)
    assert_close(whole[2].cpu().numpy(), want, want, "whole")
    assert_close(m[0].cpu().numpy(), whole[0].cpu().numpy(), a1, "shards acc")
    assert_close(m[1].cpu().numpy(), whole[1].cpu().numpy(), s2, "shards acc2")
    assert_close(hist.cpu().numpy(), whole[2].cpu().numpy(), want, "shards hist")


def test_accumulate_vegas_validates_its_arguments(libfdg, cuda):
    import torch
    t = workloads.get("sigma2")
    f = fd.compile_table(t, specialize="isa")
    B = 1000
    leaf = torch.rand((B, t.n_leaf), dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        f.accumulate_vegas(leaf, None, None, 1, 0, 0, 8)
    with pytest.raises(ValueError):
        f.accumulate_vegas(leaf, None, None, 1, 0, 3, capi.FDG_VEGAS_GRID_MAX + 1)
    with pytest.raises(ValueError):
        f.accumulate_vegas(leaf, None, torch.zeros((8, 3), dtype=torch.float64, device=cuda), 1, 0, 3, 8)
    acc = torch.zeros((1, t.n_root), dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        f.accumulate_vegas(leaf, None, None, 1, 0, 3, 8, acc=acc, acc2=acc)
    with pytest.raises(ValueError):
        f.accumulate_vegas(leaf, None, None, 1, 0, 3, 8, coef=[1.0] * (t.n_root + 1))
    a, a2, h = f.accumulate_vegas(leaf, None, None, 1, 0, 3, 8)
    assert a.shape == a2.shape == (1, t.n_root) and h.shape == (3, 8)
