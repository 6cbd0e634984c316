"""Observables on the device (include/fdg.h: fdg_accumulate_device_observables, fdg_mc_accumulate_device_observables;
GraphFunc.accumulate_observables, vegas.Observables): o_m = the left fold over k of coef[m][k] w_g(k) root_k, d_obs[j][m] += o_m and
d_cov[j][a][c] += o_a o_c over the samples of bin j.

Host reference: capi.observables_reference on the oracle's roots (on the handle's own mc_eval_device roots for the Monte-Carlo form).
Tolerance, the convention of tests/test_moments_accumulate.py: |got - want| <= 1e-12 max(1, sum |terms|), the terms |o_m| of an
entry of d_obs and |o_a o_c| of an entry of d_cov.  A unit row carries the bits of the moments call; the other blocks of a call carry
the bits of the same call without observables."""
import functools
import math
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from test_matsubara_accumulate import leaves, make_bins, random_table
from test_weight_groups_accumulate import BETA, D0, FREQ, G0, N_TAU, SETS, SPECS, assert_bits, grouped_call, leaf_strides

pytestmark = pytest.mark.gpu

TOL = 1e-12
B0 = 8_229
SENTINEL = -7.0


def obs_call(f, leaf, B, cuda, coef, w=None, rg=None, sets=None, bins=None, n_bin=1, bin_base=0, train=None, tcoef=None, mz=None,
             moments=False, out=None, fill=0.0):
    """One fdg_accumulate_device_observables call.  w: None, a [B] or (with rg and sets) a [n_group, B] CUDA tensor; train: (seed,
    offset, D, G) or None; mz: (T tensor, freq, fermionic, tin, tout) or None; out: the dict of a previous call, added to; fill: what
    obs and cov start from.  Returns the dict of output tensors."""
    import torch
    R, M = f.n_root, len(coef)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    if out is None:
        out = {"obs": z(n_bin, M) + fill, "cov": z(n_bin, M, M) + fill}
        if moments:
            out.update(acc=z(n_bin, R), acc2=z(n_bin, R))
        if train:
            out["hist"] = z(train[2], train[3])
            if bins is not None:
                out["hist_bin"] = z(n_bin)
        if mz:
            out["mz"] = z(4, n_bin, len(mz[1]), R)
    wg = None
    if rg is not None:
        wg, _keep = capi.make_weight_groups(rg, sets, w.stride(0))
    desc = None
    if mz:
        T, freq, fermionic, tin, tout = mz
        desc, _keep2 = capi.make_matsubara(freq, fermionic, tin, tout, BETA, T.shape[1], *[out["mz"][i].data_ptr() for i in range(4)],
                                           T.data_ptr(), T.stride(0), T.stride(1))
    ob, _keep3 = capi.make_observables(coef, out["obs"].data_ptr(), out["cov"].data_ptr())
    seed, off, D, G = train or (0, 0, 0, 0)
    f.handle.accumulate_device_observables(leaf.data_ptr(), *leaf_strides(leaf), 0 if bins is None else bins.data_ptr(), bin_base, n_bin,
                                           0 if w is None else w.data_ptr(), ob, wg, desc, tcoef, seed, off, D, G,
                                           out["acc"].data_ptr() if "acc" in out else 0, out["acc2"].data_ptr() if "acc2" in out else 0,
                                           out["hist"].data_ptr() if train else 0, out["hist_bin"].data_ptr() if "hist_bin" in out else 0, B,
                                           torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    return out


def assert_obs(got, want, what, fill=0.0):
    """got: the dict of obs_call (or a pair of arrays); want: capi.observables_reference's tuple.  Entries of rows without a term
    (nan in the reference) must hold ``fill`` untouched; the others ``fill`` plus the reference within the tolerance."""
    o, c = (got["obs"].cpu().numpy(), got["cov"].cpu().numpy()) if isinstance(got, dict) else got
    for key, g, ref, scale in (("obs", o, want[0], want[2]), ("cov", c, want[1], want[3])):
        dead = np.isnan(ref)
        assert (g[dead] == fill).all(), (what, key, "a row without a term was written")
        err = np.abs(g[~dead] - fill - ref[~dead])
        bound = TOL * np.maximum(1.0, scale[~dead])
        print(what, key, "max |got - want| / bound:", float((err / bound).max()) if err.size else 0.0)
        assert (err <= bound).all(), (what, key, float((err / bound).max()))
    assert_bits(c, c.transpose(0, 2, 1), (what, "cov and its mirror"))


@functools.lru_cache(maxsize=None)
def batch(name):
    t = workloads.get(name)
    h_leaf = oracle.philox_uniform(B0, t.n_leaf, 31)
    rng = np.random.default_rng(7)
    w = rng.uniform(-1.0, 2.0, size=(3, B0))
    bins = make_bins(rng, B0, 7, base=1)
    T = rng.uniform(0.0, BETA, size=(B0, N_TAU))
    T[:, 0] = 0.0
    return t, h_leaf, oracle.eval_static(t, h_leaf), w, bins, T


# ---- 1. a unit row is the moments call, bit for bit -------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("name", ["sigma2", "parquet_sigma4"])
def test_unit_rows_carry_the_bits_of_the_moments_call(libfdg, cuda, name, spec):
    import torch
    t, h_leaf, _, h_w, h_bins, _ = batch(name)
    f = fd.compile_table(t, specialize=SPECS[spec])
    R = t.n_root
    M = min(R, capi.FDG_OBS_MAX)
    eye = np.eye(R)[:M]
    w, bins = torch.from_numpy(h_w[0].copy()).to(cuda), torch.from_numpy(h_bins).to(cuda)
    for layout in ["leaf_major"] + (["tiled"] if spec == "isa" else ["row"]):
        leaf = leaves(cuda, h_leaf, layout)
        for kw in (dict(), dict(bins=bins, n_bin=7, bin_base=1)):
            a, a2 = f.accumulate_moments(leaf, weight=w, n_sample=B0, **kw)
            o, c = f.accumulate_observables(leaf, eye, weight=w, n_sample=B0, **kw)
            torch.cuda.synchronize(cuda)
            a, a2, o, c = (x.cpu().numpy() for x in (a, a2, o, c))
            assert np.abs(a).max() > 0
            assert_bits(o, a[:, :M], (layout, sorted(kw), "obs against acc"))
            assert_bits(np.einsum("jmm->jm", c), a2[:, :M], (layout, sorted(kw), "the diagonal of cov against acc2"))
            assert_bits(c, c.transpose(0, 2, 1), (layout, sorted(kw), "cov and its mirror"))
            # ... and the per-root moments beside the observables are the moments call's too
            o2, c2, b, b2 = f.accumulate_observables(leaf, eye, weight=w, n_sample=B0, moments=True, **kw)
            torch.cuda.synchronize(cuda)
            assert_bits(b.cpu().numpy(), a, (layout, "acc beside the observables"))
            assert_bits(b2.cpu().numpy(), a2, (layout, "acc2 beside the observables"))
            assert_bits(o2.cpu().numpy(), o, (layout, "obs beside the moments"))
            assert_bits(c2.cpu().numpy(), c, (layout, "cov beside the moments"))


# ---- 2. against numpy ---------------------------------------------------------------------------------------------------------------------- #
def random_coef(rng, M, R, zero_row=None):
    c = rng.uniform(-1.5, 1.5, size=(M, R))
    c[rng.random((M, R)) < 0.3] = 0.0                                         # exact zeros: not terms of the fold
    for m in range(M):
        if not c[m].any():
            c[m, m % R] = 1.25
    if zero_row is not None:
        c[zero_row] = 0.0
    return c


@pytest.mark.parametrize("n_obs", [1, 3, 16])
def test_random_rows_match_numpy(libfdg, cuda, n_obs):
    import torch
    t, h_leaf, roots, h_w, h_bins, _ = batch("parquet_sigma4")
    f = fd.compile_table(t, specialize="isa")
    R = t.n_root
    zero_row = None if n_obs == 1 else n_obs // 2
    coef = random_coef(np.random.default_rng(100 + n_obs), n_obs, R, zero_row)
    assert (coef == 0.0).any() or n_obs == 1
    leaf = leaves(cuda, h_leaf, "tiled")
    w, bins = torch.from_numpy(h_w[0].copy()).to(cuda), torch.from_numpy(h_bins).to(cuda)
    want = capi.observables_reference(roots, coef, h_w[0], None, h_bins, 7, 1)
    if zero_row is not None:
        assert np.isnan(want[0][:, zero_row]).all() and np.isnan(want[1][:, zero_row, :]).all()
    args = dict(w=w, bins=bins, n_bin=7, bin_base=1)
    # prefilled arrays grow by the increment; the all-zero row keeps what was there
    got = obs_call(f, leaf, B0, cuda, coef, fill=SENTINEL, **args)
    assert_obs(got, want, ("n_obs", n_obs), fill=SENTINEL)
    again = obs_call(f, leaf, B0, cuda, coef, fill=SENTINEL, **args)
    for key in ("obs", "cov"):
        assert_bits(again[key].cpu().numpy(), got[key].cpu().numpy(), ("the same arguments, the same bits", key))
    # no weights, no bin vector
    assert_obs(obs_call(f, leaf, B0, cuda, coef), capi.observables_reference(roots, coef), ("no weights, one bin", n_obs))


# ---- 3. chunks and slices -------------------------------------------------------------------------------------------------------------------- #
def test_chunks_slices_groups_poisoned_samples_and_shards(libfdg, cuda):
    """FDG_ROOT_SCRATCH_MB = 1 with 19 roots (root 7 does not exist): eleven chunks of 6 848 samples; 16 observables over 3 000 bins: 152
    value columns in slices of two; four weight groups; inf and nan weights and leaves on samples whose bin is out of range reach no sum."""
    import torch
    rng = np.random.default_rng(5)
    t = random_table(rng)
    R, B, n_bin, missing, M = t.n_root, 70_003, 3_000, 7, 16
    exists = np.arange(R) != missing
    rg = [k % 4 for k in range(R)]
    sets = [(0, 1), (1, 2, 3), (0, 4), (2, 5)]
    f = fd.compile_table(t, specialize="isa", options={"FDG_ROOT_SCRATCH_MB": "1"})
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 17) + 0.25
    h_bins = make_bins(rng, B, n_bin, base=0)
    h_w = rng.uniform(0.1, 2.0, size=(4, B))
    out_of_range = np.flatnonzero((h_bins < 0) | (h_bins >= n_bin))
    assert out_of_range.size > 500
    h_leaf[out_of_range[0::3], 0], h_leaf[out_of_range[1::3], 1] = np.inf, np.nan
    h_w[1, out_of_range[2::3]], h_w[2, out_of_range[0::2]] = np.nan, np.inf
    roots = oracle.eval_static(t, h_leaf)
    coef = random_coef(rng, M, R, zero_row=5)
    coef[3] = 0.0
    coef[3, missing] = 2.0                                                    # a row whose only factor sits on the root that does not exist
    leaf, w, bins = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins).to(cuda)
    with np.errstate(invalid="ignore", over="ignore"):
        want = capi.observables_reference(roots, coef, h_w, rg, h_bins, n_bin, 0, exists)
    assert np.isnan(want[0][:, [3, 5]]).all() and np.isfinite(np.delete(want[0], [3, 5], axis=1)).all()
    got = obs_call(f, leaf, B, cuda, coef, w=w, rg=rg, sets=sets, bins=bins, n_bin=n_bin, fill=SENTINEL)
    assert_obs(got, want, "19 roots, 4 groups, 3000 bins", fill=SENTINEL)
    # two shards added together (the cut on a chunk boundary of neither)
    cut = 64 * 517
    o = obs_call(f, leaf, cut, cuda, coef, w=w, rg=rg, sets=sets, bins=bins, n_bin=n_bin, fill=SENTINEL)
    obs_call(f, leaves(cuda, h_leaf[cut:], "tiled"), B - cut, cuda, coef, w=w[:, cut:], rg=rg, sets=sets, bins=bins[cut:], n_bin=n_bin, out=o)
    assert_obs(o, want, "two shards", fill=SENTINEL)
    # one column of 16 384 bins: the histogram of FDG_BIN_MAX bins
    nb = capi.FDG_BIN_MAX
    h_b2 = make_bins(rng, B, nb, base=0)
    row = coef[:1]
    ok = (h_b2 >= 0) & (h_b2 < nb)
    # (the poisoned samples of the first bin vector may be in range of this one: clean copies of what they poisoned)
    h_leaf2, h_w2 = h_leaf.copy(), h_w.copy()
    bad = ~np.isfinite(h_leaf2).all(axis=1) | ~np.isfinite(h_w2).all(axis=0)
    h_leaf2[bad], h_w2[:, bad] = 0.5, 1.0
    h_leaf2[~ok, 0], h_w2[0, ~ok] = np.nan, np.inf
    roots2 = oracle.eval_static(t, h_leaf2)
    with np.errstate(invalid="ignore", over="ignore"):
        want = capi.observables_reference(roots2, row, h_w2, rg, h_b2, nb, 0, exists)
    got = obs_call(f, leaves(cuda, h_leaf2, "tiled"), B, cuda, row, w=torch.from_numpy(h_w2).to(cuda), rg=rg, sets=sets,
                   bins=torch.from_numpy(h_b2).to(cuda), n_bin=nb)
    assert_obs(got, want, "16384 bins, one observable")


# ---- 4. beside the other blocks ---------------------------------------------------------------------------------------------------------------- #
def test_other_blocks_keep_their_bits(libfdg, cuda):
    import torch
    t, h_leaf, roots, h_w, h_bins, h_T = batch("parquet_sigma4")
    f = fd.compile_table(t, specialize="isa")
    R = t.n_root
    rg = [0, 1, 1, 2]
    tin, tout = workloads.root_times("parquet_sigma4")
    w = torch.from_numpy(np.abs(h_w) + 0.1).to(cuda)
    bins, d_T = torch.from_numpy(h_bins).to(cuda), torch.from_numpy(h_T).to(cuda)
    leaf = leaves(cuda, h_leaf, "tiled")
    coef = random_coef(np.random.default_rng(9), 3, R)
    tcoef = [0.5, -1.25, 2.0, 1.0]
    blocks = dict(bins=bins, n_bin=7, bin_base=1, train=(9, 4_000, D0, G0), mz=(d_T, FREQ, True, tin, tout))
    ref = grouped_call(f, leaf, w, rg, SETS, B0, cuda, coef=tcoef, **blocks)
    got = obs_call(f, leaf, B0, cuda, coef, w=w, rg=rg, sets=SETS, tcoef=tcoef, moments=True, **blocks)
    assert set(ref) == set(got) - {"obs", "cov"}
    for key in ref:
        assert np.abs(ref[key].cpu().numpy()).max() > 0, key
        assert_bits(got[key].cpu().numpy(), ref[key].cpu().numpy(), ("beside the observables", key))
    assert_obs(got, capi.observables_reference(roots, coef, np.abs(h_w) + 0.1, rg, h_bins, 7, 1), "beside training and projection")
    # wg NULL: the other outputs are the ungrouped call's
    a, a2, h, hb = f.accumulate_vegas_binned(leaf, bins, 7, w[0], None, None, 9, 4_000, D0, G0, coef=tcoef, bin_base=1, n_sample=B0)
    got = obs_call(f, leaf, B0, cuda, coef, w=w[0], tcoef=tcoef, moments=True, bins=bins, n_bin=7, bin_base=1, train=(9, 4_000, D0, G0))
    for key, r in (("acc", a), ("acc2", a2), ("hist", h), ("hist_bin", hb)):
        assert_bits(got[key].cpu().numpy(), r.cpu().numpy(), ("no groups", key))
    assert_obs(got, capi.observables_reference(roots, coef, np.abs(h_w[0]) + 0.1, None, h_bins, 7, 1), "no groups")


# ---- 5. the Monte-Carlo routes ----------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("route", ["split", "fused", None])
def test_mc_routes(libfdg, cuda, fdgopt, route):
    """fdg_mc_accumulate_device_observables on every route, T component-major and sample-major, against the same handle's
    mc_eval_device roots combined in numpy (the pattern of tests/test_weight_groups_accumulate.py::test_mc_routes)."""
    import torch
    z = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    R = t.n_root
    B, dim, n_loop, n_tau = 20_011, 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam = 1.919, 3.0, 1.2
    nk, C = n_loop * dim, n_loop * dim + n_tau
    col = list(range(dim, nk)) + list(range(nk + 1, C))
    D, G, seed, off = len(col), 48, 77, 12_345_678_901
    rng = np.random.default_rng(13)
    lo = np.array([-2.0] * (nk - dim) + [0.0] * (n_tau - 1))
    hi = np.array([2.0] * (nk - dim) + [beta] * (n_tau - 1))
    grid = capi.vegas_refine(vegas.uniform_grid(lo, hi, G), rng.random((D, G)) + 0.05, 1.0)
    d_grid = torch.from_numpy(grid).to(cuda)
    fixed = np.zeros(C)
    fixed[0] = kF
    x = torch.from_numpy(fixed).to(cuda)[:, None].repeat(1, B).contiguous()
    sets = [tuple(range(D // 3)), tuple(range(2 * D // 3)), tuple(range(D))]
    rg = [k % 3 for k in range(R)]
    jac = torch.zeros((3, B), dtype=torch.float64, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    capi.vegas_sample_device_grouped(d_grid.data_ptr(), D, G, col, 0, 1, 0, 0, None, None, sets, B, seed, off, x.data_ptr(), 1, B, jac.data_ptr(),
                                     0, 0, B, st)
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    if route:
        fdgopt.set("FDG_MC_ROUTE", route)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    dK, dT = x.data_ptr(), x.data_ptr() + 8 * nk * B
    root = torch.zeros((B, R), dtype=torch.float64, device=cuda)
    f.handle.mc_eval_device(dK, 1, B, dT, 1, B, kF, beta, lam, root.data_ptr(), R, 1, B, st)
    torch.cuda.synchronize()
    exists = np.array([int(t.root_slot[k]) != 0xFFFFFFFF for k in range(R)])
    coef = random_coef(rng, 3, R)
    want = capi.observables_reference(root.cpu().numpy(), coef, jac.cpu().numpy(), rg, None, 1, 0, exists)
    wg, _keep2 = capi.make_weight_groups(rg, sets, B)
    T_rows = x[nk:].t().contiguous()
    for what, (pT, ts, tc) in (("component-major", (dT, 1, B)), ("sample-major", (T_rows.data_ptr(), n_tau, 1))):
        o = torch.zeros((1, 3), dtype=torch.float64, device=cuda)
        c = torch.zeros((1, 3, 3), dtype=torch.float64, device=cuda)
        ob, _keep3 = capi.make_observables(coef, o.data_ptr(), c.data_ptr())
        f.handle.mc_accumulate_device_observables(dK, 1, B, pT, ts, tc, kF, beta, lam, 0, 0, 1, jac.data_ptr(), ob, wg, B=B, stream=st)
        torch.cuda.synchronize()
        assert_obs((o.cpu().numpy(), c.cpu().numpy()), want, (route, what))


# ---- 6. known answer through the driver ------------------------------------------------------------------------------------------------------- #
def twin_roots():
    """Two roots that are the same function: both read one bosonic leaf of order 0, leaf(K) = 8 pi (|K|^2 + lambda).  Columns 0-2 are K,
    3 the one time."""
    a = fd.Graph([])
    r0, r1 = fd.Graph([a], subgraph_factors=[1.0]), fd.Graph([a], subgraph_factors=[1.0])
    t, _, _ = lower([r0, r1])
    assert t.n_leaf == 1 and t.n_root == 2
    assert list(oracle.eval_static(t, np.array([[2.5]]))[0]) == [2.5, 2.5]
    tab, keep = capi.make_leaf_tables([2], [0], [1], [1], [1], np.array([[1.0]]), 3, 1)
    return t, tab, keep


def test_sum_and_difference_of_equal_roots_known_answer(libfdg, cuda):
    """I = int over [-L, L]^3 of 8 pi (|K|^2 + lambda) = 64 pi L^3 (lambda + L^2), twice: the observables root 0 + root 1 and
    root 0 - root 1 are 2 I with an error of 2 sigma -- quadrature of the per-root errors would say sqrt(2) sigma -- and exactly 0 with
    an error of exactly 0 -- quadrature: sqrt(2) sigma."""
    L, lam, G, B, n_iter = 2.0, 0.05, 32, 50_000, 3
    exact = 64.0 * math.pi * L ** 3 * (lam + L * L)
    t, tab, _keep = twin_roots()
    f = fd.compile_table(t, specialize="isa")
    res = vegas.vegas_integrate(f, tab, [-L] * 3, [L] * 3, [0, 1, 2], 0.0, 1.0, lam, n_iter=n_iter, n_sample=B, n_grid=G, seed=2025, device=cuda,
                                observables=vegas.Observables(((1.0, 1.0), (1.0, -1.0))))
    print("twin roots:", res.mean, res.stderr, "observables:", res.obs_mean, res.obs_stderr, res.obs_chi2_dof, "exact", 2.0 * exact)
    print("obs_cov:", res.obs_cov)
    assert res.obs_mean.shape == (2,) and res.obs_cov.shape == (2, 2) and len(res.obs_iterations) == n_iter
    assert res.stderr[0] > 0 and res.stderr[0] == res.stderr[1] and abs(res.mean[0] - exact) < 5.0 * res.stderr[0]
    assert abs(res.obs_mean[0] - 2.0 * exact) < 5.0 * res.obs_stderr[0]
    assert res.obs_stderr[0] > 1.9 * res.stderr[0]
    assert math.isclose(res.obs_stderr[0], 2.0 * res.stderr[0], rel_tol=1e-12)
    assert res.obs_mean[1] == 0.0 and res.obs_stderr[1] == 0.0
    assert np.array_equal(res.obs_cov, res.obs_cov.T)
    assert np.allclose(np.diag(res.obs_cov), res.obs_stderr ** 2, rtol=1e-12, atol=0.0)
    # without the keyword the results are what they are today
    ref = vegas.vegas_integrate(f, tab, [-L] * 3, [L] * 3, [0, 1, 2], 0.0, 1.0, lam, n_iter=n_iter, n_sample=B, n_grid=G, seed=2025, device=cuda)
    assert ref.obs_mean is None and ref.obs_cov is None
    assert_bits(ref.mean, res.mean, "mean beside the observables")
    assert_bits(ref.stderr, res.stderr, "stderr beside the observables")
