"""Weight groups on the device (include/fdg.h: fdg_vegas_sample_device_grouped, fdg_accumulate_device_grouped,
fdg_mc_accumulate_device_grouped; vegas.WeightGroups, vegas.groups_from_dof): root k is weighted by the column of its group,
t = w[g(k)][b] root_k(b), and variable d is trained by v_d = the sum, over the groups that own d, of (w_g sum_k c_k r_k)^2.

Host references: the oracle's roots weighted in numpy; the cells of the training histograms from the Philox counters
(oracle.philox_uniform), as the pass recomputes them.  Tolerances, as in tests/test_moments_accumulate.py: |d| <= 1e-12 max(1, sum |t|)
per entry of a first moment, 1e-12 max(1, sum t^2) of a second moment; the training histograms are sums of non-negative terms and take
1e-12 max(1, their own value).  The sampler and the one-group ties are bit for bit."""
import functools
import math

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from test_matsubara_accumulate import assert_projection, host_projection, leaves, make_bins, random_table
from test_vegas_host import mirror_map

pytestmark = pytest.mark.gpu

TOL = 1e-12
B0, D0, G0 = 8_229, 7, 5
SETS = [(0, 1, 2), (0, 1, 2, 3, 4, 5), tuple(range(7))]          # three nested groups of variables; the last holds them all
SPECS = {"hip": True, "isa": "isa"}
FREQ, BETA, N_TAU = (0, -3, 5), 3.0, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = bits(a) == bits(b) if a.dtype == np.float64 else a == b
    assert same.all(), (what, np.argwhere(~same)[:4])


def leaf_strides(leaf):
    """(ss, ls, lts) of a [B, L] tensor of any strides or of a tile-major [tiles, L, 64] one"""
    return (leaf.stride(2), leaf.stride(1), leaf.stride(0)) if leaf.dim() == 3 else (leaf.stride(0), leaf.stride(1), 0)


def grouped_call(f, leaf, w, root_group, var_sets, B, cuda, bins=None, n_bin=1, bin_base=0, train=None, coef=None, mz=None, out=None,
                 train_bins=True):
    """One fdg_accumulate_device_grouped call.  w: [n_group, B] CUDA tensor; train: (seed, offset, D, G) or None; mz: (T tensor, freq,
    fermionic, tin, tout) or None; out: the dict of a previous call, added to.  Returns the dict of output tensors."""
    import torch
    R = f.n_root
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    if out is None:
        out = {"acc": z(n_bin, R), "acc2": z(n_bin, R)}
        if train:
            out["hist"] = z(train[2], train[3])
            if bins is not None and train_bins:
                out["hist_bin"] = z(n_bin)
        if mz:
            out["mz"] = z(4, n_bin, len(mz[1]), R)
    wg, _keep = capi.make_weight_groups(root_group, var_sets, w.stride(0))
    desc = None
    if mz:
        T, freq, fermionic, tin, tout = mz
        desc, _keep2 = capi.make_matsubara(freq, fermionic, tin, tout, BETA, T.shape[1], *[out["mz"][i].data_ptr() for i in range(4)],
                                           T.data_ptr(), T.stride(0), T.stride(1))
    seed, off, D, G = train or (0, 0, 0, 0)
    f.handle.accumulate_device_grouped(leaf.data_ptr(), *leaf_strides(leaf), 0 if bins is None else bins.data_ptr(), bin_base, n_bin,
                                       w.data_ptr(), wg, desc, coef, seed, off, D, G, out["acc"].data_ptr(), out["acc2"].data_ptr(),
                                       out["hist"].data_ptr() if train else 0, out["hist_bin"].data_ptr() if "hist_bin" in out else 0, B,
                                       torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    return out


# ---- 1. the sampler ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("discrete", [False, True])
@pytest.mark.parametrize("polar", [False, True])
def test_sampler_matches_the_numpy_mirror_bit_for_bit(libfdg, cuda, polar, discrete):
    import torch
    rng = np.random.default_rng(11)
    lo, hi = rng.uniform(-2.0, 0.0, D0), rng.uniform(0.5, 3.0, D0)
    if polar:
        lo[:3], hi[:3] = vegas.ball(2.5, 3, 0.25)
    edges = np.sort(rng.uniform(0.0, 1.0, (D0, G0 - 1)), axis=1)
    grid = lo[:, None] + (hi - lo)[:, None] * np.concatenate([np.zeros((D0, 1)), edges, np.ones((D0, 1))], axis=1)
    grid[:, -1] = hi
    assert (np.diff(grid, axis=1) > 0).all()
    groups = [(0, (0, 1, 2))] if polar else []
    col = [None, None, None, 3, 4, 5, 6] if polar else list(range(7))
    n_col, seed, off, NB = 9, 77, 12_345, 5
    cdf = np.array([0.0, 0.1, 0.35, 0.5, 0.9, 1.0])
    d_grid = torch.from_numpy(grid).to(cuda)
    d_cdf = torch.from_numpy(cdf).to(cuda)

    def run(grouped):
        x = torch.full((n_col, B0), -77.0, dtype=torch.float64, device=cuda)
        jac = torch.full((3, B0) if grouped else (B0,), -1.0, dtype=torch.float64, device=cuda)
        b = torch.full((B0,), -5, dtype=torch.int32, device=cuda)
        cell = torch.full((D0, B0), -5, dtype=torch.int32, device=cuda)
        head = (d_grid.data_ptr(), D0, G0, col, d_cdf.data_ptr() if discrete else 0, NB, 2, 0, None, groups)
        tail = (seed, off, x.data_ptr(), 1, B0, jac.data_ptr(), b.data_ptr() if discrete else 0, cell.data_ptr(), B0)
        if grouped:
            capi.vegas_sample_device_grouped(*head, SETS, B0, *tail)
        else:
            capi.vegas_sample_device_polar(*head, *tail)
        torch.cuda.synchronize(cuda)
        return x.cpu().numpy(), jac.cpu().numpy(), b.cpu().numpy(), cell.cpu().numpy()

    x0, j0, b0, c0 = run(False)
    x1, j1, b1, c1 = run(True)
    assert_bits(x1, x0, "x")
    assert_bits(b1, b0, "bin")
    assert_bits(c1, c0, "cell")
    assert_bits(j1[2], j0, "the full mask is the polar sampler's jacobian")
    v, _, cell = mirror_map(grid, oracle.philox_uniform(B0, D0, seed, off))
    assert np.array_equal(cell, c1.T)
    factor = np.float64(G0) * (grid[np.arange(D0)[None, :], cell + 1] - grid[np.arange(D0)[None, :], cell])
    prob = (cdf[b1 - 2 + 1] - cdf[b1 - 2]) if discrete else None
    want = capi.grouped_jacobian(factor, SETS, groups, v, prob)
    assert_bits(j1, want, "jacobians against the numpy mirror")
    assert not np.array_equal(j1[0], j1[1]) and not np.array_equal(j1[1], j1[2])
    if polar:
        with pytest.raises(capi.FdgError) as e:              # a mask that splits the polar group
            capi.vegas_sample_device_grouped(d_grid.data_ptr(), D0, G0, col, 0, NB, 2, 0, None, groups, [(0, 1), tuple(range(7))], B0, seed, off,
                                             0x1000, 1, B0, 0x2000, 0, 0, B0)
        assert e.value.code == capi.FDG_E_INVALID


# ---- the shared inputs: computed once, never written to ---------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def batch(name):
    t = workloads.get(name)
    h_leaf = oracle.philox_uniform(B0, t.n_leaf, 31)
    rng = np.random.default_rng(7)
    T = rng.uniform(0.0, BETA, size=(B0, N_TAU))
    T[:, 0] = 0.0
    w = rng.uniform(0.1, 2.0, size=(3, B0))
    bins = make_bins(rng, B0, 7, base=1)
    tin, tout = workloads.root_times(name)
    return t, h_leaf, oracle.eval_static(t, h_leaf), T, w, bins, tin, tout


def cells_of(B, D, G, seed, off):
    return np.minimum((oracle.philox_uniform(B, D, seed, off) * np.float64(G)).astype(np.int64), G - 1)


# ---- 2. one group, a full mask: the bits of the calls it generalises ------------------------------------------------------------------------ #
@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("name", ["sigma2", "parquet_sigma4"])
def test_one_group_is_the_ungrouped_call_bit_for_bit(libfdg, cuda, name, spec):
    import torch
    t, h_leaf, _, h_T, h_w, h_bins, tin, tout = batch(name)
    f = fd.compile_table(t, specialize=SPECS[spec])
    R = t.n_root
    w = torch.from_numpy(h_w[:1].copy()).to(cuda)
    d_T, bins = torch.from_numpy(h_T).to(cuda), torch.from_numpy(h_bins).to(cuda)
    coef = list(np.random.default_rng(3).uniform(0.5, 1.5, R))
    seed, off = 5, 1_000
    one = dict(root_group=[0] * R, var_sets=[tuple(range(D0))], B=B0, cuda=cuda)
    for layout in ["leaf_major"] + (["tiled"] if spec == "isa" else ["row"]):
        leaf = leaves(cuda, h_leaf, layout)
        a, a2 = f.accumulate_moments(leaf, weight=w[0], n_sample=B0)
        got = grouped_call(f, leaf, w, **one)
        assert_bits(got["acc"].cpu().numpy(), a.cpu().numpy(), (layout, "moments acc"))
        assert_bits(got["acc2"].cpu().numpy(), a2.cpu().numpy(), (layout, "moments acc2"))
        a, a2, h = f.accumulate_vegas(leaf, w[0], None, seed, off, D0, G0, coef=coef, n_sample=B0)
        got = grouped_call(f, leaf, w, train=(seed, off, D0, G0), coef=coef, **one)
        for key, ref in (("acc", a), ("acc2", a2), ("hist", h)):
            assert_bits(got[key].cpu().numpy(), ref.cpu().numpy(), (layout, "vegas", key))
        a, a2, h, hb = f.accumulate_vegas_binned(leaf, bins, 7, w[0], None, None, seed, off, D0, G0, coef=coef, bin_base=1, n_sample=B0)
        got = grouped_call(f, leaf, w, bins=bins, n_bin=7, bin_base=1, train=(seed, off, D0, G0), coef=coef, **one)
        for key, ref in (("acc", a), ("acc2", a2), ("hist", h), ("hist_bin", hb)):
            assert_bits(got[key].cpu().numpy(), ref.cpu().numpy(), (layout, "vegas_binned", key))
        sums = torch.zeros((4, 7, len(FREQ), R), dtype=torch.float64, device=cuda)
        f.accumulate_matsubara(leaf, d_T, FREQ, tin, tout, BETA, True, bins, 7, w[0], sums=sums, bin_base=1, n_sample=B0)
        got = grouped_call(f, leaf, w, bins=bins, n_bin=7, bin_base=1, mz=(d_T, FREQ, True, tin, tout), **one)
        assert_bits(got["mz"].cpu().numpy(), sums.cpu().numpy(), (layout, "matsubara"))
        a, a2 = f.accumulate_moments(leaf, bins, 7, weight=w[0], bin_base=1, n_sample=B0)
        assert_bits(got["acc"].cpu().numpy(), a.cpu().numpy(), (layout, "matsubara: moments beside it"))


# ---- the host reference of a grouped call ------------------------------------------------------------------------------------------------- #
def host_grouped(roots, w, root_group, var_sets, live, bins=None, n_bin=1, base=0, train=None, coef=None, n=None):
    """dict of acc, acc2, scale, scale2 [n_bin, R] and, with train = (seed, off, D, G), hist [D, G] (nan where no group with a root owns
    the variable) and hist_bin [n_bin]; the samples b < n whose bin is in range."""
    B, R = roots.shape
    n = B if n is None else n
    j = np.zeros(B, dtype=np.int64) if bins is None else bins.astype(np.int64) - base
    ok = (j >= 0) & (j < n_bin) & (np.arange(B) < n)
    out = {key: np.zeros((n_bin, R)) for key in ("acc", "acc2", "scale")}
    for k in live:
        t = w[root_group[k], ok] * roots[ok, k]
        for key, v in (("acc", t), ("acc2", t * t), ("scale", np.abs(t))):
            out[key][:, k] = np.bincount(j[ok], weights=v, minlength=n_bin)
    if train:
        seed, off, D, G = train
        cell = cells_of(B, D, G, seed, off)[ok]
        q = {}
        for g in sorted({root_group[k] for k in live}):
            s = sum((1.0 if coef is None else coef[k]) * roots[ok, k] for k in live if root_group[k] == g)
            q[g] = (w[g, ok] * s) ** 2
        out["hist"] = np.full((D, G), np.nan)
        for d in range(D):
            owners = [g for g in q if d in var_sets[g]]
            if owners:
                out["hist"][d] = np.bincount(cell[:, d], weights=sum(q[g] for g in owners), minlength=G)
        out["hist_bin"] = np.bincount(j[ok], weights=sum(q.values()), minlength=n_bin)
    return out


def assert_grouped(got, want, what, sentinel=None):
    a, a2 = got["acc"].cpu().numpy(), got["acc2"].cpu().numpy()
    bad = np.abs(a - want["acc"]) > TOL * np.maximum(1.0, want["scale"])
    assert not bad.any(), (what, "acc", np.argwhere(bad)[:4])
    bad = np.abs(a2 - want["acc2"]) > TOL * np.maximum(1.0, want["acc2"])
    assert not bad.any(), (what, "acc2", np.argwhere(bad)[:4])
    for key in ("hist", "hist_bin"):
        if key in got:
            h, ref = got[key].cpu().numpy(), want[key]
            dead = np.isnan(ref)
            assert (h[dead] == sentinel).all(), (what, key, "a variable of no group was written")
            bad = np.abs(h[~dead] - ref[~dead]) > TOL * np.maximum(1.0, ref[~dead])
            assert not bad.any(), (what, key, np.abs(h[~dead] - ref[~dead]).max())


# ---- 3. several groups against numpy -------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("spec", list(SPECS))
def test_several_groups_match_numpy(libfdg, cuda, spec):
    import torch
    t, h_leaf, roots, h_T, h_w, h_bins, tin, tout = batch("parquet_sigma4")
    assert t.n_root == 4
    f = fd.compile_table(t, specialize=SPECS[spec])
    rg, live = [0, 1, 1, 2], range(4)
    w = torch.from_numpy(h_w).to(cuda)
    bins, d_T = torch.from_numpy(h_bins).to(cuda), torch.from_numpy(h_T).to(cuda)
    leaf = leaves(cuda, h_leaf, "tiled" if spec == "isa" else "leaf_major")
    coef = [0.5, -1.25, 2.0, 1.0]
    train = (9, 4_000, D0, G0)
    got = grouped_call(f, leaf, w, rg, SETS, B0, cuda)
    assert_grouped(got, host_grouped(roots, h_w, rg, SETS, live), "moments")
    got = grouped_call(f, leaf, w, rg, SETS, B0, cuda, train=train, coef=coef)
    assert_grouped(got, host_grouped(roots, h_w, rg, SETS, live, train=train, coef=coef), "vegas")
    got = grouped_call(f, leaf, w, rg, SETS, B0, cuda, bins=bins, n_bin=7, bin_base=1, train=train)
    assert_grouped(got, host_grouped(roots, h_w, rg, SETS, live, h_bins, 7, 1, train=train), "vegas_binned")
    # variable 6 in no group's mask: its histogram keeps what was there
    sets = [SETS[0], SETS[1], (3, 4)]
    out = {"acc": torch.zeros((1, 4), dtype=torch.float64, device=cuda), "acc2": torch.zeros((1, 4), dtype=torch.float64, device=cuda),
           "hist": torch.zeros((D0, G0), dtype=torch.float64, device=cuda)}
    out["hist"][6] = -123.0
    got = grouped_call(f, leaf, w, rg, sets, B0, cuda, train=train, coef=coef, out=out)
    want = host_grouped(roots, h_w, rg, sets, live, train=train, coef=coef)
    assert np.isnan(want["hist"][6]).all() and not np.isnan(want["hist"][:6]).any()
    assert_grouped(got, want, "a variable of no group", sentinel=-123.0)
    # one group, a mask that leaves variables out: the moments are the ungrouped call's bits, the training skips the others
    got = grouped_call(f, leaf, w[:1], [0] * 4, [(1, 4)], B0, cuda, train=train)
    a, a2 = f.accumulate_moments(leaf, weight=w[0], n_sample=B0)
    assert_bits(got["acc"].cpu().numpy(), a.cpu().numpy(), "one group, part of the variables")
    want = host_grouped(roots, h_w, [0] * 4, [(1, 4)], live, train=train)
    assert_grouped(got, want, "one group, part of the variables", sentinel=0.0)
    # the projection: each of the four sums, the roots of every group projected with the group's weight
    got = grouped_call(f, leaf, w, rg, SETS, B0, cuda, bins=bins, n_bin=7, bin_base=1, mz=(d_T, FREQ, False, tin, tout))
    want = sum(host_projection(roots, h_T, tin, tout, FREQ, BETA, False, h_bins, 7, h_w[g], base=1, live=[k for k in live if rg[k] == g])
               for g in range(3))
    assert_projection(got["mz"].cpu().numpy(), want, "projection with groups")
    assert_grouped(got, host_grouped(roots, h_w, rg, SETS, live, h_bins, 7, 1), "moments beside the projection")


# ---- 4. many roots, small chunks ---------------------------------------------------------------------------------------------------------- #
def test_chunks_root_slices_poisoned_samples_shards_and_repeats(libfdg, cuda):
    """FDG_ROOT_SCRATCH_MB = 1 with 19 roots: chunks of 6 848 samples, eleven of them; two slices of 16 roots, each with roots of all four
    groups (dealt round robin); inf and nan weights and leaves on samples whose bin is out of range reach no sum.  Root 7 does not exist."""
    import torch
    rng = np.random.default_rng(5)
    t = random_table(rng)
    R, B, n_bin, missing = t.n_root, 70_003, 3, 7
    live = [k for k in range(R) if k != missing]
    rg = [k % 4 for k in range(R)]
    sets = [(0, 1), (1, 2, 3), (0, 4), (2, 5)]                              # variable 6 belongs to no group
    f = fd.compile_table(t, specialize="isa", options={"FDG_ROOT_SCRATCH_MB": "1"})
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 17) + 0.25
    h_bins = make_bins(rng, B, n_bin, base=0)
    h_w = rng.uniform(0.1, 2.0, size=(4, B))
    out_of_range = np.flatnonzero((h_bins < 0) | (h_bins >= n_bin))
    assert out_of_range.size > 500
    h_leaf[out_of_range[0::3], 0], h_leaf[out_of_range[1::3], 1] = np.inf, np.nan
    h_w[1, out_of_range[2::3]], h_w[2, out_of_range[0::2]] = np.nan, np.inf
    roots = oracle.eval_static(t, h_leaf)
    leaf, w, bins = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins).to(cuda)
    train = (21, 500, D0, G0)
    with np.errstate(invalid="ignore", over="ignore"):
        want = host_grouped(roots, h_w, rg, sets, live, h_bins, n_bin, 0, train=train)

    def fresh():
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=cuda)
        o = {"acc": z(n_bin, R), "acc2": z(n_bin, R), "hist": z(D0, G0), "hist_bin": z(n_bin)}
        o["acc"][:, missing], o["acc2"][:, missing], o["hist"][6] = -7.0, -7.0, -9.0
        return o

    call = lambda o, lf=leaf, ww=w, bb=bins, n=B, off=train[1]: grouped_call(f, lf, ww, rg, sets, n, cuda, bins=bb, n_bin=n_bin,
                                                                             train=(train[0], off, D0, G0), out=o)
    a = call(fresh())
    host = {k: v.cpu().numpy().copy() for k, v in a.items()}
    assert (host["acc"][:, missing] == -7.0).all() and (host["acc2"][:, missing] == -7.0).all()
    for key in ("acc", "acc2"):
        a[key][:, missing] = 0.0
    assert_grouped(a, want, "19 roots, 4 groups", sentinel=-9.0)
    b = call(fresh())
    for key in host:
        assert_bits(b[key].cpu().numpy(), host[key], ("the same arguments, the same bits", key))
    b = call(b)                                                               # a second call adds on top
    for key in ("acc", "hist_bin"):
        now, once = b[key].cpu().numpy(), host[key]
        keep = np.ones_like(once, dtype=bool)
        if key == "acc":
            keep[:, missing] = False
        assert np.allclose(now[keep], 2.0 * once[keep], rtol=1e-12, atol=0.0), key
    # two shards reproduce the whole (the cut on a chunk boundary of neither)
    cut = 64 * 517
    o = fresh()
    lf2 = leaves(cuda, h_leaf[cut:], "tiled")
    call(o, n=cut)
    grouped_call(f, lf2, w[:, cut:], rg, sets, B - cut, cuda, bins=bins[cut:], n_bin=n_bin, train=(train[0], train[1] + cut, D0, G0), out=o)
    for key in ("acc", "acc2"):
        o[key][:, missing] = 0.0
    assert_grouped(o, want, "two shards", sentinel=-9.0)
    # a group whose only root does not exist contributes nothing: its variable 6 stays untouched, the others are what they were
    rg5 = [4 if k == missing else k % 4 for k in range(R)]
    c = grouped_call(f, leaf, torch.cat([w, w[:1]]).contiguous(), rg5, sets + [(6,)], B, cuda, bins=bins, n_bin=n_bin, train=train, out=fresh())
    for key in ("acc", "acc2"):
        c[key][:, missing] = 0.0
    assert_grouped(c, want, "a group without a root", sentinel=-9.0)


# ---- 5. the Monte-Carlo routes ------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("route", ["split", "fused", None])
def test_mc_routes(libfdg, cuda, fdgopt, route):
    """fdg_mc_accumulate_device_grouped on every route, T component-major and sample-major, against the same handle's mc_eval_device
    roots weighted in numpy (the pattern of tests/test_vegas_accumulate.py::test_mc_vegas_routes); the weights are the grouped sampler's."""
    import os
    import torch
    z = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    R = t.n_root
    B, dim, n_loop, n_tau = 20_011, 3, int(z["basis"].shape[1]), int(z["n_tau"])
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
    live = [k for k in range(R) if int(t.root_slot[k]) != 0xFFFFFFFF]
    coef = list(rng.uniform(-1.0, 1.0, size=R))
    train = (seed, off, D, G)
    want = host_grouped(root.cpu().numpy(), jac.cpu().numpy(), rg, sets, live, train=train, coef=coef)
    wg, _keep2 = capi.make_weight_groups(rg, sets, B)
    T_rows = x[nk:].t().contiguous()                                          # [B, n_tau]: sample-major
    for what, (pT, ts, tc) in (("component-major", (dT, 1, B)), ("sample-major", (T_rows.data_ptr(), n_tau, 1))):
        got = {"acc": torch.zeros((1, R), dtype=torch.float64, device=cuda), "acc2": torch.zeros((1, R), dtype=torch.float64, device=cuda),
               "hist": torch.zeros((D, G), dtype=torch.float64, device=cuda)}
        f.handle.mc_accumulate_device_grouped(dK, 1, B, pT, ts, tc, kF, beta, lam, 0, 0, 1, jac.data_ptr(), wg, None, coef, seed, off, D, G,
                                              got["acc"].data_ptr(), got["acc2"].data_ptr(), got["hist"].data_ptr(), 0, B, st)
        torch.cuda.synchronize()
        assert_grouped(got, want, (route, what), sentinel=0.0)


# ---- 6. known answer through the driver ----------------------------------------------------------------------------------------------------- #
def two_orders():
    """Two roots over two bosonic leaves of order 0, leaf(K) = 8 pi (|K|^2 + lambda): root 0 = leaf(K_1), root 1 = leaf(K_1) leaf(K_2).
    Columns 0-2 are K_1, 3-5 K_2, 6 the one time."""
    a, b = fd.Graph([]), fd.Graph([])
    r0, r1 = fd.Graph([a], subgraph_factors=[1.0]), fd.Graph([a, b], operator=fd.Prod())
    t, _, _ = lower([r0, r1])
    assert t.n_leaf == 2 and t.n_root == 2
    probe = oracle.eval_static(t, np.array([[2.0, 3.0]]))[0]
    assert probe[1] == 6.0 and probe[0] in (2.0, 3.0)
    first = 0 if probe[0] == 2.0 else 1                                       # the leaf root 0 reads: it sits on K_1
    loop = [1, 2] if first == 0 else [2, 1]
    tab, keep = capi.make_leaf_tables([2, 2], [0, 0], [1, 1], [1, 1], loop, np.array([[1.0, 0.0], [0.0, 1.0]]), 3, 1)
    return t, tab, keep


def test_two_orders_in_one_run_known_answer(libfdg, cuda):
    """I = int over [-L, L]^3 of 8 pi (|K|^2 + lambda) = 64 pi L^3 (lambda + L^2); root 0 integrates K_1 only (dof 1), root 1 both (dof 2):
    the exact values are I and I^2.  Without groups root 0 is integrated over K_2 as well: 64 I, with the variance of three variables it
    does not depend on -- here only of the map's jacobian over them, which is why its error, divided by 64, must lie above the grouped
    run's.  The last three variables are trained by root 1 alone and must stay a valid map.  Statistics, not bits."""
    L, lam, G, B, n_iter = 2.0, 0.05, 64, 200_000, 4
    exact = 64.0 * math.pi * L ** 3 * (lam + L * L)
    t, tab, _keep = two_orders()
    f = fd.compile_table(t, specialize="isa")
    pools = [[[0, 1, 2], [3, 4, 5]]]
    groups = vegas.groups_from_dof([[1], [2]], pools)
    assert groups.root_group == (0, 1) and groups.var_sets == ((0, 1, 2), (0, 1, 2, 3, 4, 5))
    args = dict(n_iter=n_iter, n_sample=B, n_grid=G, seed=2025, device=cuda)
    res = vegas.vegas_integrate(f, tab, [-L] * 6, [L] * 6, list(range(6)), 0.0, 1.0, lam, groups=groups, **args)
    ref = vegas.vegas_integrate(f, tab, [-L] * 6, [L] * 6, list(range(6)), 0.0, 1.0, lam, **args)
    print("two orders, grouped:", res.mean, res.stderr, res.chi2_dof, "exact", exact, exact ** 2, (res.mean - [exact, exact ** 2]) / res.stderr)
    print("two orders, one weight:", ref.mean, ref.stderr, "root 0 / 64:", ref.mean[0] / 64.0, ref.stderr[0] / 64.0)
    assert res.mean.shape == (2,) and (res.stderr > 0).all()
    assert abs(res.mean[0] - exact) < 5.0 * res.stderr[0]
    assert abs(res.mean[1] - exact ** 2) < 5.0 * res.stderr[1]
    assert abs(ref.mean[0] - 64.0 * exact) < 5.0 * ref.stderr[0]
    assert res.stderr[0] < ref.stderr[0] / 64.0
    g = res.map.grid
    assert g.shape == (6, G + 1) and (np.diff(g[3:], axis=1) > 0).all()
    assert not np.array_equal(g[3:], vegas.uniform_grid([-L] * 3, [L] * 3, G))  # ... and they were trained
