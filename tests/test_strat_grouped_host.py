"""Stratified sampling for spherical momenta and weight groups, without a device (include/fdg.h: fdg_vegas_sample_device_strat_grouped,
fdg_accumulate_device_strat_grouped, fdg_mc_accumulate_device_strat_grouped, fdg_strat_allocate_cols; feynmandiagram.jl_amd/vegas.py:
vegas_integrate_stratified): the symbols are declared, exported and bound, every argument check runs before any device work, the
host-only allocator follows the steps the header states, and the numpy mirror of the driver (what tests/test_strat_grouped_accumulate.py
compares the device with) meets on the CPU the conditions that file asserts on the GPU."""
import math
import re

import numpy as np
import pytest

import oracle
from feynmandiagram_jl_amd import capi, vegas, workloads
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_strat_host import FAKE, FAKE2, FAKE3, FAKE4, FAKE5, FAKE6, HMAX, failed, u32
from test_vegas_host import JL

NAMES = ("fdg_vegas_sample_device_strat_grouped", "fdg_accumulate_device_strat_grouped", "fdg_mc_accumulate_device_strat_grouped",
         "fdg_strat_allocate_cols")
FAKE7 = 0x70000


# ---- the known answers ---------------------------------------------------------------------------------------------------------------- #
def peak(s, a):
    """f(X, Y) = 1 / ((X - s)^2 + Y^2 + a^2) and its integral over the unit disc: the angle first (2 pi / sqrt(Q(r^2)),
    Q(u) = u^2 + 2 u (a^2 - s^2) + (s^2 + a^2)^2), then u = r^2"""
    q = lambda u: u * u + 2.0 * u * (a * a - s * s) + (s * s + a * a) ** 2
    prim = lambda u: math.log(2.0 * math.sqrt(q(u)) + 2.0 * u + 2.0 * (a * a - s * s))
    return (lambda x, y: 1.0 / ((x - s) ** 2 + y * y + a * a)), math.pi * (prim(1.0) - prim(0.0))


# test 8 / 10 of the GPU file: one dim-2 polar group on the unit disc;  test 9: two of them, two roots in two weight groups
PEAK = dict(s=0.6, a=0.05)
KNOWN_POLAR = dict(S=(16, 16), n_sample=200_000, n_iter=5, n_grid=64, seed=2025)
KNOWN_GROUPS = dict(S=(6, 6, 6, 6), n_sample=200_000, n_iter=5, n_grid=64, seed=2026)
CALIB_POLAR = dict(S=(16, 16), n_sample=20_000, n_grid=64, n_seed=32)
DISC_LO, DISC_HI = vegas.ball(1.0, 2)


def polar_case():
    """(roots(x), lo, hi, col, polar, var_sets, root_group, n_col, exact) of test 8: columns 0, 1 = X, Y"""
    f, exact = peak(**PEAK)
    return (lambda x: np.stack([f(x[:, 0], x[:, 1])], axis=1)), DISC_LO, DISC_HI, [None, None], [(0, (0, 1))], None, None, 2, np.array([exact])


def groups_case():
    """... of test 9: columns 0 .. 3 = K1x, K1y, K2x, K2y; root 0 = f(K1) in group 0 (K1's variables), root 1 = f(K1) f(K2) in group 1"""
    f, exact = peak(**PEAK)
    roots = lambda x: np.stack([f(x[:, 0], x[:, 1]), f(x[:, 0], x[:, 1]) * f(x[:, 2], x[:, 3])], axis=1)
    return (roots, DISC_LO * 2, DISC_HI * 2, [None] * 4, [(0, (0, 1)), (2, (2, 3))], ((0, 1), (0, 1, 2, 3)), (0, 1), 4,
            np.array([exact, exact * exact]))


def mirror_stratified(roots_of, lo, hi, col, polar, var_sets, root_group, n_col, strat, n_grid, n_sample, n_iter, seed, alpha=0.5, beta=0.75,
                      alloc_cols=None):
    """vegas.vegas_integrate_stratified on the CPU: the iterations [(mean [R], stderr [R])] and the counts per hypercube.  The samples are
    the device's bit for bit (oracle.philox_uniform, capi.strat_grouped_reference); the sums are numpy's."""
    grid = vegas.uniform_grid(lo, hi, n_grid)
    D, N, H = grid.shape[0], int(n_sample), int(np.prod(strat))
    its, counts = [], []
    start = None
    for it in range(n_iter):
        if start is None:
            start = capi.strat_allocate_cols_reference(None, None, [0], None, H, N, beta)
        u = oracle.philox_uniform(N, D, vegas._iteration_seed(seed, it), 0)
        r = capi.strat_grouped_reference(grid, strat, start, u, col, polar, var_sets, n_col)
        roots = roots_of(r["x"])
        R = roots.shape[1]
        rg = np.zeros(R, dtype=np.int64) if root_group is None else np.asarray(root_group)
        w = r["jac"].reshape(-1, N)
        full = capi.strat_grouped_reference(grid, strat, start, u, col, polar, var_sets, n_col, roots=roots, weight=w, root_group=rg)
        cs, cs2 = full["cube_sum"], full["cube_sum2"]
        NG = w.shape[0]
        mean = np.array([(w[rg[k]] * roots[:, k]).sum() / N for k in range(R)])
        its.append((mean, np.sqrt(vegas.strat_variance(cs[:, :R], cs2[:, :R], np.diff(start), N))))
        counts.append(np.diff(start))
        # the grouped training rule: q_g = (w_g s_g)^2, a variable's fold over its owning groups
        q = [(w[g] * roots[:, rg == g].sum(axis=1)) ** 2 for g in range(NG)]
        sets = [range(D)] if var_sets is None else var_sets
        hist = np.zeros((D, n_grid))
        for d in range(D):
            v = sum(q[g] for g in range(NG) if d in sets[g])
            hist[d] = np.bincount(r["cell"][:, d], weights=v, minlength=n_grid)
        capi.vegas_refine(grid, hist, alpha)
        cols = [R + g for g in range(NG)] if alloc_cols is None else alloc_cols
        start = capi.strat_allocate_cols_reference(cs, cs2, cols, start, H, N, beta)
    return its, counts


def mirror_known(case, k, n_iter=None, seed=None):
    roots_of, lo, hi, col, polar, var_sets, root_group, n_col, exact = case
    its, counts = mirror_stratified(roots_of, lo, hi, col, polar, var_sets, root_group, n_col, k["S"], k["n_grid"], k["n_sample"],
                                    k.get("n_iter", 1) if n_iter is None else n_iter, k.get("seed", 0) if seed is None else seed)
    return its, counts, exact


def test_mirror_meets_the_conditions_of_the_gpu_tests(libfdg):
    """Conditions, not measurements: the GPU file asserts that the combined estimates lie within 5 sigma of the exact integrals and that
    the calibration sum lies in [12, 60]; the mirror must meet the same on the CPU, or the parameters above are the wrong ones."""
    its, counts, exact = mirror_known(polar_case(), KNOWN_POLAR)
    m, e, _ = vegas.combine(its)
    print("polar", m, e, "exact", exact, "pull", (m - exact) / e)
    assert (np.abs(m - exact) < 5.0 * e).all() and (e > 0).all()
    assert all(c.sum() == KNOWN_POLAR["n_sample"] and c.min() >= 2 for c in counts)
    its, counts, exact = mirror_known(groups_case(), KNOWN_GROUPS)
    m, e, _ = vegas.combine(its)
    print("groups", m, e, "exact", exact, "pull", (m - exact) / e)
    assert (np.abs(m - exact) < 5.0 * e).all() and (e > 0).all()
    assert all(c.sum() == KNOWN_GROUPS["n_sample"] and c.min() >= 2 for c in counts)
    chi2 = 0.0
    for seed in range(CALIB_POLAR["n_seed"]):
        ((m, e),), _, exact = mirror_known(polar_case(), CALIB_POLAR, 1, seed)
        chi2 += ((m[0] - exact[0]) / e[0]) ** 2
    print("calibration chi2 over", CALIB_POLAR["n_seed"], "seeds:", chi2)
    assert 12.0 <= chi2 <= 60.0


def test_a_group_without_fac_h_would_be_biased(libfdg):
    """why every group takes fac_h: with an allocation that favours the hypercubes at small k1, the area of K1's disc -- the constant 1
    under group 0's weights, which own K1's variables only -- comes out as pi with fac_h and far from it with the weights divided by
    fac_h again"""
    roots_of, lo, hi, col, polar, var_sets, root_group, n_col, exact = groups_case()
    k = KNOWN_GROUPS
    grid = vegas.uniform_grid(lo, hi, k["n_grid"])
    H = int(np.prod(k["S"]))
    counts = np.where(np.arange(H) % k["S"][0] == 0, 100, 4)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    N = int(start[-1])
    r = capi.strat_grouped_reference(grid, k["S"], start, oracle.philox_uniform(N, 4, 9, 0), col, polar, var_sets, n_col)
    fac = np.float64(N) / (np.float64(H) * counts[r["cube"]])
    good, bad = r["jac"][0], r["jac"][0] / fac
    err = lambda t: t.std() / math.sqrt(N)
    print("area with fac_h", good.mean(), "+-", err(good), "without", bad.mean(), "+-", err(bad), "exact", math.pi)
    assert abs(good.mean() - math.pi) < 5.0 * err(good) and abs(bad.mean() - math.pi) > 10.0 * err(bad)


# ---- declared, exported, bound ------------------------------------------------------------------------------------------------------ #
def test_symbols_are_declared_exported_and_bound(libfdg):
    protos = c_prototypes()
    calls = {c[0]: c for c in jl_ccalls()}
    export = [x.strip() for x in re.search(r"^export\s+([^\n]*)", open(JL).read(), flags=re.M).group(1).split(",")]
    for name in NAMES:
        assert name in protos and name in capi.EXPORTS and hasattr(libfdg, name), name
        assert name in calls, name + ": not bound in the Julia shim"
        _, _, types, args = calls[name]
        params = protos[name][1]
        assert len(types) == len(params) == len(args) == len(getattr(libfdg, name).argtypes), name
        for jt, cp in zip(types, params):
            assert jl_class(jt) == c_class(cp), (name, jt, cp)
    for fn in ("vegas_sample_device_strat_grouped!", "accumulate_device_strat_grouped!", "mc_accumulate_device_strat_grouped!",
               "strat_allocate_cols!"):
        assert fn in export, fn
    import feynmandiagram_jl_amd as fd
    assert fd.vegas_integrate_stratified is vegas.vegas_integrate_stratified and "vegas_integrate_stratified" in fd.__all__


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def _polar(groups):
    """the fdg_vegas_polar array of (var, cols) pairs, unchecked: the library's own checks are under test"""
    arr = (capi.VegasPolar * max(len(groups), 1))()
    for g, (var, cols) in enumerate(groups):
        arr[g].var, arr[g].dim = var, len(cols)
        for i, v in enumerate(cols[:3]):
            arr[g].col[i] = v
    return arr, len(groups)


def _sample(strat=(2, 2, 1, 1, 1), n_dim=5, n_grid=8, d_grid=FAKE, d_x=FAKE2, d_jac=FAKE3, d_start=FAKE4, d_cube=FAKE5, B=100,
            polar=((0, (0, 1, 2)),), null_polar=False, n_polar=None, masks=((0, 1, 2, 3, 4), (0, 1, 2)), null_masks=False, n_group=None,
            jstride=100, col=(0, 0, 0, 3, 4)):
    sv = None if strat is None else u32(strat)
    arr, n = _polar(polar)
    vm = capi.var_masks(masks) if not (len(masks) and isinstance(masks[0], (int, np.integer))) else np.array(masks, dtype=np.uint64)
    c = u32(col)
    return capi.lib().fdg_vegas_sample_device_strat_grouped(
        d_grid, n_dim, n_grid, c.ctypes.data, None if (null_polar or n == 0) else capi.C.addressof(arr), n if n_polar is None else n_polar,
        None if (null_masks or vm.shape[0] == 0) else vm.ctypes.data, vm.shape[0] if n_group is None else n_group, jstride,
        None if sv is None else sv.ctypes.data, d_start, 1, 0, d_x, 1, 100, d_jac, d_cube, None, B, None)


def test_sampler_argument_checks_need_no_device(libfdg):
    # the stratified sampler's cases
    for kw in (dict(strat=None), dict(d_start=None), dict(d_cube=None), dict(strat=(2, 0, 1, 1, 1)), dict(d_grid=None), dict(d_x=None),
               dict(d_jac=None), dict(B=-1), dict(n_grid=0), dict(n_dim=0, strat=(), polar=(), masks=((),), col=())):
        assert failed(_sample(**kw), capi.FDG_E_INVALID), kw
    assert failed(_sample(strat=(1024, 1024, 2, 1, 1)), capi.FDG_E_UNSUPPORTED)
    assert failed(_sample(strat=(65536, 65536, 65536, 1, 1)), capi.FDG_E_UNSUPPORTED)
    assert failed(_sample(n_grid=capi.FDG_VEGAS_GRID_MAX + 1), capi.FDG_E_UNSUPPORTED)
    # the grouped sampler's cases
    for kw in (dict(null_masks=True), dict(n_group=0), dict(masks=((0, 1, 2, 3, 4), (5,))), dict(masks=((0, 1, 2, 3, 4), (0, 1))),
               dict(masks=((0, 1, 2, 3, 4), (1, 2, 3))), dict(jstride=99), dict(null_polar=True), dict(polar=((0, (0,)),)),
               dict(polar=((3, (0, 1, 2)),)), dict(polar=((0, (0, 1, 2)), (2, (5, 6)))), dict(polar=((0, (0, 1, 3)),)),
               dict(polar=((0, (0, 1, 4)),))):
        assert failed(_sample(**kw), capi.FDG_E_INVALID), kw
    assert failed(_sample(n_group=capi.FDG_WEIGHT_GROUP_MAX + 1), capi.FDG_E_UNSUPPORTED)
    assert failed(_sample(n_polar=capi.FDG_VEGAS_POLAR_MAX + 1), capi.FDG_E_UNSUPPORTED)
    # valid and nothing to do: no device work; without groups (var_mask NULL and n_group 0) one jacobian
    assert _sample(B=0) == capi.FDG_OK
    assert _sample(B=0, masks=()) == capi.FDG_OK
    assert _sample(B=0, masks=(), polar=(), col=(0, 1, 2, 3, 4)) == capi.FDG_OK
    assert _sample(B=0, strat=(1024, 1024, 1, 1, 1)) == capi.FDG_OK
    assert _sample(B=0, masks=((0, 1, 2, 3, 4),), jstride=0) == capi.FDG_OK           # one group: the stride is not read
    with pytest.raises(ValueError):
        capi.vegas_sample_device_strat_grouped(FAKE, 3, 8, None, (), None, 0, (2, 2), FAKE4, 1, 0, FAKE2, 1, 100, FAKE3, FAKE5, 0, 100)
    with pytest.raises(capi.FdgError) as e:
        capi.vegas_sample_device_strat_grouped(FAKE, 3, 8, None, (), ((0, 1, 2), (0,)), 100, (2, 2, 0), FAKE4, 1, 0, FAKE2, 1, 100, FAKE3,
                                               FAKE5, 0, 100)
    assert e.value.code == capi.FDG_E_INVALID


def _groups(n_root, root_group=None, masks=((0, 1, 2), (0, 1)), stride=100, null=None, n_group=None):
    rg = u32(np.arange(n_root) % len(masks) if root_group is None else root_group)
    vm = capi.var_masks(masks)
    wg = capi.WeightGroups(len(masks) if n_group is None else n_group, None if null == "root_group" else rg.ctypes.data,
                           None if null == "var_mask" else vm.ctypes.data, stride)
    return wg, (rg, vm)


def _acc(h, mc=False, strat=(2, 2, 1), n_dim=3, n_grid=8, B=100, d_in=FAKE, d_w=FAKE7, d_acc=FAKE, d_acc2=FAKE2, d_hist=FAKE3, d_cube=FAKE4,
         d_sum=FAKE5, d_sum2=FAKE6, wg="default", **gkw):
    sv = None if strat is None else u32(strat)
    keep = None
    if wg == "default":
        wg, keep = _groups(h.table.n_root if h else 1, **gkw)
    tail = (d_w, None, 1, 0, n_dim, n_grid, d_acc, d_acc2, d_hist, None if sv is None else sv.ctypes.data, d_cube, d_sum, d_sum2,
            None if wg is None else capi.C.addressof(wg), B, None)
    if mc:
        return capi.lib().fdg_mc_accumulate_device_strat_grouped(h._h if h else None, d_in, 1, 8, d_in, 1, 8, 1.0, 2.0, 0.5, *tail)
    return capi.lib().fdg_accumulate_device_strat_grouped(h._h if h else None, d_in, 1, 8, 0, *tail)


def test_accumulate_argument_checks_need_no_device(libfdg):
    t = workloads.get("sigma2")
    h = capi.GraphHandle(t)
    for mc in (False, True):
        # the stratified calls' cases
        for kw in (dict(strat=None), dict(d_cube=None), dict(d_sum=None), dict(d_sum2=None), dict(strat=(2, 0, 1)), dict(d_sum2=FAKE5),
                   dict(d_sum=FAKE), dict(d_sum2=FAKE2), dict(d_sum=FAKE3), dict(d_acc=None), dict(d_acc2=None), dict(d_hist=None),
                   dict(d_hist=FAKE), dict(B=-1), dict(n_dim=0, strat=(), masks=((), ())), dict(n_grid=0)):
            assert failed(_acc(h, mc, **kw), capi.FDG_E_INVALID), kw
        assert failed(_acc(None, mc), capi.FDG_E_INVALID)
        assert failed(_acc(h, mc, strat=(1024, 1024, 2)), capi.FDG_E_UNSUPPORTED)
        assert failed(_acc(h, mc, n_grid=capi.FDG_VEGAS_GRID_MAX + 1), capi.FDG_E_UNSUPPORTED)
        # the grouped calls' cases
        for kw in (dict(wg=None), dict(null="root_group"), dict(null="var_mask"), dict(d_w=None), dict(n_group=0),
                   dict(root_group=[2] * t.n_root), dict(masks=((0, 1, 2), (3,))), dict(stride=99)):
            assert failed(_acc(h, mc, **kw), capi.FDG_E_INVALID), kw
        assert failed(_acc(h, mc, n_group=capi.FDG_WEIGHT_GROUP_MAX + 1), capi.FDG_E_UNSUPPORTED)
        assert _acc(h, mc, B=0) == capi.FDG_OK
    many = capi.GraphHandle(workloads.get("parquet_ver4_4"))                         # 180 roots and 2 groups
    assert failed(_acc(many, strat=(512, 256, 1)), capi.FDG_E_UNSUPPORTED)            # 2^17 * 182 > 2^24
    assert _acc(many, strat=(256, 256, 1), B=0) == capi.FDG_OK                        # 2^16 * 182 <= 2^24
    eight = tuple((0, 1, 2) for _ in range(8))
    assert failed(_acc(many, strat=(360, 256, 1), masks=eight), capi.FDG_E_UNSUPPORTED)     # 92160 * 188 > 2^24 >= 92160 * 181
    assert 92160 * 181 <= 1 << 24 < 92160 * 188
    assert _acc(many, strat=(360, 256, 1), masks=(eight[0],), B=0) == capi.FDG_OK
    assert failed(_acc(h, d_in=None), capi.FDG_E_INVALID)
    assert failed(_acc(h, True, d_in=None), capi.FDG_E_INVALID)
    assert failed(_acc(h, True), capi.FDG_E_INVALID)                                  # fdg_graph_specialize_fused has not been called
    wg, _keep = capi.make_weight_groups([0] * t.n_root, [(0, 1, 2)], 100)
    with pytest.raises(ValueError):
        h.accumulate_device_strat_grouped(FAKE, 1, 8, 0, FAKE7, None, 1, 0, 3, 8, FAKE, FAKE2, FAKE3, (2, 2), FAKE4, FAKE5, FAKE6, wg, 100)
    with pytest.raises(capi.FdgError) as e:
        h.mc_accumulate_device_strat_grouped(FAKE, 1, 8, FAKE, 1, 8, 1.0, 2.0, 0.5, FAKE7, None, 1, 0, 3, 8, FAKE, FAKE2, FAKE3, (2, 2, 1), 0,
                                             FAKE5, FAKE6, wg, 100)
    assert e.value.code == capi.FDG_E_INVALID


# ---- the allocator ------------------------------------------------------------------------------------------------------------------ #
def moments(rng, H, ld, counts):
    """per-hypercube sums and sums of squares of counts[h] random values of very different spread per (hypercube, column)"""
    s1, s2 = np.zeros((H, ld)), np.zeros((H, ld))
    for h in range(H):
        v = rng.normal(rng.uniform(-2, 2, ld), 10.0 ** rng.uniform(-3, 1, ld), size=(counts[h], ld))
        s1[h], s2[h] = v.sum(axis=0), (v * v).sum(axis=0)
    return s1, s2


@pytest.mark.parametrize("cols", [[2], [0, 3], [4, 1, 2]])
def test_allocate_cols_equals_its_restatement(libfdg, cols):
    rng = np.random.default_rng(100 + len(cols))
    for H, N in ((1, 50), (7, 1000), (256, 20_000), (1000, 2001)):
        old = capi.strat_allocate_cols(None, None, cols, None, H, N)
        assert np.array_equal(old, capi.strat_allocate_cols_reference(None, None, cols, None, H, N))
        for beta in (0.75, 1.0, 0.0, 0.3):
            s1, s2 = moments(rng, H, 5, np.diff(old))
            new = capi.strat_allocate_cols(s1, s2, cols, old, H, N, beta)
            assert np.array_equal(new, capi.strat_allocate_cols_reference(s1, s2, cols, old, H, N, beta)), (H, N, beta)
            assert new[0] == 0 and new[-1] == N and np.diff(new).min() >= 2 and np.diff(new).sum() == N
            if len(cols) == 1:
                assert np.array_equal(new, capi.strat_allocate(s1, s2, cols[0], old, H, N, beta))
                assert np.array_equal(new, capi.strat_allocate_reference(s1, s2, cols[0], old, H, N, beta))
            old = new
    # the order of the columns is the order of the fold; a column with all the variance steers the allocation alone
    s1, s2 = moments(rng, 7, 5, [40] * 7)
    start = capi.strat_allocate_cols(None, None, [0], None, 7, 280)
    s1[:, 1], s2[:, 1] = 3.0, 9.0 / 40.0                                            # forty equal values: no variance
    assert np.array_equal(capi.strat_allocate_cols(s1, s2, [2, 1], start, 7, 280), capi.strat_allocate(s1, s2, 2, start, 7, 280))


def test_allocate_cols_leaves_the_output_alone_on_every_error(libfdg):
    H, N, ld = 6, 100, 4
    rng = np.random.default_rng(3)
    old = capi.strat_allocate(None, None, 0, None, H, N)
    s1, s2 = moments(rng, H, ld, np.diff(old))

    def call(cols=(1, 3), n_col=None, null_cols=False, s1=s1, s2=s2, old=old, H=H, N=N, beta=0.75, null_new=False):
        out = np.full(H + 1, -7, dtype=np.int64)
        cv = u32(cols)
        rc = capi.lib().fdg_strat_allocate_cols(None if s1 is None else s1.ctypes.data, None if s2 is None else s2.ctypes.data, ld,
                                                None if null_cols else cv.ctypes.data, len(cols) if n_col is None else n_col,
                                                None if old is None else old.ctypes.data, H, N, beta, None if null_new else out.ctypes.data)
        assert rc == capi.FDG_OK or (out == -7).all()
        return rc

    assert call() == capi.FDG_OK
    assert call(old=None, s1=None, s2=None) == capi.FDG_OK
    for kw in (dict(null_cols=True), dict(n_col=0), dict(cols=(1, 4)), dict(cols=(4,)), dict(N=2 * H - 1), dict(beta=-0.1), dict(beta=1.5),
               dict(beta=float("nan")), dict(s1=None), dict(s2=None), dict(null_new=True), dict(H=0)):
        assert failed(call(**kw), capi.FDG_E_INVALID), kw
    bad = s2.copy()
    bad[2, 3] = np.inf                                                              # the second of the two columns
    assert failed(call(s2=bad), capi.FDG_E_INVALID)
    assert call(s2=bad, cols=(1, 2)) == capi.FDG_OK                                   # a column that is not named is not read
    short = old.copy()
    short[3] -= short[3] - short[2] - 1
    assert failed(call(old=short), capi.FDG_E_INVALID)
    assert failed(call(H=HMAX + 1, N=4 * HMAX, old=None), capi.FDG_E_UNSUPPORTED)
    with pytest.raises(ValueError):
        capi.strat_allocate_cols(s1, s2, [1], old[:-1], H, N)


# ---- the restatement's own ties ------------------------------------------------------------------------------------------------------- #
def test_reference_reduces_to_the_plain_restatements(libfdg):
    """no polar group and no weight group: capi.strat_reference; one stratum per variable: capi.grouped_jacobian on the plain map"""
    rng = np.random.default_rng(4)
    D, G, B = 4, 9, 500
    grid = capi.vegas_refine(vegas.uniform_grid([0.0] * D, [1.0, 2.0, 3.0, 6.0], G), rng.random((D, G)) + 0.1, 1.0)
    strat = (2, 1, 3, 1)
    start = np.concatenate([[0], np.cumsum([100, 50, 150, 2, 98, 100])]).astype(np.int64)
    u = oracle.philox_uniform(B, D, 6, 0)
    plain = capi.strat_reference(grid, strat, start, u)
    got = capi.strat_grouped_reference(grid, strat, start, u, [2, 0, 3, 1])
    assert np.array_equal(got["x"][:, [2, 0, 3, 1]], plain["x"]) and np.array_equal(got["jac"], plain["jac"])
    assert np.array_equal(got["cube"], plain["cube"]) and np.array_equal(got["cell"], plain["cell"])
    sets = ((0, 1, 2, 3), (0, 1), (2, 3))
    polar = [(0, (0, 1))]
    one = capi.strat_grouped_reference(grid, (1,) * D, np.array([0, B]), u, [None, None, 2, 3], polar, sets)
    f = np.float64(G) * (grid[np.arange(D)[None, :], one["cell"] + 1] - grid[np.arange(D)[None, :], one["cell"]])
    assert np.array_equal(one["jac"], capi.grouped_jacobian(f, sets, polar, value=one["value"]))
    assert np.allclose(np.hypot(one["x"][:, 0], one["x"][:, 1]), one["value"][:, 0], rtol=1e-14)


# ---- the driver's own checks ------------------------------------------------------------------------------------------------------------ #
def test_driver_checks_its_arguments_and_the_old_refusals_stand():
    h = capi.GraphHandle(workloads.get("sigma2"))
    R, L = h.table.n_root, h.table.n_leaf
    assert L >= 4
    lo, hi = DISC_LO + [0.0, 0.0], DISC_HI + [1.0, 1.0]
    polar = [vegas.PolarVar(0, (0, 1))]
    col = [None, None, 2, 3]
    s = vegas.Stratification((2, 2, 2, 2))
    kw = dict(n_sample=1000, n_grid=8, device="cpu")
    whole = vegas.WeightGroups((0,) * R, ((0, 1, 2, 3),))
    with pytest.raises(ValueError, match="whole or not at all"):
        vegas.vegas_integrate_stratified(h, None, lo, hi, col, s, polar=polar, groups=vegas.WeightGroups((0,) * R, ((0, 2, 3),)), **kw)
    for bad in ([R + 1], [-1], []):
        with pytest.raises(ValueError, match="alloc_cols"):
            vegas.vegas_integrate_stratified(h, None, lo, hi, col, s, polar=polar, groups=whole, alloc_cols=bad, **kw)
    with pytest.raises(ValueError, match="alloc_cols"):
        vegas.vegas_integrate_stratified(h, None, lo, hi, col, s, polar=polar, alloc_cols=[R + 1], **kw)     # without groups: R + 1 columns
    with pytest.raises(ValueError, match="one count"):
        vegas.vegas_integrate_stratified(h, None, lo, hi, col, vegas.Stratification((2, 2, 2)), polar=polar, groups=whole, **kw)
    with pytest.raises(ValueError, match="needs a Stratification"):
        vegas.vegas_integrate_stratified(h, None, lo, hi, col, None, polar=polar, **kw)
    with pytest.raises(ValueError, match="root_group"):
        vegas.vegas_integrate_stratified(h, None, lo, hi, col, s, groups=vegas.WeightGroups((0,) * (R + 1), ((0, 1, 2, 3),)), polar=polar, **kw)
    # vegas_integrate still refuses the combination, and says where it went
    args = (object(), None, [0, 0], [1, 1], [0, 1])
    for extra in (dict(polar=[vegas.PolarVar(0, (0, 1))]), dict(groups=vegas.WeightGroups((0,), ((0, 1),)))):
        with pytest.raises(ValueError, match="strat cannot be combined") as e:
            vegas.vegas_integrate(*args, strat=vegas.Stratification((2, 2)), **extra)
        assert "vegas_integrate_stratified" in str(e.value)
