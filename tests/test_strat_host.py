"""Adaptive stratified sampling without a device (include/fdg.h: fdg_vegas_sample_device_strat, fdg_accumulate_device_strat,
fdg_mc_accumulate_device_strat, fdg_strat_allocate; feynmandiagram.jl_amd/vegas.py: Stratification, strat_for): the symbols are
declared, exported and bound, every argument check runs before any device work, the host-only allocator follows the steps the header
states -- checked against the Python restatement in capi -- and the numpy mirror of the whole driver (what tests/test_strat_accumulate.py
compares the device with) meets on the CPU the conditions that file asserts on the GPU."""
import math
import re

import numpy as np
import pytest

import oracle
from feynmandiagram_jl_amd import capi, vegas, workloads
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_vegas_host import JL, mirror_map

NAMES = ("fdg_vegas_sample_device_strat", "fdg_accumulate_device_strat", "fdg_mc_accumulate_device_strat", "fdg_strat_allocate")
FAKE, FAKE2, FAKE3, FAKE4, FAKE5, FAKE6 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000   # compared with NULL and each other only
HMAX = capi.FDG_STRAT_CUBE_MAX


# ---- the numpy mirror of the driver --------------------------------------------------------------------------------------------------- #
def ridge(a):
    """f(x, y) = 1 / ((x - y)^2 + a^2) and its integral over the unit square"""
    return (lambda x: 1.0 / ((x[:, 0] - x[:, 1]) ** 2 + a * a)), 2.0 * (math.atan(1.0 / a) / a - math.log(1.0 + 1.0 / (a * a)) / 2.0)


def mirror_integrate(f, lo, hi, n_grid, n_sample, n_iter, seed, alpha=0.5, strat=None, beta=0.75):
    """vegas.vegas_integrate on the CPU for one root f(x): the iterations [(mean, stderr)] and the counts per hypercube.  The samples
    are the device's bit for bit (oracle.philox_uniform, test_vegas_host.mirror_map, capi.strat_reference); the sums are numpy's."""
    grid = vegas.uniform_grid(lo, hi, n_grid)
    D, N = grid.shape[0], int(n_sample)
    its, counts = [], []
    if strat is not None:
        H = int(np.prod(strat))
        start = capi.strat_allocate_reference(None, None, 0, None, H, N, beta)
    for it in range(n_iter):
        if strat is None:
            x, jac, c = mirror_map(grid, oracle.philox_uniform(N, D, seed, it * N))
            t = f(x) * jac
            mean = t.sum() / N
            its.append((mean, math.sqrt(max(0.0, ((t * t).sum() / N - mean * mean) / (N - 1)))))
        else:
            r = capi.strat_reference(grid, strat, start, oracle.philox_uniform(N, D, vegas._iteration_seed(seed, it), 0))
            x, jac, c = r["x"], r["jac"], r["cell"]
            t = f(x) * jac
            s1 = np.bincount(r["cube"], weights=t, minlength=H)[:, None]
            s2 = np.bincount(r["cube"], weights=t * t, minlength=H)[:, None]
            its.append((t.sum() / N, math.sqrt(vegas.strat_variance(s1, s2, np.diff(start), N)[0])))
            counts.append(np.diff(start))
            start = capi.strat_allocate_reference(s1, s2, 0, start, H, N, beta)
        hist = np.stack([np.bincount(c[:, d], weights=t * t, minlength=n_grid) for d in range(D)])
        capi.vegas_refine(grid, hist, alpha)
    return its, counts


# the known-answer case of tests/test_strat_accumulate.py: a ridge along the diagonal, which no separable map can see
KNOWN = dict(a=0.02, S=16, n_sample=200_000, n_iter=5, n_grid=64, seed=2024)
CALIB = dict(a=0.02, S=16, n_sample=20_000, n_grid=64, n_seed=32)


def test_mirror_meets_the_conditions_of_the_gpu_tests(libfdg):
    """Conditions, not measurements: the GPU file asserts ratio <= 0.5 and 12 <= chi2 <= 60; the mirror must give a ratio of at most
    0.25 and a chi2 inside the same range, or the parameters above are the wrong ones."""
    f, exact = ridge(KNOWN["a"])
    k = KNOWN
    plain, _ = mirror_integrate(f, [0, 0], [1, 1], k["n_grid"], k["n_sample"], k["n_iter"], k["seed"])
    strat, counts = mirror_integrate(f, [0, 0], [1, 1], k["n_grid"], k["n_sample"], k["n_iter"], k["seed"], strat=(k["S"], k["S"]))
    mp, ep, _ = vegas.combine([(np.array([m]), np.array([e])) for m, e in plain])
    ms, es, _ = vegas.combine([(np.array([m]), np.array([e])) for m, e in strat])
    ratio = (es[0] / ep[0]) ** 2
    print("plain", mp[0], ep[0], "strat", ms[0], es[0], "exact", exact, "variance ratio", ratio)
    assert abs(mp[0] - exact) < 5 * ep[0] and abs(ms[0] - exact) < 5 * es[0]
    assert ratio <= 0.25
    assert all(c.sum() == k["n_sample"] and c.min() >= 2 for c in counts) and counts[-1].max() > 4 * counts[0].max()
    f, exact = ridge(CALIB["a"])
    c = CALIB
    chi2 = 0.0
    for seed in range(c["n_seed"]):
        (m, e), = mirror_integrate(f, [0, 0], [1, 1], c["n_grid"], c["n_sample"], 1, seed, strat=(c["S"], c["S"]))[0]
        chi2 += ((m - exact) / e) ** 2
    print("calibration chi2 over", c["n_seed"], "seeds:", chi2)
    assert 12.0 <= chi2 <= 60.0


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
    for fn in ("vegas_sample_device_strat!", "accumulate_device_strat!", "mc_accumulate_device_strat!", "strat_allocate!"):
        assert fn in export, fn
    import feynmandiagram_jl_amd as fd
    assert fd.Stratification is vegas.Stratification and fd.strat_for is vegas.strat_for
    assert capi.FDG_STRAT_CUBE_MAX == 1 << 20


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def u32(v):
    return np.ascontiguousarray(v, dtype=np.uint32)


def _sample(strat=(2, 2, 1), n_dim=3, n_grid=8, d_grid=FAKE, d_x=FAKE2, d_jac=FAKE3, d_start=FAKE4, d_cube=FAKE5, B=100):
    sv = None if strat is None else u32(strat)
    return capi.lib().fdg_vegas_sample_device_strat(d_grid, n_dim, n_grid, None, None if sv is None else sv.ctypes.data, d_start, 1, 0, d_x, 1,
                                                    100, d_jac, d_cube, None, B, None)


def _tail(strat, d_cube, d_sum, d_sum2):
    sv = None if strat is None else u32(strat)
    return sv, (None if sv is None else sv.ctypes.data, d_cube, d_sum, d_sum2)


def _acc(h, strat=(2, 2, 1), n_dim=3, n_grid=8, B=100, d_leaf=FAKE, d_acc=FAKE, d_acc2=FAKE2, d_hist=FAKE3, d_cube=FAKE4, d_sum=FAKE5,
         d_sum2=FAKE6):
    sv, tail = _tail(strat, d_cube, d_sum, d_sum2)
    return capi.lib().fdg_accumulate_device_strat(h._h if h else None, d_leaf, 1, 8, 0, None, None, 1, 0, n_dim, n_grid, d_acc, d_acc2, d_hist,
                                                  *tail, B, None)


def _mc(h, strat=(2, 2, 1), n_dim=3, n_grid=8, B=100, d_K=FAKE, d_T=FAKE, d_acc=FAKE, d_acc2=FAKE2, d_hist=FAKE3, d_cube=FAKE4, d_sum=FAKE5,
        d_sum2=FAKE6):
    sv, tail = _tail(strat, d_cube, d_sum, d_sum2)
    return capi.lib().fdg_mc_accumulate_device_strat(h._h if h else None, d_K, 1, 8, d_T, 1, 8, 1.0, 2.0, 0.5, None, None, 1, 0, n_dim, n_grid,
                                                     d_acc, d_acc2, d_hist, *tail, B, None)


def failed(rc, code):
    return rc == code and len(capi.lib().fdg_last_error()) > 0


def test_sampler_argument_checks_need_no_device(libfdg):
    assert failed(_sample(strat=None), capi.FDG_E_INVALID)
    assert failed(_sample(d_start=None), capi.FDG_E_INVALID)
    assert failed(_sample(d_cube=None), capi.FDG_E_INVALID)
    assert failed(_sample(strat=(2, 0, 1)), capi.FDG_E_INVALID)
    assert failed(_sample(strat=(1024, 1024, 2)), capi.FDG_E_UNSUPPORTED)            # H = 2^21
    assert failed(_sample(strat=(65536, 65536, 65536)), capi.FDG_E_UNSUPPORTED)      # the product overflows 32 bits: still caught
    for kw in (dict(d_grid=None), dict(d_x=None), dict(d_jac=None), dict(B=-1), dict(n_dim=0, strat=()), dict(n_grid=0)):
        assert failed(_sample(**kw), capi.FDG_E_INVALID), kw
    assert failed(_sample(n_grid=capi.FDG_VEGAS_GRID_MAX + 1), capi.FDG_E_UNSUPPORTED)
    assert _sample(B=0) == capi.FDG_OK                                              # valid and nothing to do: no device work
    assert _sample(strat=(1024, 1024, 1), B=0) == capi.FDG_OK                        # H = 2^20 exactly
    with pytest.raises(ValueError):
        capi.vegas_sample_device_strat(FAKE, 3, 8, None, (2, 2), FAKE4, 1, 0, FAKE2, 1, 100, FAKE3, FAKE5, 0, 100)   # one count per variable
    with pytest.raises(capi.FdgError) as e:
        capi.vegas_sample_device_strat(FAKE, 3, 8, None, (2, 2, 0), FAKE4, 1, 0, FAKE2, 1, 100, FAKE3, FAKE5, 0, 100)
    assert e.value.code == capi.FDG_E_INVALID


def test_accumulate_argument_checks_need_no_device(libfdg):
    t = workloads.get("sigma2")
    h = capi.GraphHandle(t)
    for call in (_acc, _mc):
        for kw in (dict(strat=None), dict(d_cube=None), dict(d_sum=None), dict(d_sum2=None), dict(strat=(2, 0, 1)), dict(d_sum2=FAKE5),
                   dict(d_sum=FAKE), dict(d_sum2=FAKE2), dict(d_sum=FAKE3), dict(d_acc=None), dict(d_acc2=None), dict(d_hist=None),
                   dict(d_hist=FAKE), dict(B=-1), dict(n_dim=0, strat=()), dict(n_grid=0)):
            assert failed(call(h, **kw), capi.FDG_E_INVALID), kw
        assert failed(call(None), capi.FDG_E_INVALID)
        assert failed(call(h, strat=(1024, 1024, 2)), capi.FDG_E_UNSUPPORTED)
        assert failed(call(h, n_grid=capi.FDG_VEGAS_GRID_MAX + 1), capi.FDG_E_UNSUPPORTED)
        # H * (n_root + 1) > 2^24 with H within its own limit
        big = (1024, 1024, 1)
        want = capi.FDG_E_UNSUPPORTED if (1 << 20) * (t.n_root + 1) > (1 << 24) else None
        if want is not None:
            assert failed(call(h, strat=big), want)
        assert call(h, B=0) == capi.FDG_OK
    many = capi.GraphHandle(workloads.get("parquet_ver4_4"))                         # 180 roots: 2^17 hypercubes are too many
    assert failed(_acc(many, strat=(512, 256, 1)), capi.FDG_E_UNSUPPORTED)
    assert _acc(many, strat=(256, 256, 1), B=0) == capi.FDG_OK                        # 2^16 * 181 <= 2^24
    assert failed(_acc(h, d_leaf=None), capi.FDG_E_INVALID)
    assert failed(_mc(h, d_K=None), capi.FDG_E_INVALID)
    assert failed(_mc(h), capi.FDG_E_INVALID)                                        # fdg_graph_specialize_fused has not been called
    with pytest.raises(ValueError):
        h.accumulate_device_strat(FAKE, 1, 8, 0, 0, None, 1, 0, 3, 8, FAKE, FAKE2, FAKE3, (2, 2), FAKE4, FAKE5, FAKE6, 100)
    with pytest.raises(capi.FdgError) as e:
        h.mc_accumulate_device_strat(FAKE, 1, 8, FAKE, 1, 8, 1.0, 2.0, 0.5, 0, None, 1, 0, 3, 8, FAKE, FAKE2, FAKE3, (2, 2, 1), 0, FAKE5, FAKE6, 100)
    assert e.value.code == capi.FDG_E_INVALID


# ---- the allocator ------------------------------------------------------------------------------------------------------------------ #
def random_moments(rng, start, ld, scale=1.0):
    """per-hypercube sums of n_h random terms each, so that sum2 >= sum^2 / n as real moments do"""
    H = len(start) - 1
    s1, s2 = np.zeros((H, ld)), np.zeros((H, ld))
    for h in range(H):
        t = rng.normal(rng.uniform(-1, 1), rng.uniform(0, 3) ** 4 * scale, size=(int(start[h + 1] - start[h]), ld))
        s1[h], s2[h] = t.sum(axis=0), (t * t).sum(axis=0)
    return s1, s2


def test_allocate_sums_to_n_total_with_at_least_two_each(libfdg):
    rng = np.random.default_rng(1)
    for H, N in ((1, 2), (1, 1000), (7, 14), (7, 15), (12, 1000), (256, 200_000), (1000, 2003)):
        uni = capi.strat_allocate(None, None, 0, None, H, N)
        assert uni[0] == 0 and uni[-1] == N and np.diff(uni).min() >= 2 and np.diff(uni).max() - np.diff(uni).min() <= 1
        s1, s2 = random_moments(rng, uni, 3)
        for beta in (0.25, 0.75, 1.0):
            new = capi.strat_allocate(s1, s2, 2, uni, H, N, beta)
            assert new[0] == 0 and new[-1] == N and np.diff(new).min() >= 2, (H, N, beta)
            # ... and a total that differs from the old one
            assert capi.strat_allocate(s1, s2, 2, uni, H, 3 * N + 1, beta)[-1] == 3 * N + 1


def test_allocate_is_uniform_without_variance_or_with_beta_zero(libfdg):
    rng = np.random.default_rng(2)
    H, N = 12, 1003
    uni = capi.strat_allocate(None, None, 0, None, H, N)
    assert np.array_equal(np.diff(uni), [84] * 7 + [83] * 5)
    old = capi.strat_allocate(*random_moments(rng, uni, 1), 0, uni, H, N, 1.0)
    assert not np.array_equal(old, uni)
    s1, s2 = random_moments(rng, old, 2)
    assert np.array_equal(capi.strat_allocate(s1, s2, 1, old, H, N, 0.0), uni)
    const = np.diff(old)[:, None] * np.array([[0.0, 2.5]])                           # every term 0 or 2.5: no variance
    assert np.array_equal(capi.strat_allocate(const, const * np.array([[0.0, 2.5]]), 1, old, H, N, 0.75), uni)
    assert np.array_equal(capi.strat_allocate(const, const, 0, old, H, N, 0.75), uni)
    # all of the variance in one hypercube: it receives everything beyond two each
    one = np.zeros((H, 1)), np.zeros((H, 1))
    one[1][5] = 7.0
    got = np.diff(capi.strat_allocate(one[0], one[1], 0, old, H, N, 0.75))
    assert got[5] == N - 2 * (H - 1) and (np.delete(got, 5) == 2).all()


def test_allocate_matches_the_python_restatement_exactly(libfdg):
    rng = np.random.default_rng(3)
    for H, N, ld in ((1, 50, 1), (5, 64, 2), (96, 10_000, 3), (256, 200_000, 2), (1000, 2500, 1)):
        start = capi.strat_allocate(None, None, 0, None, H, N)
        for rnd in range(4):
            s1, s2 = random_moments(rng, start, ld, scale=10.0 ** rng.integers(-3, 4))
            col, beta, n_new = int(rng.integers(0, ld)), float(rng.choice([0.0, 0.3, 0.75, 1.0])), int(N + rng.integers(0, 50))
            got = capi.strat_allocate(s1, s2, col, start, H, n_new, beta)
            want = capi.strat_allocate_reference(s1, s2, col, start, H, n_new, beta)
            assert np.array_equal(got, want), (H, N, rnd, beta)
            start = capi.strat_allocate(s1, s2, col, start, H, N, 0.75)              # the next round starts from an uneven allocation
        assert np.diff(start).max() > np.diff(start).min() + 1 or H == 1


def test_allocate_errors_leave_start_new_untouched(libfdg):
    H, N = 6, 100
    old = capi.strat_allocate(None, None, 0, None, H, N)
    s1, s2 = random_moments(np.random.default_rng(4), old, 2)

    def call(s1=s1, s2=s2, ld=2, col=1, old=old, H=H, N=N, beta=0.75, null_new=False):
        out = np.full(H + 1 if H <= 64 else 1, -5, dtype=np.int64)
        rc = capi.lib().fdg_strat_allocate(None if s1 is None else s1.ctypes.data, None if s2 is None else s2.ctypes.data, ld, col,
                                           None if old is None else old.ctypes.data, H, N, beta, None if null_new else out.ctypes.data)
        assert (out == -5).all() or rc == capi.FDG_OK
        return rc

    assert call() == capi.FDG_OK
    assert failed(call(N=2 * H - 1), capi.FDG_E_INVALID)
    for beta in (-0.1, 1.1, float("nan"), float("inf")):
        assert failed(call(beta=beta), capi.FDG_E_INVALID)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for which in (0, 1):
            m = [s1.copy(), s2.copy()]
            m[which][3, 1] = bad
            assert failed(call(s1=m[0], s2=m[1]), capi.FDG_E_INVALID)
    m = s1.copy()
    m[3, 0] = float("nan")                                                           # another column: not read
    assert call(s1=m) == capi.FDG_OK
    short = old.copy()
    short[3] -= short[3] - short[2] - 1                                             # hypercube 2 holds one sample
    assert failed(call(old=short), capi.FDG_E_INVALID)
    assert failed(call(s1=None), capi.FDG_E_INVALID)
    assert failed(call(s2=None), capi.FDG_E_INVALID)
    assert failed(call(null_new=True), capi.FDG_E_INVALID)
    assert failed(call(col=2), capi.FDG_E_INVALID)
    assert failed(call(H=0), capi.FDG_E_INVALID)
    assert failed(call(H=HMAX + 1, N=4 * HMAX, old=None), capi.FDG_E_UNSUPPORTED)
    with pytest.raises(capi.FdgError):
        capi.strat_allocate(s1, s2, 1, old, H, 5)
    with pytest.raises(ValueError):
        capi.strat_allocate(s1, s2, 1, old[:-1], H, N)


# ---- Lepage's rule and the driver's keyword -------------------------------------------------------------------------------------------- #
def test_strat_for_gives_lepages_numbers():
    assert vegas.strat_for(200_000, 2) == (223, 223)                 # (2e5 / 4)^(1/2) = 223.6
    assert vegas.strat_for(1_000_000, 4) == (22, 22, 22, 22)         # 250000^(1/4) = 22.36
    assert vegas.strat_for(256, 3) == (4, 4, 4)                      # 64^(1/3) is 3.9999999999999996 in floating point
    assert vegas.strat_for(1000, 9) == (1,) * 9                      # 250^(1/9) = 1.85
    assert vegas.strat_for(3, 2) == (1, 1)
    assert vegas.strat_for(10 ** 8, 17) == (2,) * 17                 # 2.5e7^(1/17) = 2.72: 2^17 hypercubes
    assert vegas.strat_for(10 ** 9, 2) == (1024, 1024)               # 15811^2 > 2^20: one stratum less per axis, from the last, in rounds
    assert vegas.strat_for(10 ** 9, 3) == (102, 101, 101)            # 629^3 > 2^20; 102 * 101 * 101 = 1040502
    assert vegas.strat_for(200_000, 2, max_cubes=49_000) == (221, 221)
    assert math.prod(vegas.strat_for(10 ** 9, 3)) <= capi.FDG_STRAT_CUBE_MAX
    with pytest.raises(ValueError):
        vegas.strat_for(0, 2)


def test_driver_refuses_the_excluded_combinations():
    s = vegas.Stratification((2, 2))
    assert s.beta == 0.75
    args = (object(), None, [0, 0], [1, 1], [0, 1])
    for kw in (dict(polar=[vegas.PolarVar(0, (0, 1))]), dict(matsubara=vegas.MatsubaraProjection((0,), True, (1,), (1,))),
               dict(groups=vegas.WeightGroups((0,), ((0, 1),))), dict(observables=vegas.Observables(((1.0,),)))):
        with pytest.raises(ValueError, match="strat cannot be combined"):
            vegas.vegas_integrate(*args, strat=s, **kw)
    with pytest.raises(ValueError, match="strat cannot be combined"):
        vegas.vegas_integrate_binned(*args, object(), strat=s)
