"""The discrete external variable of VEGAS without a device (include/fdg.h: fdg_vegas_sample_device_discrete,
fdg_accumulate_device_vegas_binned, fdg_mc_accumulate_device_vegas_binned, fdg_vegas_refine_discrete): the four symbols are declared,
exported and bound, every argument check runs before any device work, and the host-only refinement of the probabilities follows the six
steps the header states -- checked against a numpy mirror written here.  The mirrors of the sampler and of the refinement are what
tests/test_vegas_discrete_accumulate.py compares the device with."""
import os
import re

import numpy as np
import pytest

import oracle
from feynmandiagram_jl_amd import capi, vegas, workloads
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_vegas_host import mirror_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "feynmandiagram.jl_amd", "julia", "hip_compiler.jl")
NAMES = ("fdg_vegas_sample_device_discrete", "fdg_accumulate_device_vegas_binned", "fdg_mc_accumulate_device_vegas_binned",
         "fdg_vegas_refine_discrete")
FAKE, FAKE2, FAKE3, FAKE4, FAKE5 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # only compared with NULL or each other; never read through
DMAX, GMAX, BMAX, EMAX = capi.FDG_VEGAS_DIM_MAX, capi.FDG_VEGAS_GRID_MAX, capi.FDG_BIN_MAX, capi.FDG_VEGAS_EXT_MAX
TOL = 1e-12


# ---- numpy mirrors ------------------------------------------------------------------------------------------------------------------ #
def mirror_refine_discrete(cdf, hist_bin, alpha, floor):
    """Steps 1-5 of fdg_vegas_refine_discrete (include/fdg.h) in numpy (np.cumsum is the left fold); the arguments are taken as valid."""
    cdf = np.array(cdf, dtype=np.float64)
    n = cdf.shape[0] - 1
    q = np.asarray(hist_bin, dtype=np.float64) * (cdf[1:] - cdf[:-1])
    qs = np.cumsum(q)[-1]
    if not qs > 0.0 or alpha == 0.0 or n == 1:
        return cdf
    s = q / qs
    w = np.where(s > 0.0, s ** alpha, 0.0)
    p = (1.0 - floor) * w / np.cumsum(w)[-1] + floor / n
    out = np.concatenate([[0.0], np.cumsum(p)])
    out[n] = 1.0
    return out


def mirror_sample_discrete(grid, cdf, seed, sample_offset, n_sample, bin_base=0):
    """x [B, D], jac [B], bin [B], cell [B, D]: the continuous variables through mirror_map, the discrete one from Philox column D"""
    D, n = grid.shape[0], cdf.shape[0] - 1
    u = oracle.philox_uniform(n_sample, D + 1, seed, sample_offset)
    x, jc, c = mirror_map(grid, np.ascontiguousarray(u[:, :D]))
    j = np.searchsorted(cdf[1:n], u[:, D], side="right")
    p = cdf[j + 1] - cdf[j]
    return x, jc / p, (j + bin_base).astype(np.int32), c


# ---- declared, exported, bound ------------------------------------------------------------------------------------------------------ #
def test_symbols_are_declared_exported_and_bound(libfdg):
    protos = c_prototypes()
    calls = {c[0]: c for c in jl_ccalls()}
    export = re.search(r"^export\s+([^\n]*)", open(JL).read(), flags=re.M).group(1)
    for name in NAMES:
        assert name in protos, name
        assert name in capi.EXPORTS, name
        assert hasattr(libfdg, name), name
        assert name in calls, name + ": not bound in the Julia shim"
        _, _, types, args = calls[name]
        params = protos[name][1]
        assert len(types) == len(params) == len(args) == len(getattr(libfdg, name).argtypes), name
        for jt, cp in zip(types, params):
            assert jl_class(jt) == c_class(cp), (name, jt, cp)
    for fn in ("vegas_sample_device_discrete!", "accumulate_device_vegas_binned!", "mc_accumulate_device_vegas_binned!",
               "vegas_refine_discrete!"):
        assert fn in [x.strip() for x in export.split(",")], fn
    for name in ("accumulate_device_vegas_binned", "mc_accumulate_device_vegas_binned"):
        assert hasattr(capi.GraphHandle, name)
    import feynmandiagram_jl_amd as fd
    assert fd.DiscreteMap is vegas.DiscreteMap and fd.vegas_integrate_binned is vegas.vegas_integrate_binned
    assert hasattr(fd.compilers.GraphFunc, "accumulate_vegas_binned")


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def _u32(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.uint32)


def _sample(n_dim=3, n_grid=8, col=None, d_grid=FAKE, d_cdf=FAKE4, n_bin=5, d_ext=None, ext_col=None, n_ext=None, d_x=FAKE2, d_jac=FAKE3,
            d_bin=FAKE5, B=100):
    c, e = _u32(col), _u32(ext_col)
    n_ext = (0 if e is None else e.shape[0]) if n_ext is None else n_ext
    return capi.lib().fdg_vegas_sample_device_discrete(d_grid, n_dim, n_grid, None if c is None else c.ctypes.data, d_cdf, n_bin, 0, d_ext, n_ext,
                                                       None if e is None else e.ctypes.data, 1, 0, d_x, 1, 100, d_jac, d_bin, None, B, None)


def _acc(h, n_dim=3, n_grid=8, n_bin=5, B=100, d_leaf=FAKE, d_bin=FAKE5, d_acc=FAKE, d_acc2=FAKE2, d_hist=FAKE3, d_hist_bin=FAKE4, lts=0):
    return capi.lib().fdg_accumulate_device_vegas_binned(h._h if h else None, d_leaf, 1, 8, lts, d_bin, 0, n_bin, None, None, 1, 0, n_dim, n_grid,
                                                         d_acc, d_acc2, d_hist, d_hist_bin, B, None)


def _mc(h, n_dim=3, n_grid=8, n_bin=5, B=100, d_K=FAKE, d_T=FAKE, d_bin=FAKE5, d_acc=FAKE, d_acc2=FAKE2, d_hist=FAKE3, d_hist_bin=FAKE4):
    return capi.lib().fdg_mc_accumulate_device_vegas_binned(h._h if h else None, d_K, 1, 8, d_T, 1, 8, 1.0, 2.0, 0.5, d_bin, 0, n_bin, None, None,
                                                            1, 0, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, B, None)


def test_limits_in_every_call(libfdg):
    h = capi.GraphHandle(workloads.get("sigma2"))
    for call in (lambda **kw: _sample(**kw), lambda **kw: _acc(h, **kw), lambda **kw: _mc(h, **kw)):
        assert call(n_dim=0) == capi.FDG_E_INVALID
        assert call(n_grid=0) == capi.FDG_E_INVALID
        assert call(n_dim=DMAX + 1) == capi.FDG_E_UNSUPPORTED
        assert call(n_grid=GMAX + 1) == capi.FDG_E_UNSUPPORTED
        assert call(n_bin=0) == capi.FDG_E_INVALID
        assert call(n_bin=BMAX + 1) == capi.FDG_E_UNSUPPORTED
        assert call(n_dim=DMAX, n_grid=GMAX, n_bin=BMAX, B=0) == capi.FDG_OK
    cdf, hist = np.linspace(0.0, 1.0, BMAX + 2), np.ones(BMAX + 1)
    assert capi.lib().fdg_vegas_refine_discrete(cdf.ctypes.data, hist.ctypes.data, 0, 0.5, 0.0) == capi.FDG_E_INVALID
    assert capi.lib().fdg_vegas_refine_discrete(cdf.ctypes.data, hist.ctypes.data, BMAX + 1, 0.5, 0.0) == capi.FDG_E_UNSUPPORTED
    assert np.array_equal(cdf, np.linspace(0.0, 1.0, BMAX + 2))


def test_sampler_argument_checks_need_no_device(libfdg):
    for name in ("d_grid", "d_cdf", "d_x", "d_jac", "d_bin"):
        assert _sample(**{name: None}) == capi.FDG_E_INVALID, name
    assert _sample(B=-1) == capi.FDG_E_INVALID
    assert _sample(B=0) == capi.FDG_OK                                     # valid and nothing to do: no device work
    assert _sample(d_ext=FAKE, ext_col=[3, 4], B=0) == capi.FDG_OK
    assert _sample(d_ext=FAKE, ext_col=list(range(3, 3 + EMAX)), B=0) == capi.FDG_OK
    assert _sample(d_ext=FAKE, ext_col=list(range(3, 4 + EMAX))) == capi.FDG_E_UNSUPPORTED
    assert _sample(d_ext=None, ext_col=[3, 4]) == capi.FDG_E_INVALID       # a table's columns without the table
    assert _sample(d_ext=FAKE, ext_col=None, n_ext=2) == capi.FDG_E_INVALID
    assert _sample(d_ext=FAKE, ext_col=[3, 4, 3]) == capi.FDG_E_INVALID    # repeats
    assert _sample(d_ext=FAKE, ext_col=[3, 2]) == capi.FDG_E_INVALID       # names a column of the default col = 0, 1, 2
    assert _sample(col=[5, 0, 7], d_ext=FAKE, ext_col=[1, 7]) == capi.FDG_E_INVALID
    assert _sample(col=[5, 0, 7], d_ext=FAKE, ext_col=[1, 2], B=0) == capi.FDG_OK
    with pytest.raises(capi.FdgError) as e:
        capi.vegas_sample_device_discrete(FAKE, 3, 8, None, FAKE4, BMAX + 1, 0, 0, None, 1, 0, FAKE2, 1, 100, FAKE3, FAKE5, 0, 100)
    assert e.value.code == capi.FDG_E_UNSUPPORTED
    with pytest.raises(ValueError):
        capi.vegas_sample_device_discrete(FAKE, 3, 8, [0, 1], FAKE4, 5, 0, 0, None, 1, 0, FAKE2, 1, 100, FAKE3, FAKE5, 0, 100)


def test_accumulate_argument_checks_need_no_device(libfdg):
    h = capi.GraphHandle(workloads.get("sigma2"))
    for call in (_acc, _mc):
        for name in ("d_acc", "d_acc2", "d_hist", "d_bin"):
            assert call(h, **{name: None}) == capi.FDG_E_INVALID, name
        assert call(h, d_bin=None, n_bin=1) == capi.FDG_E_INVALID          # no bin vector: the call without a discrete variable
        assert call(h, d_acc2=FAKE) == capi.FDG_E_INVALID                  # any two of the four the same buffer
        assert call(h, d_hist=FAKE) == capi.FDG_E_INVALID
        assert call(h, d_hist=FAKE2) == capi.FDG_E_INVALID
        assert call(h, d_hist_bin=FAKE) == capi.FDG_E_INVALID
        assert call(h, d_hist_bin=FAKE2) == capi.FDG_E_INVALID
        assert call(h, d_hist_bin=FAKE3) == capi.FDG_E_INVALID
        assert call(h, B=-1) == capi.FDG_E_INVALID
        assert call(None) == capi.FDG_E_INVALID
        assert call(h, B=0) == capi.FDG_OK
        assert call(h, d_hist_bin=None, B=0) == capi.FDG_OK                # the discrete variable is not trained
    assert _acc(h, d_leaf=None) == capi.FDG_E_INVALID
    assert _mc(h, d_K=None) == capi.FDG_E_INVALID
    assert _mc(h, d_T=None) == capi.FDG_E_INVALID
    assert _mc(h) == capi.FDG_E_INVALID                                    # fdg_graph_specialize_fused has not been called
    assert _acc(h, lts=8 * 64) == capi.FDG_E_UNSUPPORTED                   # a tile-major batch on a handle without FDG_SPEC_ISA
    with pytest.raises(capi.FdgError) as e:
        h.accumulate_device_vegas_binned(FAKE, 1, 8, 0, FAKE5, 0, 5, 0, None, 1, 0, 3, GMAX + 1, FAKE, FAKE2, FAKE3, FAKE4, 100)
    assert e.value.code == capi.FDG_E_UNSUPPORTED
    with pytest.raises(capi.FdgError) as e:
        h.mc_accumulate_device_vegas_binned(FAKE, 1, 8, FAKE, 1, 8, 1.0, 2.0, 0.5, FAKE5, 0, 5, 0, None, 1, 0, 3, 8, FAKE, FAKE2, FAKE3, FAKE3, 100)
    assert e.value.code == capi.FDG_E_INVALID
    with pytest.raises(ValueError):
        h.accumulate_device_vegas_binned(FAKE, 1, 8, 0, FAKE5, 0, 5, 0, [1.0], 1, 0, 3, 8, FAKE, FAKE2, FAKE3, FAKE4, 100)   # coef: one per root


def test_refine_argument_checks(libfdg):
    c0, flat = vegas.uniform_cdf(16), np.ones(16)
    L = capi.lib()
    for alpha, floor in ((-0.1, 0.0), (2.1, 0.0), (float("nan"), 0.0), (0.5, -0.1), (0.5, 1.0), (0.5, float("nan")), (float("inf"), 0.0)):
        c = c0.copy()
        assert L.fdg_vegas_refine_discrete(c.ctypes.data, flat.ctypes.data, 16, alpha, floor) == capi.FDG_E_INVALID, (alpha, floor)
        assert np.array_equal(c, c0)
    for v in (-1.0, float("nan"), float("inf")):
        h, c = flat.copy(), c0.copy()
        h[5], h[:3] = v, 50.0
        assert L.fdg_vegas_refine_discrete(c.ctypes.data, h.ctypes.data, 16, 0.5, 0.05) == capi.FDG_E_INVALID
        assert np.array_equal(c, c0)
    for i, v in ((0, 1e-3), (16, 1.0 - 1e-12), (16, 1.5), (7, c0[6]), (7, c0[8]), (7, float("nan"))):   # not 0 .. 1, not strictly increasing
        c = c0.copy()
        c[i] = v
        keep = c.copy()
        assert L.fdg_vegas_refine_discrete(c.ctypes.data, flat.ctypes.data, 16, 0.5, 0.05) == capi.FDG_E_INVALID, (i, v)
        assert np.array_equal(c, keep, equal_nan=True)
    assert L.fdg_vegas_refine_discrete(None, flat.ctypes.data, 16, 0.5, 0.0) == capi.FDG_E_INVALID
    assert L.fdg_vegas_refine_discrete(c0.ctypes.data, None, 16, 0.5, 0.0) == capi.FDG_E_INVALID
    with pytest.raises(capi.FdgError):
        capi.vegas_refine_discrete(c0.copy(), flat, 3.0)
    with pytest.raises(ValueError):
        capi.vegas_refine_discrete(c0.copy(), np.ones(15))


# ---- the refinement ----------------------------------------------------------------------------------------------------------------- #
def test_refine_unchanged_cases_and_end_points(libfdg):
    rng = np.random.default_rng(0)
    c0 = capi.vegas_refine_discrete(vegas.uniform_cdf(64), rng.random(64) + 0.1, 1.0, 0.1)
    assert not np.array_equal(c0, vegas.uniform_cdf(64)) and c0[0] == 0.0 and c0[64] == 1.0
    h = rng.random(64)
    assert np.array_equal(capi.vegas_refine_discrete(c0.copy(), h, 0.0, 0.3).view(np.uint64), c0.view(np.uint64))        # alpha = 0
    assert np.array_equal(capi.vegas_refine_discrete(c0.copy(), np.zeros(64), 0.5, 0.3).view(np.uint64), c0.view(np.uint64))
    c1 = vegas.uniform_cdf(1)
    assert np.array_equal(capi.vegas_refine_discrete(c1.copy(), np.array([5.0]), 0.5, 0.2), c1)                            # n_bin = 1
    # the fixed point: hist ~ I2 / p makes q ~ I2 whatever p was, so two different starts land on one cdf (alpha = 1/2: p ~ sqrt(I2))
    i2 = rng.random(64) + 0.01
    a = capi.vegas_refine_discrete(c0.copy(), i2 / np.diff(c0), 0.5, 0.0)
    b = capi.vegas_refine_discrete(vegas.uniform_cdf(64), i2 * 64.0, 0.5, 0.0)
    assert np.abs(a - b).max() <= TOL
    assert np.abs(np.diff(a) - np.sqrt(i2) / np.sqrt(i2).sum()).max() <= TOL


def test_refine_matches_the_numpy_mirror(libfdg):
    rng = np.random.default_rng(12)
    for trial in range(300):
        n = int(rng.choice([2, 3, 7, 16, 64, 1024, BMAX]))
        c0 = vegas.uniform_cdf(n)
        if trial % 3 == 0:                                                  # probabilities that have been refined before
            c0 = capi.vegas_refine_discrete(c0, rng.random(n) ** 4, 1.0, 0.2)
        h = rng.random(n) ** int(rng.integers(1, 8)) * 10.0 ** rng.uniform(-3, 6)
        if trial % 2:                                                       # many empty bins
            h[rng.random(n) < rng.uniform(0.3, 0.95)] = 0.0
            h[int(rng.integers(n))] = 1.0
        alpha = float(rng.choice([0.25, 0.5, 1.0, 1.5, 2.0]))
        floor = float(rng.choice([0.01, 0.05, 0.5, 0.99]))
        c = capi.vegas_refine_discrete(c0.copy(), h, alpha, floor)
        what = (trial, n, alpha, floor)
        assert c[0] == 0.0 and c[n] == 1.0, what
        assert (np.diff(c) > 0).all(), what
        want = mirror_refine_discrete(c0, h, alpha, floor)
        assert np.abs(c - want).max() <= TOL, what + (np.abs(c - want).max(),)
        # floor > 0: every p'_j of step 4 is at least floor / n_bin.  The cdf holds their running sum: each of its entries is rounded to
        # half an ulp of 1 (2^-53), and the last one is then set to 1 exactly, which moves it by the drift of n roundings at the most
        assert (np.diff(c) >= floor / n - (n + 1) * 2.0 ** -53).all(), what


def test_refine_without_a_floor_refuses_an_empty_bin(libfdg):
    c0 = vegas.uniform_cdf(8)
    h = np.ones(8)
    h[3] = 0.0
    c = c0.copy()
    assert capi.lib().fdg_vegas_refine_discrete(c.ctypes.data, h.ctypes.data, 8, 0.5, 0.0) == capi.FDG_E_INTERNAL
    assert np.array_equal(c.view(np.uint64), c0.view(np.uint64))
    c = capi.vegas_refine_discrete(c0.copy(), h, 0.5, 0.08)
    p = np.diff(c)
    assert abs(p[3] - 0.01) <= TOL and (p > 0).all()


# ---- the Python side ---------------------------------------------------------------------------------------------------------------- #
def test_uniform_cdf_and_the_sampler_mirror():
    c = vegas.uniform_cdf(7)
    assert c.shape == (8,) and c[0] == 0.0 and c[7] == 1.0 and np.array_equal(c[:7], np.arange(7) / 7)
    assert np.array_equal(vegas.uniform_cdf(1), [0.0, 1.0])
    for bad in (0, BMAX + 1):
        with pytest.raises(ValueError):
            vegas.uniform_cdf(bad)
    grid = vegas.uniform_grid([0.0, -1.0], [1.0, 1.0], 4)
    x, jac, b, cell = mirror_sample_discrete(grid, c, 5, 77, 1000, bin_base=1)
    u = oracle.philox_uniform(1000, 3, 5, 77)
    assert ((c[b - 1] <= u[:, 2]) & (u[:, 2] < c[b])).all()                # the value whose interval holds the uniform of column D
    assert np.allclose(jac, 2.0 * 7.0, rtol=1e-14) and b.min() >= 1 and b.max() <= 7
    # one value: the continuous sampler's mirror, bit for bit
    x1, j1, b1, _ = mirror_sample_discrete(grid, vegas.uniform_cdf(1), 5, 77, 1000)
    x0, j0, _ = mirror_map(grid, oracle.philox_uniform(1000, 2, 5, 77))
    assert np.array_equal(x1.view(np.uint64), x0.view(np.uint64)) and np.array_equal(j1.view(np.uint64), j0.view(np.uint64)) and (b1 == 0).all()


def test_discrete_map_validates(libfdg):
    import torch
    ok = vegas.uniform_cdf(4)
    m = vegas.DiscreteMap(ok, ext=np.arange(8.0).reshape(4, 2), ext_col=[0, 2], device="cpu")
    assert m.n_bin == 4 and np.array_equal(m.prob, [0.25] * 4) and m.ext.shape == (4, 2) and m.d_cdf.dtype == torch.float64
    m.refine(np.array([1.0, 4.0, 9.0, 16.0]), 0.5, 0.0)
    assert np.abs(m.prob - np.array([1.0, 2.0, 3.0, 4.0]) / 10.0).max() <= TOL and np.array_equal(m.d_cdf.numpy(), m.cdf)
    keep = m.cdf.copy()
    with pytest.raises(capi.FdgError):
        m.refine(np.array([1.0, -4.0, 9.0, 16.0]))
    assert np.array_equal(m.cdf, keep) and np.array_equal(m.d_cdf.numpy(), keep)
    plain = vegas.DiscreteMap(ok, device="cpu")
    assert plain.ext is None and plain.d_ext is None and plain.ext_col == []
    for bad in (dict(cdf=[0.0, 0.5, 0.5, 1.0]), dict(cdf=[0.1, 0.5, 1.0]), dict(cdf=[0.0, 0.5, 0.9]), dict(cdf=[1.0]),
                dict(cdf=ok, ext=np.zeros((4, 2)), ext_col=[1, 1]), dict(cdf=ok, ext=np.zeros((3, 2)), ext_col=[0, 1]),
                dict(cdf=ok, ext=np.zeros((4, 2))), dict(cdf=ok, ext_col=[0]),
                dict(cdf=ok, ext=np.zeros((4, EMAX + 1)), ext_col=list(range(EMAX + 1)))):
        with pytest.raises(ValueError):
            vegas.DiscreteMap(device="cpu", **bad)
