"""Spherical momentum variables of VEGAS without a device (include/fdg.h: fdg_vegas_sample_device_polar, fdg_sincos; csrc/fdg_sincos.h;
feynmandiagram.jl_amd/vegas.py: PolarVar, ball, the keyword ``polar``): the two symbols are declared, exported and bound; fdg_sincos
carries the bits of a numpy restatement of the header's operation order, stays within 4 * 2^-53 of a sine and cosine of 64 mantissa
bits and gives s >= 0 on [0, fl(pi)]; every argument check of the sampler runs before any device work; the driver refuses what the
sampler's contract leaves to the caller.  The mirrors written here are what tests/test_vegas_polar_accumulate.py compares the device with."""
import math
import os
import re

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas
from feynmandiagram_jl_amd.lowering import lower
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_vegas_discrete_host import mirror_sample_discrete
from test_vegas_host import mirror_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "feynmandiagram.jl_amd", "julia", "hip_compiler.jl")
NAMES = ("fdg_vegas_sample_device_polar", "fdg_sincos")
FAKE, FAKE2, FAKE3, FAKE4, FAKE5 = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # only compared with NULL; never read through
DMAX, GMAX, BMAX, EMAX, PMAX = (capi.FDG_VEGAS_DIM_MAX, capi.FDG_VEGAS_GRID_MAX, capi.FDG_BIN_MAX, capi.FDG_VEGAS_EXT_MAX,
                                capi.FDG_VEGAS_POLAR_MAX)
PI = np.float64(math.pi)
UNIT = 2.0 ** -53


# ---- numpy mirrors ------------------------------------------------------------------------------------------------------------------ #
TWO_OVER_PI, P1, P1T = np.float64(0.6366197723675814), np.float64(1.5707963267341256), np.float64(6.077100506506192e-11)
S = [np.float64(v) for v in (-0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06,
                             -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15)]       # S1 .. S8
CC = [np.float64(v) for v in (0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
                              2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14)]                                  # C2 .. C8


def mirror_sincos(x):
    """(s, c) of csrc/fdg_sincos.h for an array of doubles in [0, 2 pi]: the header's operations, one numpy operation each, in its order"""
    x = np.asarray(x, dtype=np.float64)
    fn = x * TWO_OVER_PI
    fn = fn + 0.5
    q = fn.astype(np.int64)
    qd = q.astype(np.float64)
    r = x - qd * P1
    t = qd * P1T
    r = r - t
    z = r * r
    ps = np.full_like(z, S[7])
    for k in range(6, -1, -1):
        ps = ps * z
        ps = ps + S[k]
    sn = r * z
    sn = sn * ps
    sn = r + sn
    pc = np.full_like(z, CC[6])
    for k in range(5, -1, -1):
        pc = pc * z
        pc = pc + CC[k]
    h = 0.5 * z
    w = z * z
    w = w * pc
    h = h - w
    cs = 1.0 - h
    odd = (q & 1) != 0
    s = np.where(odd, cs, sn)
    c = np.where(odd, sn, cs)
    s = np.where((q & 2) != 0, -s, s)
    c = np.where(((q + 1) & 2) != 0, -c, c)
    return s, c


def mirror_sample_polar(grid, col, polar, seed, sample_offset, n_sample, n_col, cdf=None, ext=None, ext_col=(), bin_base=0, fill=-77.0):
    """(x [B, n_col], jac [B], bin [B] or None, cell [B, D]) of fdg_vegas_sample_device_polar: the variables through mirror_map (or
    mirror_sample_discrete, whose jacobian is divided by p afterwards -- so the fold is redone here in the header's order), the groups
    ``(var, cols)`` in the order of the list, columns nobody names = ``fill``."""
    D = grid.shape[0]
    if cdf is None:
        v, jc, cell = mirror_map(grid, oracle.philox_uniform(n_sample, D, seed, sample_offset))
        b = None
    else:
        v, _, b, cell = mirror_sample_discrete(grid, cdf, seed, sample_offset, n_sample, bin_base)
        _, jc, _ = mirror_map(grid, oracle.philox_uniform(n_sample, D, seed, sample_offset))
    x = np.full((n_sample, n_col), fill)
    grouped = {d for var, cols in polar for d in range(var, var + len(cols))}
    for d in range(D):
        if d not in grouped:
            x[:, col[d]] = v[:, d]
    for var, cols in polar:
        k = v[:, var]
        if len(cols) == 3:
            st, ct = mirror_sincos(v[:, var + 1])
            sp, cp = mirror_sincos(v[:, var + 2])
            ks = k * st
            x[:, cols[0]], x[:, cols[1]], x[:, cols[2]] = ks * cp, ks * sp, k * ct
            jc = jc * k
            jc = jc * k
            jc = jc * st
        else:
            sp, cp = mirror_sincos(v[:, var + 1])
            x[:, cols[0]], x[:, cols[1]] = k * cp, k * sp
            jc = jc * k
    if cdf is not None:
        j = b - bin_base
        jc = jc / (cdf[j + 1] - cdf[j])
        if ext is not None:
            for i, e in enumerate(ext_col):
                x[:, e] = ext[j, i]
    return x, jc, b, cell


def sincos_points():
    """1e5 Philox-drawn values in [0, 2 pi], and 0, fl(pi/4), fl(pi/2), fl(pi), fl(3 pi/2), fl(2 pi) with their neighbours inside the domain
    (which includes the double above fl(2 pi))"""
    u = oracle.philox_uniform(100_000, 1, 20_240_607)[:, 0] * (2.0 * PI)
    exact = np.array([0.0, PI / 4, PI / 2, PI, 3 * PI / 2, 2 * PI])
    pts = np.concatenate([u, exact, np.nextafter(exact, np.inf), np.nextafter(exact[1:], -np.inf)])
    assert pts.min() == 0.0 and pts.max() == np.nextafter(2 * PI, np.inf)
    return pts


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
    for fn in ("vegas_sample_device_polar!", "fdg_sincos"):
        assert fn in [x.strip() for x in export.split(",")], fn
    hdr = open(os.path.join(ROOT, "include", "fdg.h")).read()
    assert re.search(r"#define\s+FDG_VEGAS_POLAR_MAX\s+(\d+)", hdr).group(1) == str(PMAX) == "21"
    assert re.search(r"typedef struct fdg_vegas_polar \{ uint32_t var, dim, col\[3\]; \} fdg_vegas_polar;", hdr)
    import ctypes
    assert ctypes.sizeof(capi.VegasPolar) == 20
    assert fd.PolarVar is vegas.PolarVar and fd.ball is vegas.ball
    assert callable(capi.vegas_sample_device_polar) and callable(capi.sincos)


# ---- fdg_sincos --------------------------------------------------------------------------------------------------------------------- #
def test_sincos_matches_the_numpy_restatement_bit_for_bit(libfdg):
    pts = sincos_points()
    got = np.array([capi.sincos(v) for v in pts])
    ws, wc = mirror_sincos(pts)
    assert np.array_equal(got[:, 0].view(np.uint64), ws.view(np.uint64)), pts[got[:, 0].view(np.uint64) != ws.view(np.uint64)][:4]
    assert np.array_equal(got[:, 1].view(np.uint64), wc.view(np.uint64)), pts[got[:, 1].view(np.uint64) != wc.view(np.uint64)][:4]
    assert capi.sincos(0.0) == (0.0, 1.0)


def test_sincos_accuracy_and_sign(libfdg):
    """|s - sin x| and |c - cos x| <= 4 * 2^-53 against the long double sine and cosine (64 mantissa bits), the bound OpenCL sets for a
    conforming double sin / cos; s >= 0 on [0, fl(pi)].  Reached over these points: 1.24 and 1.07 units of 2^-53."""
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs at least 63 mantissa bits"
    pts = sincos_points()
    got = np.array([capi.sincos(v) for v in pts])
    lx = pts.astype(np.longdouble)
    es = np.abs(got[:, 0].astype(np.longdouble) - np.sin(lx)).astype(np.float64)
    ec = np.abs(got[:, 1].astype(np.longdouble) - np.cos(lx)).astype(np.float64)
    print("fdg_sincos: max |s - sin| =", es.max() / UNIT, "x 2^-53 at", pts[es.argmax()], "; max |c - cos| =", ec.max() / UNIT, "x 2^-53 at",
          pts[ec.argmax()])
    assert es.max() <= 4 * UNIT and ec.max() <= 4 * UNIT
    low = pts <= PI
    assert low.sum() > 40_000 and (got[low, 0] >= 0.0).all()
    s_pi, c_pi = capi.sincos(float(PI))
    assert 0.0 < s_pi < 2e-16 and c_pi == -1.0                              # fl(pi) lies below pi: its sine is +1.22e-16


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def _u32(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.uint32)


def _groups(polar):
    arr = (capi.VegasPolar * max(len(polar), 1))()
    for g, (var, dim, cols) in enumerate(polar):
        arr[g].var, arr[g].dim = var, dim
        for i, c in enumerate(cols):
            arr[g].col[i] = c
    return arr


def _sample(n_dim=6, n_grid=8, col=None, d_grid=FAKE, d_cdf=None, n_bin=5, d_ext=None, ext_col=None, n_ext=None, polar=((0, 3, (0, 1, 2)),),
            n_polar=None, null_polar=False, d_x=FAKE2, d_jac=FAKE3, d_bin=None, B=100):
    """polar: (var, dim, cols) triples, passed as they are (the checks are the library's)"""
    c, e = _u32(col), _u32(ext_col)
    n_ext = (0 if e is None else e.shape[0]) if n_ext is None else n_ext
    arr = _groups(polar)
    import ctypes
    return capi.lib().fdg_vegas_sample_device_polar(d_grid, n_dim, n_grid, None if c is None else c.ctypes.data, d_cdf, n_bin, 0, d_ext, n_ext,
                                                    None if e is None else e.ctypes.data, None if null_polar else ctypes.addressof(arr),
                                                    len(polar) if n_polar is None else n_polar, 1, 0, d_x, 1, 100, d_jac, d_bin, None, B, None)


def test_sampler_argument_checks_need_no_device(libfdg):
    INV, UNS, OK = capi.FDG_E_INVALID, capi.FDG_E_UNSUPPORTED, capi.FDG_OK
    assert _sample(B=0) == OK                                              # valid and nothing to do: no device work
    # the existing calls' own cases
    for name in ("d_grid", "d_x", "d_jac"):
        assert _sample(**{name: None}) == INV, name
    assert _sample(B=-1) == INV
    assert _sample(n_dim=0) == INV and _sample(n_grid=0) == INV
    assert _sample(n_dim=DMAX + 1) == UNS and _sample(n_grid=GMAX + 1) == UNS
    assert _sample(n_dim=DMAX, n_grid=GMAX, B=0) == OK
    # no discrete variable: n_bin, d_bin, d_ext, ext_col are ignored
    assert _sample(n_bin=0, B=0) == OK and _sample(n_bin=BMAX + 1, B=0) == OK and _sample(n_ext=EMAX + 1, B=0) == OK
    assert _sample(ext_col=[0, 0], B=0) == OK
    # with one: the discrete call's cases
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, B=0) == OK
    assert _sample(d_cdf=FAKE4, d_bin=None) == INV
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, n_bin=0) == INV
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, n_bin=BMAX + 1) == UNS
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, d_ext=FAKE, ext_col=list(range(6, 7 + EMAX))) == UNS
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, d_ext=None, ext_col=[6, 7]) == INV
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, d_ext=FAKE, ext_col=None, n_ext=2) == INV
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, d_ext=FAKE, ext_col=[6, 7, 6]) == INV
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, d_ext=FAKE, ext_col=[6, 5]) == INV      # a column of the ungrouped variable 5
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, d_ext=FAKE, ext_col=[6, 1]) == INV      # a column of the group
    assert _sample(d_cdf=FAKE4, d_bin=FAKE5, d_ext=FAKE, ext_col=[6, 7], B=0) == OK
    # the groups
    assert _sample(null_polar=True) == INV                                 # polar == NULL with n_polar > 0
    assert _sample(null_polar=True, n_polar=0, B=0) == OK
    assert _sample(polar=(), B=0) == OK
    for dim in (0, 1, 4, 2 ** 31):
        assert _sample(polar=((0, dim, (0, 1, 2)),)) == INV, dim
    assert _sample(polar=((4, 3, (0, 1, 2)),)) == INV                      # var + dim > n_dim
    assert _sample(polar=((5, 2, (0, 1)),)) == INV
    assert _sample(polar=((6, 2, (0, 1)),)) == INV
    assert _sample(polar=((2 ** 32 - 1, 2, (0, 1)),)) == INV               # var + dim wraps around
    assert _sample(polar=((3, 3, (0, 1, 2)),), col=[3, 4, 5, 0, 0, 0], B=0) == OK
    assert _sample(polar=((4, 2, (0, 1)),), col=[2, 3, 4, 5, 0, 0], B=0) == OK
    assert _sample(polar=((0, 3, (0, 1, 2)), (2, 2, (6, 7)))) == INV      # two groups share variable 2
    assert _sample(polar=((0, 3, (0, 1, 2)), (0, 3, (6, 7, 8)))) == INV
    assert _sample(polar=((0, 3, (6, 7, 8)), (3, 3, (9, 10, 11))), B=0) == OK
    assert _sample(polar=((0, 3, (6, 7, 6)),)) == INV                      # a column written twice: inside a group,
    assert _sample(polar=((0, 3, (6, 7, 8)), (3, 3, (9, 8, 11)))) == INV   # by two groups,
    assert _sample(polar=((0, 3, (6, 7, 4)),)) == INV                      # by a group and the ungrouped variable 4 (col NULL: col[d] = d),
    assert _sample(polar=((0, 3, (6, 7, 8)),), col=[0, 0, 0, 1, 2, 2]) == INV   # by two ungrouped variables;
    assert _sample(polar=((0, 3, (6, 7, 8)),), col=[9, 9, 9, 1, 2, 3], B=0) == OK   # the col of a grouped variable is not read
    assert _sample(polar=((0, 2, (6, 7, 7)),), B=0) == OK                  # nor col[2] of a group of two
    many = tuple((3 * g, 3, (3 * g, 3 * g + 1, 3 * g + 2)) for g in range(PMAX))
    assert _sample(n_dim=DMAX, polar=many, B=0) == OK
    assert _sample(n_dim=DMAX, polar=many + ((63, 2, (70, 71)),)) == UNS   # n_polar > FDG_VEGAS_POLAR_MAX
    assert _sample(n_dim=DMAX, polar=many, n_polar=PMAX + 1) == UNS
    with pytest.raises(capi.FdgError) as e:
        capi.vegas_sample_device_polar(FAKE, 6, 8, None, 0, 1, 0, 0, None, [(0, (0, 1, 2)), (2, (6, 7))], 1, 0, FAKE2, 1, 100, FAKE3, 0, 0, 100)
    assert e.value.code == INV
    with pytest.raises(capi.FdgError) as e:
        capi.vegas_sample_device_polar(FAKE, 6, GMAX + 1, None, 0, 1, 0, 0, None, [(0, (0, 1, 2))], 1, 0, FAKE2, 1, 100, FAKE3, 0, 0, 100)
    assert e.value.code == UNS
    with pytest.raises(ValueError):
        capi.vegas_sample_device_polar(FAKE, 6, 8, [0, 1], 0, 1, 0, 0, None, [(0, (0, 1, 2))], 1, 0, FAKE2, 1, 100, FAKE3, 0, 0, 100)
    with pytest.raises(ValueError):
        capi.vegas_sample_device_polar(FAKE, 6, 8, None, 0, 1, 0, 0, None, [(0, (0, 1, 2, 3))], 1, 0, FAKE2, 1, 100, FAKE3, 0, 0, 100)
    capi.vegas_sample_device_polar(FAKE, 6, 8, [None, None, None, 3, 4, 5], 0, 1, 0, 0, None, [(0, (0, 1, 2))], 1, 0, FAKE2, 1, 100, FAKE3, 0, 0, 0)


# ---- the Python side ---------------------------------------------------------------------------------------------------------------- #
def test_ball_and_the_sampler_mirror():
    lo, hi = vegas.ball(2.5, 3)
    assert lo == [0.0, 0.0, 0.0] and hi == [2.5, math.pi, 2.0 * math.pi]
    lo, hi = vegas.ball(2.5, 2, k_min=0.5)
    assert lo == [0.5, 0.0] and hi == [2.5, 2.0 * math.pi]
    for bad in (dict(k_max=1.0, dim=1), dict(k_max=1.0, dim=4), dict(k_max=0.0), dict(k_max=-1.0), dict(k_max=1.0, k_min=-0.1),
                dict(k_max=1.0, k_min=1.0), dict(k_max=float("inf"))):
        with pytest.raises(ValueError):
            vegas.ball(**bad)
    # the mirror: no groups = mirror_map in the named columns; a group = |x| is k and the weight carries k^2 sin(theta)
    lo, hi = vegas.ball(2.0, 3)
    grid = vegas.uniform_grid(lo + [-1.0], hi + [1.0], 16)
    x0, j0, b0, c0 = mirror_sample_polar(grid, [3, 2, 1, 0], [], 5, 77, 1000, 5)
    v, jm, cm = mirror_map(grid, oracle.philox_uniform(1000, 4, 5, 77))
    assert b0 is None and np.array_equal(x0[:, [3, 2, 1, 0]], v) and np.array_equal(j0, jm) and np.array_equal(c0, cm) and (x0[:, 4] == -77.0).all()
    x1, j1, _, c1 = mirror_sample_polar(grid, [None, None, None, 0], [(0, (4, 2, 3))], 5, 77, 1000, 5)
    assert np.array_equal(c1, cm) and np.array_equal(x1[:, 0], v[:, 3]) and (x1[:, 1] == -77.0).all()
    assert np.allclose(np.sqrt((x1[:, [4, 2, 3]] ** 2).sum(axis=1)), v[:, 0], rtol=1e-14)
    assert np.allclose(x1[:, 3], v[:, 0] * np.cos(v[:, 1]), rtol=1e-13, atol=1e-15)
    assert np.allclose(j1, jm * v[:, 0] ** 2 * np.sin(v[:, 1]), rtol=1e-13)
    # with the discrete variable: its mirror's jacobian, times the group's factors (up to the order of the operations)
    cdf = vegas.uniform_cdf(7)
    ext = np.arange(14.0).reshape(7, 2)
    x2, j2, b2, _ = mirror_sample_polar(grid, [None, None, None, 0], [(0, (4, 2, 3))], 5, 77, 1000, 7, cdf=cdf, ext=ext, ext_col=[5, 6], bin_base=1)
    _, jd, bd, _ = mirror_sample_discrete(grid, cdf, 5, 77, 1000, 1)
    assert np.array_equal(b2, bd) and np.array_equal(x2[:, :5], x1) and np.array_equal(x2[:, 5:], ext[bd - 1])
    assert np.allclose(j2, jd * v[:, 0] ** 2 * np.sin(v[:, 1]), rtol=1e-13)


def _one_leaf():
    """a handle and the tables of one bosonic leaf on K_1 + K_2 (columns 0-2 K_1, 3-5 K_2, 6 the one time); nothing touches a device"""
    a = fd.Graph([])
    t, _, _ = lower([fd.Graph([a], subgraph_factors=[1.0])])
    tab, keep = capi.make_leaf_tables([2], [2], [1], [1], [1], np.array([[1.0, 1.0]]), 3, 1)
    return capi.GraphHandle(t), tab, keep


def test_the_driver_refuses_what_the_sampler_leaves_to_the_caller(libfdg):
    h, tab, _keep = _one_leaf()
    P = vegas.PolarVar
    lo, hi = vegas.ball(2.0, 3)
    kw = dict(n_iter=1, n_sample=100, n_grid=8, device="cpu", specialize_fused=False)

    def run(lo, hi, col, polar, **more):
        return vegas.vegas_integrate(h, tab, lo, hi, col, 0.0, 1.0, 0.05, polar=polar, **dict(kw, **more))

    def run_binned(lo, hi, col, polar):
        dm = vegas.DiscreteMap(vegas.uniform_cdf(4), ext=np.zeros((4, 3)), ext_col=[0, 1, 2], device="cpu")
        return vegas.vegas_integrate_binned(h, tab, lo, hi, col, dm, 0.0, 1.0, 0.05, polar=polar, **kw)

    eps = 1e-9
    bad = [
        ([-0.1, 0.0, 0.0], hi, [None] * 3, [P(0, (3, 4, 5))]),                                  # a negative k_lo
        ([0.0, -eps, 0.0], hi, [None] * 3, [P(0, (3, 4, 5))]),                                  # theta below 0
        (lo, [2.0, math.pi + eps, 2 * math.pi], [None] * 3, [P(0, (3, 4, 5))]),                 # theta beyond pi
        (lo, [2.0, math.pi, 2 * math.pi + eps], [None] * 3, [P(0, (3, 4, 5))]),                 # phi beyond 2 pi
        ([0.0, -eps], [2.0, 1.0], [None] * 2, [P(0, (3, 4))]),                                  # 2D: phi below 0
        ([0.0, 0.0], [2.0, 2 * math.pi + eps], [None] * 2, [P(0, (3, 4))]),                     # 2D: phi beyond 2 pi
        (lo, hi, [None, 0, None], [P(0, (3, 4, 5))]),                                           # a grouped variable with a column
        (lo, hi, [3, 4, 5], [P(0, (3, 4, 5))]),
        (lo + lo[:2], hi + [2.0, 1.0], [None] * 5, [P(0, (3, 4, 5)), P(2, (0, 1))]),            # overlapping groups
        (lo + lo, hi + hi, [None] * 6, [P(0, (3, 4, 5)), P(1, (0, 1, 2))]),
        (lo, hi, [None] * 3, [P(1, (3, 4, 5))]),                                                # a group that reaches past the map
        (lo, hi, [None] * 3, [P(0, (3, 4, 5, 6))]),                                             # four columns
        (lo, hi, [None] * 3, [P(0, (3, 4, 7))]),                                                # a column x does not have
        (lo, hi, [None] * 3, [P(0, (3, 4, 4))]),                                                # a column twice
        (lo + [0.0], hi + [1.0], [None, None, None, 4], [P(0, (3, 4, 5))]),                     # ... by a group and a plain variable
        (lo + [0.0], hi + [1.0], [None] * 4, [P(0, (3, 4, 5))]),                                # an ungrouped variable without a column
    ]
    for case in bad:
        with pytest.raises(ValueError):
            run(*case)
        with pytest.raises(ValueError):
            run_binned(*case)
    with pytest.raises(ValueError):
        run_binned(lo, hi, [None] * 3, [P(0, (2, 3, 4))])                                       # a column of the discrete variable's table
    # the check applies equally to a map passed in
    vm = vegas.VegasMap(vegas.uniform_grid(lo, [2.0, 3.2, 6.0], 8), "cpu")
    with pytest.raises(ValueError):
        run(None, None, [None] * 3, [P(0, (3, 4, 5))], vmap=vm)
    # without groups a column of None is an error as it always was
    with pytest.raises((TypeError, ValueError)):
        run(lo, hi, [None] * 3, None)
