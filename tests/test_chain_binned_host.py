"""The Markov chain with a discrete external variable and per-bin measurement, without a device (include/fdg.h:
fdg_chain_propose_device_discrete, fdg_chain_step_device_binned, fdg_mc_chain_step_device_binned; feynmandiagram.jl_amd/vegas.py:
chain_integrate_binned): the symbols are declared, exported and bound, the numpy mirror (capi.chain_binned_reference: what
tests/test_chain_binned_accumulate.py compares the device with) ties to the grouped mirror bit for bit where the discrete variable has
one value, and the mirror of the whole driver meets on the CPU the statistical conditions of the known answer.

The known answer (leaf form, sign-changing).  Leaves x, y, the constant c = 1 and e over the unit square; e is written from the
discrete variable's table ext = (0.5, 1, 2, 3), whose values are drawn with p = (0.1, 0.2, 0.3, 0.4):
    r_0 = (x - 0.3 c)(c - y)^3 e     exact 0.05 e_j
    r_1 = x y e^2                    exact 0.25 e_j^2
4096 walkers, 48 steps with 16 discarded, moves [all + discrete, x, y, discrete], gamma_rel = 1, the uniform map."""
import functools
import math
import re

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT
from test_chain_groups_host import GROUPS3, IDENTITY_STEPS, host_random_case
from test_chain_host import CHI2_HI, CHI2_LO, INIT, MEASURE, fresh_state, oracle_roots, philox_columns, step_uniforms
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_matsubara_accumulate import phase_table
from test_vegas_host import JL

NAMES = ("fdg_chain_propose_device_discrete", "fdg_chain_step_device_binned", "fdg_mc_chain_step_device_binned")
KNOWN_B = dict(n_walker=4096, n_step=48, n_therm=16, gamma_rel=1.0, n_grid=8, n_seed=32, moves=(7, 1, 2, 4), ext=(0.5, 1.0, 2.0, 3.0),
               p=(0.1, 0.2, 0.3, 0.4))
KNOWN_B["exact"] = np.array([[0.05 * e, 0.25 * e * e] for e in KNOWN_B["ext"]])


def cdf_of(p):
    """the cdf of the probabilities ``p``: running sums from 0, the last entry exactly 1"""
    c = np.concatenate([[0.0], np.cumsum(np.asarray(p, dtype=np.float64))])
    assert abs(c[-1] - 1.0) < 1e-12
    c[-1] = 1.0
    return c


def fresh_binned_state(fixed, D, R, B, n_bin, n_freq=0):
    st = fresh_state(fixed, D, R, B)
    st["fac"] = np.ones((D + 1, B))
    st["bin"] = np.zeros(B, dtype=np.int32)
    st["sum"] = np.zeros((n_bin * (2 * n_freq * R if n_freq else R) + 1, B))
    return st


def binned_uniforms(B, D, mask, seed, off):
    """``(u [B, D], u_acc [B], u_disc [B])`` of one step; bit ``D`` of ``mask`` is the discrete variable's (Philox column ``D``)"""
    u, ua = step_uniforms(B, D, mask & ((1 << D) - 1), seed, off)
    ud = philox_columns(B, [D], seed, off)[:, 0] if (mask >> D) & 1 else None
    return u, ua, ud


def mirror_binned_step(st, grid, col, mask, seed, off, gamma, flags, ev, cdf, ext, ext_col, groups=None, reweight=None, mz=None, coef=None,
                       exists=None):
    D = grid.shape[0]
    u, ua, ud = binned_uniforms(st["x"].shape[1], D, mask, seed, off)
    g = groups or dict(root_group=None, var_sets=None)
    return capi.chain_binned_reference(grid, col, st, mask & ((1 << D) - 1), u, ua, gamma, flags, ev, cdf, ext, ext_col, bool((mask >> D) & 1), ud,
                                       g["root_group"], g["var_sets"], reweight, coef, exists, mz, phase_table)


def mirror_chain_binned(eval_roots, grid, col, fixed, R, cdf, ext, ext_col, *, n_walker, n_step, n_therm, moves=None, gamma=None,
                        gamma_rel=1.0, seed=0, coef=None, exists=None):
    """vegas.chain_integrate_binned without groups and without a warm-up, on the CPU: INIT with every variable and the discrete one
    drawn, gamma, the steps, the reduction, chain_estimate (tests/test_chain_host.py: mirror_chain)"""
    grid = np.asarray(grid, dtype=np.float64)
    D, B, n_bin = grid.shape[0], int(n_walker), len(cdf) - 1
    moves = vegas.chain_moves(D + 1) if moves is None else list(moves)
    st = fresh_binned_state(fixed, D, R, B, n_bin)
    st = mirror_binned_step(st, grid, col, (1 << (D + 1)) - 1, seed, 0, 1.0, INIT, eval_roots, cdf, ext, ext_col, coef=coef, exists=exists)
    if gamma is None:
        gamma = gamma_rel * float(st["a"].sum()) / B
    st["n_accept"][:] = 0
    for t in range(n_step):
        st = mirror_binned_step(st, grid, col, moves[t % len(moves)], seed, (t + 1) * B, gamma, MEASURE if t >= n_therm else 0, eval_roots, cdf,
                                ext, ext_col, coef=coef, exists=exists)
    Cs = n_bin * R
    red = capi.chain_reduce_reference(st["sum"])
    S, Q, X = red[:Cs + 1], red[Cs + 1:2 * Cs + 2], red[2 * Cs + 2:]
    mean, err = vegas.chain_estimate(S, Q, X, B)
    return dict(mean=mean.reshape(n_bin, R), stderr=err.reshape(n_bin, R), acceptance=float(st["n_accept"].sum()) / (B * n_step), gamma=gamma,
                state=st)


@functools.lru_cache(maxsize=None)
def known_b_graph():
    """(table, [leaf of x, leaf of y], leaf of e, fixed leaf values) of the known answer"""
    x, y, c, e = fd.Graph([]), fd.Graph([]), fd.Graph([]), fd.Graph([])
    a = fd.Graph([x, c], subgraph_factors=[1.0, -0.3], operator=fd.Sum())
    cube = fd.Graph([fd.Graph([c, y], subgraph_factors=[1.0, -1.0], operator=fd.Sum())], operator=fd.Power(3))
    r0 = fd.Graph([a, cube, e], operator=fd.Prod())
    r1 = fd.Graph([x, y, fd.Graph([e], operator=fd.Power(2))], operator=fd.Prod())
    t, leafmap, _ = lower([r0, r1])
    at = {g.id: i - 1 for i, g in leafmap.items()}
    assert t.n_leaf == 4 and t.n_root == 2 and all(int(s) != FDG_NO_ROOT for s in t.root_slot)
    fixed = np.zeros(4)
    fixed[at[c.id]] = 1.0
    return t, [at[x.id], at[y.id]], at[e.id], fixed


def known_b_mirror(seed):
    t, col, ecol, fixed = known_b_graph()
    k = KNOWN_B
    return mirror_chain_binned(oracle_roots(t), vegas.uniform_grid([0, 0], [1, 1], k["n_grid"]), col, fixed, 2, cdf_of(k["p"]),
                               np.array(k["ext"])[:, None], [ecol], n_walker=k["n_walker"], n_step=k["n_step"], n_therm=k["n_therm"],
                               moves=k["moves"], gamma_rel=k["gamma_rel"], seed=seed)


def test_known_b_graph_is_the_two_polynomials():
    t, col, ecol, fixed = known_b_graph()
    rng = np.random.default_rng(0)
    xp = np.repeat(fixed[:, None], 50, axis=1)
    xp[col[0]], xp[col[1]], xp[ecol] = rng.random(50), rng.random(50), rng.choice(KNOWN_B["ext"], size=50)
    x, y, e = xp[col[0]], xp[col[1]], xp[ecol]
    got = oracle_roots(t)(xp)
    assert np.allclose(got[0], (x - 0.3) * (1 - y) ** 3 * e, rtol=1e-13, atol=1e-16) and np.allclose(got[1], x * y * e * e, rtol=1e-14)


def test_known_answer_on_the_mirror(libfdg):
    """The sum over seeds 0 .. 31 of ((mean - exact) / sigma)^2 lies inside [10.3, 70.6], the 1e-4 and 1 - 1e-4 quantiles of chi^2
    with 32 degrees of freedom, for each of the 8 (bin, root) pairs."""
    chi2, first = np.zeros((4, 2)), None
    for seed in range(KNOWN_B["n_seed"]):
        r = known_b_mirror(seed)
        first = first or r
        chi2 += ((r["mean"] - KNOWN_B["exact"]) / r["stderr"]) ** 2
    print("seed 0: mean", first["mean"], "stderr", first["stderr"], "acceptance", first["acceptance"], "gamma", first["gamma"])
    print("chi2 over 32 seeds", chi2)
    assert ((CHI2_LO <= chi2) & (chi2 <= CHI2_HI)).all()
    assert (np.abs(first["mean"] - KNOWN_B["exact"]) <= 5.0 * first["stderr"]).all()
    assert 0.3 < first["acceptance"] < 1.0
    visits = np.bincount(first["state"]["bin"], minlength=4)
    assert (visits > 0).all()                                   # every value is occupied at the end of the run


# ---- mirror identities ------------------------------------------------------------------------------------------------------------------ #
CDF3 = cdf_of((0.5, 0.125, 0.375))
EXT3 = np.array([[0.3, -0.8], [-0.1, 0.6], [0.9, 0.2]])
ECOL3 = [1, 6]                                              # two of the random case's leaves that are no variables
BINNED_STEPS = [(0b1111, INIT), (0b1111, 0), (0b0010, MEASURE), (0b1000, MEASURE), (0, MEASURE), (0b1111, MEASURE), (0b1001, MEASURE),
                (0b0101, MEASURE)]                          # INIT and 7 steps; bit 3 is the discrete variable


def test_doubling_reweight_and_gamma_halves_every_sum(libfdg):
    """reweight and gamma both doubled: x, fac, bin, root and n_accept identical, a exactly doubled, sum exactly halved"""
    t, col, fixed, grid, coef, exists = host_random_case()
    B, R, D, seed, gamma = 70, t.n_root, 3, 5, 0.21
    rho = np.array([0.7, 1.9, 3.3])
    ev = oracle_roots(t)
    one, two = fresh_binned_state(fixed, D, R, B, 3), fresh_binned_state(fixed, D, R, B, 3)
    for i, (mask, flags) in enumerate(BINNED_STEPS):
        one = mirror_binned_step(one, grid, col, mask, seed, i * B, gamma, flags, ev, CDF3, EXT3, ECOL3, GROUPS3, rho, None, coef, exists)
        two = mirror_binned_step(two, grid, col, mask, seed, i * B, 2.0 * gamma, flags, ev, CDF3, EXT3, ECOL3, GROUPS3, 2.0 * rho, None, coef,
                                 exists)
        for k in ("x", "fac", "bin", "root", "n_accept"):
            assert np.array_equal(one[k], two[k]), (i, k)
        assert np.array_equal(two["a"], 2.0 * one["a"]) and np.array_equal(two["sum"], 0.5 * one["sum"]), i
    assert 0 < (one["n_accept"] < len(BINNED_STEPS)).sum() and np.abs(one["sum"]).max() > 0.0
    assert set(one["bin"]) == {0, 1, 2}
    assert np.array_equal(one["fac"][D], 1.0 / (CDF3[one["bin"] + 1] - CDF3[one["bin"]]))
    assert np.array_equal(one["x"][ECOL3], EXT3[one["bin"]].T)                    # the table's row of the walker's value
    assert (one["sum"][[3, R + 3, 2 * R + 3]] == 0.0).all()                        # the root that does not exist, in every bin


@pytest.mark.parametrize("projected", [False, True])
def test_one_value_is_the_grouped_mirror(libfdg, projected):
    """n_bin = 1, cdf = {0, 1}, no table: fd = 1.0, and x, fac rows 0 .. D - 1, root, a, sum and n_accept are the grouped mirror's bit
    for bit over INIT and 7 steps, whether or not the discrete variable is redrawn"""
    t, col, fixed, grid, coef, exists = host_random_case()
    B, R, D, seed, gamma = 70, t.n_root, 3, 3, 0.37
    rng = np.random.default_rng(17)
    mz = None
    if projected:
        mz = dict(freq=(2, -1, 0), fermionic=True, weight_freq=1, root_col_in=[int(v) for v in rng.integers(0, t.n_leaf, size=R)],
                  root_col_out=[int(v) for v in rng.integers(0, t.n_leaf, size=R)], beta=1.7)
    rho = np.array([0.7, 1.9, 3.3])
    ev = oracle_roots(t)
    grp, one = fresh_state(fixed, D, R, B), fresh_binned_state(fixed, D, R, B, 1, 3 if projected else 0)
    grp["sum"] = np.zeros_like(one["sum"])
    for i, (mask, flags) in enumerate(BINNED_STEPS):
        u, ua = step_uniforms(B, D, mask & 7, seed, i * B)
        grp = capi.chain_grouped_reference(grid, col, grp, mask & 7, u, ua, gamma, flags, ev, GROUPS3["root_group"], GROUPS3["var_sets"], rho,
                                           coef, exists, mz, phase_table)
        one = mirror_binned_step(one, grid, col, mask, seed, i * B, gamma, flags, ev, np.array([0.0, 1.0]), None, [], GROUPS3, rho, mz, coef,
                                 exists)
        for k in ("x", "root", "a", "sum", "n_accept", "xp"):
            assert np.array_equal(grp[k].view(np.uint8), one[k].view(np.uint8)), (i, k)
        assert np.array_equal(grp["fac"].view(np.uint8), one["fac"][:D].view(np.uint8)) and (one["fac"][D] == 1.0).all(), i
        assert (one["bin"] == 0).all()
    assert 0 < (grp["n_accept"] < len(BINNED_STEPS)).sum() and np.abs(grp["sum"][:-1]).max() > 0.0


def test_null_groups_are_one_group_of_everything(libfdg):
    """root_group and var_sets None (a NULL cg): the same bits as one group holding every root and every variable"""
    t, col, fixed, grid, coef, exists = host_random_case()
    B, R, D, seed, gamma = 70, t.n_root, 3, 3, 0.37
    ev = oracle_roots(t)
    a, b = fresh_binned_state(fixed, D, R, B, 3), fresh_binned_state(fixed, D, R, B, 3)
    for i, (mask, flags) in enumerate(BINNED_STEPS):
        a = mirror_binned_step(a, grid, col, mask, seed, i * B, gamma, flags, ev, CDF3, EXT3, ECOL3, None, None, None, coef, exists)
        b = mirror_binned_step(b, grid, col, mask, seed, i * B, gamma, flags, ev, CDF3, EXT3, ECOL3, dict(root_group=[0] * R, var_sets=[(0, 1, 2)]),
                               None, None, coef, exists)
        for k in ("x", "fac", "bin", "root", "a", "sum", "n_accept"):
            assert np.array_equal(a[k], b[k]), (i, k)
    with pytest.raises(ValueError):
        capi.chain_binned_reference(grid, col, dict(a, fac=a["fac"][:D]), 1, None, None, gamma, 0, ev, CDF3)        # fac without row D


# ---- declared, exported, bound -------------------------------------------------------------------------------------------------------- #
def test_symbols_are_declared_exported_and_bound(libfdg):
    protos = c_prototypes()
    calls = {c[0]: c for c in jl_ccalls()}
    export = [x.strip() for line in re.findall(r"^export\s+([^\n]*)", open(JL).read(), flags=re.M) for x in line.split(",")]
    for name in NAMES:
        assert name in protos and name in capi.EXPORTS and hasattr(libfdg, name), name
        assert name in calls, name + ": not bound in the Julia shim"
        _, _, types, args = calls[name]
        params = protos[name][1]
        assert len(types) == len(params) == len(args) == len(getattr(libfdg, name).argtypes), name
        for jt, cp in zip(types, params):
            assert jl_class(jt) == c_class(cp), (name, jt, cp)
    for name in NAMES[1:]:                                   # the grouped step's arguments, then n_bin, d_binp, d_bin before n_walker
        grouped = protos[name.replace("_binned", "_grouped")][1]
        params = protos[name][1]
        assert params[:len(grouped) - 2] == grouped[:-2] and params[-2:] == grouped[-2:]
        assert [p.split()[-1].lstrip("*") for p in params[-5:-2]] == ["n_bin", "d_binp", "d_bin"]
    plain = protos["fdg_chain_propose_device"][1]
    params = protos[NAMES[0]][1]
    assert params[:len(plain) - 2] == plain[:-2] and params[-2:] == plain[-2:]
    assert [p.split()[-1].lstrip("*") for p in params[len(plain) - 2:-2]] == ["move_discrete", "d_cdf", "n_bin", "d_ext", "n_ext", "ext_col", "d_bin",
                                                                             "d_binp"]
    for fn in ("chain_propose_device_discrete!", "chain_step_device_binned!", "mc_chain_step_device_binned!"):
        assert fn in export, fn
    hdr = open(JL.replace("feynmandiagram.jl_amd/julia/hip_compiler.jl", "include/fdg.h")).read()
    assert re.search(r"#define FDG_CHAIN_BIN_MAX 64\b", hdr) and capi.FDG_CHAIN_BIN_MAX == 64
    for h in (capi.GraphHandle.chain_step_device_binned, capi.GraphHandle.mc_chain_step_device_binned, capi.chain_propose_device_discrete,
              capi.chain_binned_reference, vegas.chain_integrate_binned):
        assert callable(h)
    assert fd.chain_integrate_binned is vegas.chain_integrate_binned


# ---- the driver --------------------------------------------------------------------------------------------------------------------- #
def test_driver_refusals():
    h = capi.GraphHandle(workloads.get("sigma2"))
    n_leaf = h.table.n_leaf
    assert n_leaf >= 4
    dmap = vegas.DiscreteMap(vegas.uniform_cdf(3), np.zeros((3, 1)), [2], device="cpu")
    kw = dict(n_walker=64, n_step=4, n_therm=1, n_warm=0, device="cpu")
    args = (h, None, [0, 0], [1, 1], [0, 1])
    for name, value in (("polar", [vegas.PolarVar(0, (0, 1, 2))]), ("observables", object()), ("freq_observables", object()),
                        ("strat", vegas.Stratification((1, 1))), ("matsubara", object()), ("groups", object())):
        with pytest.raises(ValueError, match=name):
            vegas.chain_integrate_binned(*args, dmap, **kw, **{name: value})
    with pytest.raises(TypeError):
        vegas.chain_integrate_binned(*args, dmap, **kw, n_iter=3)
    with pytest.raises(TypeError):
        vegas.chain_integrate_binned(*args, dmap, **kw, dmap=dmap)
    with pytest.raises(ValueError, match="dmap"):
        vegas.chain_integrate_binned(*args, object(), **kw)
    with pytest.raises(ValueError, match="reweight"):
        vegas.chain_integrate_binned(*args, dmap, **kw, reweight=[1.0])
    with pytest.raises(ValueError, match="warm-up"):                              # the leaf form has no warm-up with a discrete variable
        vegas.chain_integrate_binned(*args, dmap, **dict(kw, n_warm=1))
    for bad in (dict(n_therm=4), dict(n_walker=0), dict(n_step=0), dict(gamma=0.0), dict(gamma=math.inf), dict(gamma_rel=-1.0),
                dict(moves=[8]), dict(moves=[]), dict(shard_start=1), dict(n_warm=-1), dict(fixed=[0.0])):
        with pytest.raises(ValueError):
            vegas.chain_integrate_binned(*args, dmap, **dict(kw, **bad))
    with pytest.raises(ValueError, match="ext_col"):                              # the table's column is a variable's
        vegas.chain_integrate_binned(*args, vegas.DiscreteMap(vegas.uniform_cdf(3), np.zeros((3, 1)), [1], device="cpu"), **kw)
    with pytest.raises(ValueError, match="ext_col"):                              # ... or none of the graph's
        vegas.chain_integrate_binned(*args, vegas.DiscreteMap(vegas.uniform_cdf(3), np.zeros((3, 1)), [n_leaf], device="cpu"), **kw)
    big = capi.FDG_CHAIN_BIN_MAX + 1
    with pytest.raises(ValueError, match=str(capi.FDG_CHAIN_BIN_MAX)):
        vegas.chain_integrate_binned(*args, vegas.DiscreteMap(vegas.uniform_cdf(big), device="cpu"), **kw)
    # the drivers without the discrete variable go on refusing it
    groups = vegas.WeightGroups([0] * h.table.n_root, [[0, 1]])
    with pytest.raises(ValueError, match="dmap"):
        vegas.chain_integrate(*args, **kw, dmap=dmap)
    with pytest.raises(ValueError, match="dmap"):
        vegas.chain_integrate_grouped(*args, groups, **kw, dmap=dmap)
    assert "dmap" in vegas._CHAIN_EXCLUDED
