"""The Markov chain with weight groups and reweighting between orders, without a device (include/fdg.h:
fdg_chain_step_device_grouped, fdg_mc_chain_step_device_grouped; feynmandiagram.jl_amd/vegas.py: chain_integrate_grouped): the symbols
are declared, exported and bound, every argument check runs before any device work, the numpy mirror (capi.chain_grouped_reference:
what tests/test_chain_groups_accumulate.py compares the device with) ties to the plain and the projected mirrors bit for bit, and
the mirror of the whole driver meets on the CPU the statistical conditions of known answer A.

Known answer A (leaf form, sign-changing).  Leaves x, y and the constant c = 1 over the box [0, 2] x [0, 1]:
    r_0 = x - 0.3 c              group 0, variable 0 only      exact 1.4
    r_1 = (x - 0.3 c)(c - y)^3   group 1, variables 0 and 1    exact 0.35
    r_2 = x y                    group 1                       exact 1.0
coef = (1, 1, 1); a fixed non-uniform map with G = 16, edges 2 (i / G)^1.5 and (i / G)^0.7, so that the jacobians vary and differ
between the groups; 4096 walkers, 48 steps with 16 discarded, moves [3, 1, 2], gamma_rel = 1, rho from the first placement."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT
from test_chain_host import CHI2_HI, CHI2_LO, FAKE, INIT, MEASURE, failed, fresh_state, oracle_roots, step_uniforms
from test_chain_matsubara_host import MZ_INVALID, mz_desc
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_matsubara_accumulate import phase_table
from test_strat_accumulate import random_program, refined_grid
from test_vegas_host import JL

NAMES = ("fdg_chain_step_device_grouped", "fdg_mc_chain_step_device_grouped")
KNOWN_A = dict(n_walker=4096, n_step=48, n_therm=16, gamma_rel=1.0, n_grid=16, n_seed=32, moves=(3, 1, 2), exact=np.array([1.4, 0.35, 1.0]),
               root_group=(0, 1, 1), var_sets=((0,), (0, 1)), coef=(1.0, 1.0, 1.0), lo=(0.0, 0.0), hi=(2.0, 1.0))


# ---- the numpy mirror of the driver ----------------------------------------------------------------------------------------------------- #
def group_rho(st, root_group, var_sets, coef, exists, n_total=None):
    """rho_g = 1 / mean_b |jac_g s_g| of a placed state, the unprojected s_g; 1 for a group without a root that exists"""
    R, B = st["root"].shape
    rho = np.ones(len(var_sets))
    for g, vs in enumerate(var_sets):
        ks = [k for k in range(R) if (exists is None or exists[k]) and int(root_group[k]) == g]
        if not ks:
            continue
        jac = np.ones(B)
        for d in sorted(set(vs)):
            jac = jac * st["fac"][d]
        s = sum((1.0 if coef is None else float(coef[k])) * st["root"][k] for k in ks)
        rho[g] = 1.0 / (float(np.abs(jac * s).sum()) / (B if n_total is None else n_total))
    return rho


def mirror_chain_grouped(eval_roots, grid, col, fixed, R, root_group, var_sets, *, n_walker, n_step, n_therm, moves=None, gamma=None,
                         gamma_rel=1.0, seed=0, coef=None, exists=None, reweight=None, matsubara=None, each_step=None):
    """vegas.chain_integrate_grouped after the map's training, on the CPU: INIT without factors, rho, INIT again, gamma, the steps,
    the reduction, chain_estimate (tests/test_chain_host.py: mirror_chain)"""
    grid = np.asarray(grid, dtype=np.float64)
    D, B = grid.shape[0], int(n_walker)
    moves = vegas.chain_moves(D) if moves is None else list(moves)
    F = 0 if matsubara is None else len(matsubara["freq"])
    Cs = 2 * F * R if F else R

    def place(rho):
        st = fresh_state(fixed, D, R, B)
        st["sum"] = np.zeros((Cs + 1, B))
        u, ua = step_uniforms(B, D, (1 << D) - 1, seed, 0)
        return capi.chain_grouped_reference(grid, col, st, (1 << D) - 1, u, ua, 1.0, INIT, eval_roots, root_group, var_sets, rho, coef, exists,
                                            matsubara, phase_table)
    rho = None if reweight is None else np.asarray(reweight, dtype=np.float64)
    if rho is None:
        rho = group_rho(place(None), root_group, var_sets, coef, exists)
    st = place(rho)
    if gamma is None:
        gamma = gamma_rel * float(st["a"].sum()) / B
    st["n_accept"][:] = 0
    for t in range(n_step):
        mask, off = moves[t % len(moves)], (t + 1) * B
        u, ua = step_uniforms(B, D, mask, seed, off)
        st = capi.chain_grouped_reference(grid, col, st, mask, u, ua, gamma, MEASURE if t >= n_therm else 0, eval_roots, root_group, var_sets,
                                          rho, coef, exists, matsubara, phase_table)
        if each_step:
            each_step(t, st)
    red = capi.chain_reduce_reference(st["sum"])
    S, Q, X = red[:Cs + 1], red[Cs + 1:2 * Cs + 2], red[2 * Cs + 2:]
    mean, err = vegas.chain_estimate(S, Q, X, B)
    return dict(mean=mean, stderr=err, acceptance=float(st["n_accept"].sum()) / (B * n_step), gamma=gamma, reweight=rho, S=S, Q=Q, X=X, state=st)


@functools.lru_cache(maxsize=None)
def known_a_graph():
    """(table, [leaf of x, leaf of y], fixed leaf values) of known answer A"""
    x, y, c = fd.Graph([]), fd.Graph([]), fd.Graph([])
    r0 = fd.Graph([x, c], subgraph_factors=[1.0, -0.3], operator=fd.Sum())
    cube = fd.Graph([fd.Graph([c, y], subgraph_factors=[1.0, -1.0], operator=fd.Sum())], operator=fd.Power(3))
    r1 = fd.Graph([r0, cube], operator=fd.Prod())
    r2 = fd.Graph([x, y], operator=fd.Prod())
    t, leafmap, _ = lower([r0, r1, r2])
    at = {g.id: i - 1 for i, g in leafmap.items()}
    assert t.n_leaf == 3 and t.n_root == 3 and all(int(s) != FDG_NO_ROOT for s in t.root_slot)
    fixed = np.zeros(3)
    fixed[at[c.id]] = 1.0
    return t, [at[x.id], at[y.id]], fixed


def known_a_grid():
    i = np.arange(KNOWN_A["n_grid"] + 1, dtype=np.float64) / KNOWN_A["n_grid"]
    g = np.stack([2.0 * i ** 1.5, i ** 0.7])
    g[:, -1] = KNOWN_A["hi"]
    return np.ascontiguousarray(g)


def known_a_mirror(seed):
    t, col, fixed = known_a_graph()
    k = KNOWN_A
    return mirror_chain_grouped(oracle_roots(t), known_a_grid(), col, fixed, 3, k["root_group"], k["var_sets"], n_walker=k["n_walker"],
                                n_step=k["n_step"], n_therm=k["n_therm"], moves=k["moves"], gamma_rel=k["gamma_rel"], seed=seed,
                                coef=np.array(k["coef"]))


def test_known_a_graph_is_the_three_polynomials():
    t, col, fixed = known_a_graph()
    rng = np.random.default_rng(0)
    xp = np.repeat(fixed[:, None], 50, axis=1)
    xp[col[0]], xp[col[1]] = 2.0 * rng.random(50), rng.random(50)
    x, y = xp[col[0]], xp[col[1]]
    got = oracle_roots(t)(xp)
    assert np.allclose(got[0], x - 0.3, rtol=1e-14, atol=1e-16) and np.allclose(got[1], (x - 0.3) * (1 - y) ** 3, rtol=1e-13, atol=1e-16)
    assert np.allclose(got[2], x * y, rtol=1e-15)
    g = known_a_grid()
    assert g.shape == (2, 17) and (np.diff(g, axis=1) > 0).all() and g[0, 0] == 0.0 and g[0, -1] == 2.0 and g[1, -1] == 1.0


def test_known_answer_a_on_the_mirror(libfdg):
    """The sum over seeds 0 .. 31 of ((mean - exact) / sigma)^2 lies inside [10.3, 70.6] for each of the three roots, the 1e-4 and
    1 - 1e-4 quantiles of chi^2 with 32 degrees of freedom.  The values found are recorded in DESIGN 8m."""
    chi2, first = np.zeros(3), None
    for seed in range(KNOWN_A["n_seed"]):
        r = known_a_mirror(seed)
        first = first or r
        chi2 += ((r["mean"] - KNOWN_A["exact"]) / r["stderr"]) ** 2
    print("seed 0: mean", first["mean"], "stderr", first["stderr"], "errors", first["mean"] - KNOWN_A["exact"], "acceptance", first["acceptance"],
          "rho", first["reweight"], "gamma", first["gamma"])
    print("chi2 over 32 seeds", chi2)
    assert ((CHI2_LO <= chi2) & (chi2 <= CHI2_HI)).all()
    assert (np.abs(first["mean"] - KNOWN_A["exact"]) <= 5.0 * first["stderr"]).all()       # what the GPU file asserts at seed 0
    assert (first["reweight"] > 0).all() and 0.3 < first["acceptance"] < 1.0


# ---- mirror identities ------------------------------------------------------------------------------------------------------------------ #
def host_random_case():
    """tests/test_chain_accumulate.py's random case without the compiled function: ten roots, one of which does not exist; seven
    leaves, three of them variables"""
    t = random_program(21)
    rng = np.random.default_rng(8)
    col = [5, 0, 3]
    fixed = rng.uniform(-1.0, 1.0, size=t.n_leaf)
    grid = refined_grid(rng, len(col), 6)
    coef = rng.uniform(-1.0, 1.0, size=t.n_root)
    exists = [int(s) != FDG_NO_ROOT for s in t.root_slot]
    assert sum(exists) == t.n_root - 1 and t.n_root == 10
    return t, col, fixed, grid, coef, exists


IDENTITY_STEPS = [(0b111, INIT), (0b111, 0), (0b010, MEASURE), (0b101, MEASURE), (0, MEASURE), (0b111, MEASURE), (0b001, MEASURE)]   # INIT and 6 steps


def test_one_full_group_is_the_plain_mirror(libfdg):
    """one group, a full mask and reweight None: capi.chain_reference bit for bit over INIT and 6 steps"""
    t, col, fixed, grid, coef, exists = host_random_case()
    B, R, D, seed, gamma = 70, t.n_root, 3, 3, 0.37
    ev = oracle_roots(t)
    plain, grp = fresh_state(fixed, D, R, B), fresh_state(fixed, D, R, B)
    for i, (mask, flags) in enumerate(IDENTITY_STEPS):
        u, ua = step_uniforms(B, D, mask, seed, i * B)
        plain = capi.chain_reference(grid, col, plain, mask, u, ua, gamma, flags, ev, coef, exists)
        grp = capi.chain_grouped_reference(grid, col, grp, mask, u, ua, gamma, flags, ev, [0] * R, [(0, 1, 2)], None, coef, exists)
        for k in ("x", "fac", "root", "a", "sum", "n_accept", "xp", "facp"):
            assert np.array_equal(plain[k].view(np.uint8), grp[k].view(np.uint8)), (i, k)
    assert 0 < (plain["n_accept"] < len(IDENTITY_STEPS)).sum() and np.abs(plain["sum"][:R]).max() > 0.0


def test_one_full_group_with_the_projection_is_the_projected_mirror(libfdg):
    t, col, fixed, grid, coef, exists = host_random_case()
    B, R, D, seed, gamma, freq = 70, t.n_root, 3, 3, 0.37, (2, -1, 0)
    rng = np.random.default_rng(17)
    cin, cout = [int(v) for v in rng.integers(0, t.n_leaf, size=R)], [int(v) for v in rng.integers(0, t.n_leaf, size=R)]
    mz = dict(freq=freq, fermionic=True, weight_freq=1, root_col_in=cin, root_col_out=cout, beta=1.7)
    ev = oracle_roots(t)
    proj, grp = fresh_state(fixed, D, R, B), fresh_state(fixed, D, R, B)
    proj["sum"], grp["sum"] = np.zeros((2 * 3 * R + 1, B)), np.zeros((2 * 3 * R + 1, B))
    for i, (mask, flags) in enumerate(IDENTITY_STEPS):
        u, ua = step_uniforms(B, D, mask, seed, i * B)
        proj = capi.chain_matsubara_reference(grid, col, proj, mask, u, ua, gamma, flags, ev, freq, True, 1, cin, cout, 1.7, coef, exists)
        grp = capi.chain_grouped_reference(grid, col, grp, mask, u, ua, gamma, flags, ev, [0] * R, [(2, 0, 1)], None, coef, exists, mz)
        for k in ("x", "fac", "root", "a", "sum", "n_accept"):
            assert np.array_equal(proj[k].view(np.uint8), grp[k].view(np.uint8)), (i, k)
    assert 0 < (proj["n_accept"] < len(IDENTITY_STEPS)).sum() and np.abs(proj["sum"][1:-1:2]).max() > 0.0


GROUPS3 = dict(root_group=[2, 0, 2, 1, 0, 0, 2, 0, 2, 2], var_sets=[(0, 2), (0, 1, 2), ()])
"""three groups on the random case: group 1 holds only the root that does not exist (root 3), variable 1 belongs to no group with an
existing root, and group 2 has an empty mask"""


def test_doubling_reweight_and_gamma_scales_by_two(libfdg):
    """reweight and gamma both doubled: x, fac, root, n_accept identical, a exactly doubled, sum exactly halved (a scaling by 2 is
    exact in binary floating point, and both sides of the accept rule double)"""
    t, col, fixed, grid, coef, exists = host_random_case()
    assert not exists[3] and set(GROUPS3["root_group"][k] for k in range(10) if exists[k]) == {0, 2}
    B, R, D, seed, gamma = 70, t.n_root, 3, 5, 0.21
    rho = np.array([0.7, 1.9, 3.3])
    ev = oracle_roots(t)
    one, two = fresh_state(fixed, D, R, B), fresh_state(fixed, D, R, B)
    for i, (mask, flags) in enumerate(IDENTITY_STEPS):
        u, ua = step_uniforms(B, D, mask, seed, i * B)
        one = capi.chain_grouped_reference(grid, col, one, mask, u, ua, gamma, flags, ev, GROUPS3["root_group"], GROUPS3["var_sets"], rho, coef, exists)
        two = capi.chain_grouped_reference(grid, col, two, mask, u, ua, 2.0 * gamma, flags, ev, GROUPS3["root_group"], GROUPS3["var_sets"],
                                           2.0 * rho, coef, exists)
        for k in ("x", "fac", "root", "n_accept"):
            assert np.array_equal(one[k], two[k]), (i, k)
        assert np.array_equal(two["a"], 2.0 * one["a"]) and np.array_equal(two["sum"], 0.5 * one["sum"]), i
    assert 0 < (one["n_accept"] < len(IDENTITY_STEPS)).sum() and np.abs(one["sum"]).max() > 0.0
    assert (one["sum"][3] == 0.0).all() and (one["root"][3] == 0.0).all()             # the root that does not exist
    with pytest.raises(ValueError):
        capi.chain_grouped_reference(grid, col, one, 1, u, ua, gamma, 0, ev, [3] * R, GROUPS3["var_sets"], None, coef, exists)


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
        proj = protos[name.replace("_grouped", "_matsubara")][1]              # the projected step's arguments, the groups before n_walker
        assert params[:len(proj) - 2] == proj[:-2] and params[-2:] == proj[-2:] and "fdg_chain_groups" in params[-3]
    for fn in ("chain_step_device_grouped!", "mc_chain_step_device_grouped!"):
        assert fn in export, fn
    assert [n for n, _ in capi.ChainGroups._fields_] == ["n_group", "root_group", "var_mask", "reweight"]
    assert C.sizeof(capi.ChainGroups) == 32 and capi.ChainGroups.root_group.offset == 8 and capi.ChainGroups.reweight.offset == 24
    hdr = open(JL.replace("feynmandiagram.jl_amd/julia/hip_compiler.jl", "include/fdg.h")).read()
    assert re.search(r"typedef struct fdg_chain_groups \{", hdr)
    for h in (capi.GraphHandle.chain_step_device_grouped, capi.GraphHandle.mc_chain_step_device_grouped, capi.chain_grouped_reference,
              capi.make_chain_groups, vegas.chain_integrate_grouped):
        assert callable(h)
    assert fd.chain_integrate_grouped is vegas.chain_integrate_grouped
    assert [f.name for f in vegas.ChainResult.__dataclass_fields__.values()][-1] == "reweight"
    d, keep = capi.make_chain_groups([0, 1], [(0,), (0, 5)], [0.5, 2.0])
    assert d.n_group == 2 and keep[1].tolist() == [1, 33] and keep[2].tolist() == [0.5, 2.0]
    assert capi.make_chain_groups([0], [()])[0].reweight is None
    with pytest.raises(ValueError):
        capi.make_chain_groups([0, 1], [(0,), (1,)], [1.0])


# ---- argument errors, no device present ----------------------------------------------------------------------------------------------- #
def groups_desc(R, **kw):
    """a valid descriptor of R roots in two groups over three variables with the fields of ``kw`` replaced (a None array: NULL)"""
    rg, vm, rw = kw.pop("root_group", [k % 2 for k in range(R)]), kw.pop("var_mask", [0b011, 0b111]), kw.pop("reweight", None)
    keep = [None if v is None else np.ascontiguousarray(v, dtype=dt) for v, dt in ((rg, np.uint32), (vm, np.uint64), (rw, np.float64))]
    ptr = [None if v is None else v.ctypes.data for v in keep]
    d = capi.ChainGroups(kw.pop("n_group", 0 if vm is None else len(vm)), *ptr)
    assert not kw
    return d, keep


GROUPS_INVALID = (dict(root_group=None), dict(var_mask=None, n_group=2), dict(n_group=0), dict(var_mask=[0b011, 0b1000]),
                  dict(var_mask=[1 << 63, 0b111]), dict(reweight=[1.0, 0.0]), dict(reweight=[-1.0, 1.0]), dict(reweight=[math.inf, 1.0]),
                  dict(reweight=[1.0, math.nan]))


def _step_grp(h, cg, desc=None, mc=False, d_xp=FAKE[0], xpc=100, d_facp=FAKE[1], n_col=None, n_dim=3, coef=None, gamma=0.5, flags=MEASURE,
              d_x=FAKE[2], xc=100, d_fac=FAKE[3], d_root=FAKE[4], d_a=FAKE[5], d_sum=FAKE[6], d_n_accept=FAKE[7], B=100):
    if n_col is None:
        n_col = h.table.n_leaf if h is not None and not mc else 5
    c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    tail = (d_facp, n_col, n_dim, None if c is None else c.ctypes.data, gamma, 1, 0, flags, d_x, xc, d_fac, d_root, d_a, d_sum, d_n_accept,
            None if desc is None else C.addressof(desc), None if cg is None else C.addressof(cg), B, None)
    if mc:
        return capi.lib().fdg_mc_chain_step_device_grouped(h._h if h else None, d_xp, xpc, 1.0, 2.0, 0.5, *tail)
    return capi.lib().fdg_chain_step_device_grouped(h._h if h else None, d_xp, xpc, *tail)


def test_step_argument_checks_need_no_device(libfdg, tmp_path):
    t = workloads.get("sigma2")
    h = capi.GraphHandle(t)
    R, L = t.n_root, t.n_leaf
    ok, _k = groups_desc(R)
    for mc in (False, True):
        n_col = 5 if mc else L
        for B in (100, 0):                                   # refused with nothing to do, too
            # everything the plain step refuses
            for name in ("d_xp", "d_facp", "d_x", "d_fac", "d_root", "d_a", "d_sum"):
                assert failed(_step_grp(h, ok, None, mc, B=B, **{name: None}), capi.FDG_E_INVALID), name
            for kw in (dict(d_x=FAKE[0]), dict(d_n_accept=FAKE[6]), dict(gamma=0.0), dict(gamma=math.nan), dict(n_dim=0), dict(flags=4),
                       dict(coef=[math.nan] * R)) + ((dict(xc=99), dict(xpc=99)) if B else ()):      # (no stride is too short for no walker)
                assert failed(_step_grp(h, ok, None, mc, B=B, **kw), capi.FDG_E_INVALID), kw
            assert failed(_step_grp(None, ok, None, mc, B=B), capi.FDG_E_INVALID)
            assert failed(_step_grp(h, ok, None, mc, B=B, n_dim=capi.FDG_VEGAS_DIM_MAX + 1), capi.FDG_E_UNSUPPORTED)
            # everything the projected step refuses of its descriptor, except the NULL one
            for kw in MZ_INVALID:
                d, _k1 = mz_desc(R, n_col, **kw)
                assert failed(_step_grp(h, ok, d, mc, B=B), capi.FDG_E_INVALID), kw
            d, _k1 = mz_desc(R, n_col, cin=[0] * (R - 1) + [n_col])
            assert failed(_step_grp(h, ok, d, mc, B=B), capi.FDG_E_INVALID)
            d, _k1 = mz_desc(R, n_col, freq=list(range(capi.FDG_MATSUBARA_FREQ_MAX + 1)))
            assert failed(_step_grp(h, ok, d, mc, B=B), capi.FDG_E_UNSUPPORTED)
            # the groups
            good_mz, _k2 = mz_desc(R, n_col)
            for desc in (None, good_mz):
                assert failed(_step_grp(h, None, desc, mc, B=B), capi.FDG_E_INVALID)
                for kw in GROUPS_INVALID:
                    d, _k1 = groups_desc(R, **kw)
                    assert failed(_step_grp(h, d, desc, mc, B=B), capi.FDG_E_INVALID), kw
                d, _k1 = groups_desc(R, root_group=[0] * (R - 1) + [2])
                assert failed(_step_grp(h, d, desc, mc, B=B), capi.FDG_E_INVALID)
                n = capi.FDG_WEIGHT_GROUP_MAX + 1
                d, _k1 = groups_desc(R, var_mask=[0b111] * n, reweight=[1.0] * n)
                assert failed(_step_grp(h, d, desc, mc, B=B), capi.FDG_E_UNSUPPORTED)
        assert failed(_step_grp(h, ok, None, mc, B=-1), capi.FDG_E_INVALID)
    assert failed(_step_grp(h, ok, n_col=L + 1), capi.FDG_E_INVALID)                  # the leaf form: n_col is the number of leaves
    assert _step_grp(h, ok, B=0) == capi.FDG_OK and _step_grp(h, ok, B=0, flags=INIT, d_sum=None) == capi.FDG_OK
    good_mz, _k2 = mz_desc(R, L)
    assert _step_grp(h, ok, good_mz, B=0) == capi.FDG_OK
    d, _k1 = groups_desc(R, var_mask=[0, 0b111] + [0b101] * (capi.FDG_WEIGHT_GROUP_MAX - 2), reweight=[1e-300] + [1e300] * (capi.FDG_WEIGHT_GROUP_MAX - 1))
    assert _step_grp(h, d, B=0) == capi.FDG_OK                                        # 8 groups, an empty mask, extreme but finite factors
    d, _k1 = groups_desc(R, var_mask=[(1 << 64) - 1, 1 << 63])
    assert _step_grp(h, d, B=0, n_dim=64) == capi.FDG_OK                              # 64 variables: every bit is a variable
    assert failed(_step_grp(h, ok, None, True), capi.FDG_E_INVALID)                   # fdg_graph_specialize_fused has not been called
    # the Monte-Carlo form after fdg_graph_specialize_fused: two loops in two dimensions and one time are five columns
    a = fd.Graph([])
    t1, _, _ = lower([fd.Graph([a], subgraph_factors=[2.0])])
    tab, _keep = capi.make_leaf_tables([2], [2], [1], [1], [1], np.array([[1.0, -1.0]]), 2, 1)
    h1 = fd.compile_table(t1, specialize="isa", cache_dir=str(tmp_path)).handle
    h1.specialize_fused(tab, str(tmp_path))
    d1, _k3 = groups_desc(1)
    assert failed(_step_grp(h1, d1, None, True, n_col=4), capi.FDG_E_INVALID) and _step_grp(h1, d1, None, True, n_col=5, B=0) == capi.FDG_OK
    with pytest.raises(capi.FdgError) as e:
        h.chain_step_device_grouped(FAKE[0], 100, FAKE[1], L, 3, None, 0.5, 1, 0, MEASURE, FAKE[2], 100, FAKE[3], FAKE[4], FAKE[5], FAKE[6], 0,
                                    None, None, 100)
    assert e.value.code == capi.FDG_E_INVALID


def test_a_missing_root_may_name_any_group(libfdg):
    a, b = fd.Graph([]), fd.Graph([])
    g = fd.Graph([a, b], operator=fd.Prod())
    t, _, _ = lower([g], root=[g.id, 424_242])
    assert t.n_root == 2 and int(t.root_slot[1]) == FDG_NO_ROOT
    h = capi.GraphHandle(t)
    d, _k = groups_desc(2, root_group=[1, 1 << 30], var_mask=[0b01, 0b11])
    assert _step_grp(h, d, B=0, n_dim=2) == capi.FDG_OK
    d, _k = groups_desc(2, root_group=[2, 0], var_mask=[0b01, 0b11])
    assert failed(_step_grp(h, d, B=0, n_dim=2), capi.FDG_E_INVALID)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------ #
def test_driver_argument_checks():
    h = capi.GraphHandle(workloads.get("sigma2"))
    R = h.table.n_root
    kw = dict(n_walker=64, n_step=4, n_therm=1, device="cpu")
    good = vegas.WeightGroups((0,) * R, ((0, 1),))
    run = lambda groups=good, **more: vegas.chain_integrate_grouped(h, None, [0, 0], [1, 1], [0, 1], groups, **dict(kw, **more))
    for name, value in (("polar", [vegas.PolarVar(0, (0, 1, 2))]), ("dmap", object()), ("observables", object()),
                        ("freq_observables", object()), ("strat", vegas.Stratification((1, 1)))):
        with pytest.raises(ValueError, match=name):
            run(**{name: value})
    with pytest.raises(TypeError):
        run(n_iter=3)
    with pytest.raises(TypeError):
        vegas.chain_integrate_grouped(h, None, [0, 0], [1, 1], [0, 1], **kw)          # groups is not optional here
    for bad in (None, object(), vegas.WeightGroups((0,) * (R - 1), ((0, 1),)), vegas.WeightGroups((1,) * R, ((0, 1),)),
                vegas.WeightGroups((0,) * R, ((0, 2),)), vegas.WeightGroups((0,) * R, ((0,),) * (capi.FDG_WEIGHT_GROUP_MAX + 1))):
        with pytest.raises(ValueError, match="groups"):
            run(bad)
    for rw in ([1.0, 1.0], [0.0], [-1.0], [math.inf], [math.nan]):
        with pytest.raises(ValueError, match="reweight"):
            run(reweight=rw)
    with pytest.raises(ValueError):
        run(n_therm=4)                                       # the plain checks still run
    # chain_integrate itself keeps refusing groups
    with pytest.raises(ValueError, match="groups"):
        vegas.chain_integrate(h, None, [0, 0], [1, 1], [0, 1], **kw, groups=good)
    assert "groups" in vegas._CHAIN_EXCLUDED
