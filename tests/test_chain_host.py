"""Markov-chain sampling on the VEGAS map without a device (include/fdg.h: fdg_chain_propose_device, fdg_chain_step_device,
fdg_mc_chain_step_device, fdg_chain_reduce_device; feynmandiagram.jl_amd/vegas.py: chain_estimate, chain_integrate): the symbols are
declared, exported and bound, every argument check runs before any device work, chain_estimate is the delta method it states, and the
numpy mirror of the whole driver (capi.chain_reference step by step: what tests/test_chain_accumulate.py compares the device with)
meets on the CPU the statistical conditions that file asserts on the GPU, so that they cannot have been tuned against the device.

The known-answer case.  The graph model has sums, products and integer powers, no exp, so the pair of roots is a polynomial one with
a closed form and the same change of sign: over [0, 1]^2
    r_0 = (x - 0.3) (1 - y)^3,   I_0 = 0.2 / 4 = 0.05          r_1 = x y,   I_1 = 0.25
with coef = [1, 1]; a third leaf holds the constant 1.  n_walker = 4096, n_step = 48, n_therm = 16, moves = [all, x, y],
gamma = 0.05, the uniform map."""
import math
import re

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_vegas_host import JL

NAMES = ("fdg_chain_propose_device", "fdg_chain_step_device", "fdg_mc_chain_step_device", "fdg_chain_reduce_device")
FAKE = [0x10000 * (i + 1) for i in range(8)]              # compared with NULL and each other only
INIT, MEASURE = capi.FDG_CHAIN_INIT, capi.FDG_CHAIN_MEASURE
U_COL = capi.FDG_VEGAS_DIM_MAX                            # the variable index of the accept rule's uniform
CHI2_LO, CHI2_HI = 10.3, 70.6                             # the 1e-4 and 1 - 1e-4 quantiles of chi^2 with 32 degrees of freedom

KNOWN = dict(n_walker=4096, n_step=48, n_therm=16, gamma=0.05, n_grid=8, n_seed=32, exact=np.array([0.05, 0.25]))


# ---- the numpy mirror of the driver --------------------------------------------------------------------------------------------------- #
def philox_columns(B, cols, seed, sample_offset=0):
    """oracle.philox_uniform for the columns ``cols`` only: ``[B, len(cols)]`` (the chain needs a few variables and column 64)."""
    b = (np.arange(B, dtype=np.uint64) + np.uint64(sample_offset))[:, None]
    i = np.asarray(list(cols), dtype=np.uint64)[None, :]
    shape = (B, i.shape[1])
    MASK = np.uint64(0xFFFFFFFF)
    c0, c1 = np.broadcast_to(b & MASK, shape).copy(), np.broadcast_to(b >> np.uint64(32), shape).copy()
    c2, c3 = np.broadcast_to(i, shape).copy(), np.zeros(shape, dtype=np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & MASK, (k1 + np.uint64(0xBB67AE85)) & MASK
    return (((c0 >> np.uint64(5)) << np.uint64(26)) | (c1 >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def step_uniforms(B, D, mask, seed, off):
    """``(u [B, D], u_acc [B])`` of one step: only the columns of ``mask`` are filled"""
    u = np.zeros((B, D))
    ds = [d for d in range(D) if (mask >> d) & 1]
    if ds:
        u[:, ds] = philox_columns(B, ds, seed, off)
    return u, philox_columns(B, [U_COL], seed, off)[:, 0]


def fresh_state(fixed, D, R, B):
    return {"x": np.repeat(np.asarray(fixed, dtype=np.float64)[:, None], B, axis=1), "fac": np.ones((D, B)), "root": np.zeros((R, B)),
            "a": np.zeros(B), "sum": np.zeros((R + 1, B)), "n_accept": np.zeros(B, dtype=np.int32)}


def oracle_roots(table):
    """the roots of proposals ``xp [n_leaf, B]`` by the CPU oracle: bit for bit the device's in the leaf form"""
    return lambda xp: np.ascontiguousarray(oracle.eval_static(table, np.ascontiguousarray(xp.T)).T)


def mirror_chain(eval_roots, grid, col, fixed, R, *, n_walker, n_step, n_therm, moves=None, gamma=None, gamma_rel=1.0, seed=0, coef=None,
                 exists=None, n_total=None, shard_start=0, each_step=None):
    """vegas.chain_integrate after the map's training, on the CPU: INIT, gamma, the steps, the reduction, chain_estimate.  The
    states are the device's bit for bit (capi.chain_reference on the device's uniforms); the reduced sums are exact (math.fsum).
    ``each_step(t, state)`` sees the state after INIT (t = -1) and after every step."""
    grid = np.asarray(grid, dtype=np.float64)
    D, B = grid.shape[0], int(n_walker)
    N = B if n_total is None else int(n_total)
    moves = vegas.chain_moves(D) if moves is None else list(moves)
    st = fresh_state(fixed, D, R, B)
    u, ua = step_uniforms(B, D, (1 << D) - 1, seed, shard_start)
    st = capi.chain_reference(grid, col, st, (1 << D) - 1, u, ua, 1.0, INIT, eval_roots, coef, exists)
    if gamma is None:
        gamma = gamma_rel * float(st["a"].sum()) / N
    st["n_accept"][:] = 0
    if each_step:
        each_step(-1, st)
    for t in range(n_step):
        mask, off = moves[t % len(moves)], (t + 1) * N + shard_start
        u, ua = step_uniforms(B, D, mask, seed, off)
        st = capi.chain_reference(grid, col, st, mask, u, ua, gamma, MEASURE if t >= n_therm else 0, eval_roots, coef, exists)
        if each_step:
            each_step(t, st)
    red = capi.chain_reduce_reference(st["sum"])
    S, Q, X = red[:R + 1], red[R + 1:2 * R + 2], red[2 * R + 2:]
    mean, err = vegas.chain_estimate(S, Q, X, B)
    return dict(mean=mean, stderr=err, acceptance=float(st["n_accept"].sum()) / (B * n_step), gamma=gamma, S=S, Q=Q, X=X, state=st)


def known_graph():
    """(table, [leaf of x, leaf of y], fixed leaf values) of r_0 = (x - 0.3 c)(c - y)^3, r_1 = x y with the constant leaf c = 1"""
    x, y, c = fd.Graph([]), fd.Graph([]), fd.Graph([])
    a = fd.Graph([x, c], subgraph_factors=[1.0, -0.3], operator=fd.Sum())
    b = fd.Graph([fd.Graph([c, y], subgraph_factors=[1.0, -1.0], operator=fd.Sum())], operator=fd.Power(3))
    r0 = fd.Graph([a, b], operator=fd.Prod())
    r1 = fd.Graph([x, y], operator=fd.Prod())
    t, leafmap, _ = lower([r0, r1])
    at = {g.id: i - 1 for i, g in leafmap.items()}
    assert t.n_leaf == 3 and t.n_root == 2
    fixed = np.zeros(3)
    fixed[at[c.id]] = 1.0
    return t, [at[x.id], at[y.id]], fixed


def known_mirror(seed, n_therm=None, table=None):
    t, col, fixed = table or known_graph()
    k = KNOWN
    return mirror_chain(oracle_roots(t), vegas.uniform_grid([0, 0], [1, 1], k["n_grid"]), col, fixed, 2, n_walker=k["n_walker"],
                        n_step=k["n_step"], n_therm=k["n_therm"] if n_therm is None else n_therm, moves=[3, 1, 2], gamma=k["gamma"],
                        seed=seed, coef=np.array([1.0, 1.0]))


def known_chi2(run):
    """sum over the seeds of ((mean - exact) / sigma)^2 per root, and the results of seed 0"""
    chi2, first = np.zeros(2), None
    for seed in range(KNOWN["n_seed"]):
        r = run(seed)
        first = first or r
        chi2 += ((np.asarray(r["mean"]) - KNOWN["exact"]) / np.asarray(r["stderr"])) ** 2
    return chi2, first


def test_philox_columns_are_the_oracles():
    want = oracle.philox_uniform(70, U_COL + 1, 0x1234567890ABCDEF, (1 << 33) + 5)
    assert np.array_equal(philox_columns(70, [0, 3, U_COL], 0x1234567890ABCDEF, (1 << 33) + 5), want[:, [0, 3, U_COL]])


def test_known_graph_is_the_polynomial_pair():
    t, col, fixed = known_graph()
    rng = np.random.default_rng(0)
    xp = np.repeat(fixed[:, None], 50, axis=1)
    xp[col] = rng.random((2, 50))
    x, y = xp[col[0]], xp[col[1]]
    got = oracle_roots(t)(xp)
    assert np.allclose(got[0], (x - 0.3) * (1 - y) ** 3, rtol=1e-13, atol=1e-16) and np.allclose(got[1], x * y, rtol=1e-15)


def test_mirror_meets_the_conditions_of_the_gpu_tests(libfdg):
    """Conditions, not measurements: the GPU file asserts |mean - exact| < 5 sigma at seed 0 and chi2 over 32 seeds inside
    [10.3, 70.6] per root; the mirror alone must meet both.  It gives chi2 = 31.57 (root 0) and 40.61 (root 1), acceptance 0.740."""
    table = known_graph()
    chi2, first = known_chi2(lambda seed: known_mirror(seed, table=table))
    print("seed 0: mean", first["mean"], "stderr", first["stderr"], "acceptance", first["acceptance"], "chi2 over 32 seeds", chi2)
    assert (np.abs(first["mean"] - KNOWN["exact"]) < 5.0 * first["stderr"]).all()
    assert ((CHI2_LO <= chi2) & (chi2 <= CHI2_HI)).all()
    assert 0.5 < first["acceptance"] < 0.95


def test_mirror_without_thermalisation_is_worse(libfdg):
    """A chain measured from its first step is biased: the walkers start in the map's density, not in the stationary one.  With
    n_therm = 0 the chi2 over the 32 seeds is larger than with n_therm = 16 for both roots: 80.4 and 252.9 against 31.6 and 40.6."""
    table = known_graph()
    cold, _ = known_chi2(lambda seed: known_mirror(seed, n_therm=0, table=table))
    warm, _ = known_chi2(lambda seed: known_mirror(seed, table=table))
    print("chi2 with n_therm = 0:", cold, "with n_therm = 16:", warm)
    assert (cold > warm).all()


def test_mirror_identities(libfdg):
    """The empty mask leaves the state as it is and accepts everywhere; coef = 0 with gamma = 1 accepts every proposal."""
    t, col, fixed = known_graph()
    grid = vegas.uniform_grid([0, 0], [1, 1], 4)
    seen = {}
    r = mirror_chain(oracle_roots(t), grid, col, fixed, 2, n_walker=70, n_step=4, n_therm=1, moves=[3, 0], gamma=0.05, seed=3,
                     each_step=lambda s, st: seen.__setitem__(s, st))
    for k in ("x", "fac", "root", "a"):
        assert np.array_equal(seen[1][k], seen[0][k]) and np.array_equal(seen[3][k], seen[2][k]), k
    assert (seen[1]["n_accept"] == seen[0]["n_accept"] + 1).all()
    r = mirror_chain(oracle_roots(t), grid, col, fixed, 2, n_walker=70, n_step=3, n_therm=0, moves=[3], gamma=1.0, seed=3, coef=np.zeros(2))
    assert r["acceptance"] == 1.0


# ---- declared, exported, bound ------------------------------------------------------------------------------------------------------ #
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
    for fn in ("chain_propose_device!", "chain_step_device!", "mc_chain_step_device!", "chain_reduce_device!"):
        assert fn in export, fn
    assert fd.chain_integrate is vegas.chain_integrate and fd.chain_estimate is vegas.chain_estimate and fd.ChainResult is vegas.ChainResult
    assert (INIT, MEASURE) == (1, 2)
    hdr = open(JL.replace("feynmandiagram.jl_amd/julia/hip_compiler.jl", "include/fdg.h")).read()
    assert re.search(r"#define FDG_CHAIN_INIT 1u", hdr) and re.search(r"#define FDG_CHAIN_MEASURE 2u", hdr)
    for h in (capi.GraphHandle.chain_step_device, capi.GraphHandle.mc_chain_step_device, capi.chain_reference, capi.chain_reduce_reference):
        assert callable(h)


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def failed(rc, code):
    return rc == code and len(capi.lib().fdg_last_error()) > 0


def _propose(n_dim=3, n_grid=8, col=None, n_col=5, mask=0b101, d_grid=FAKE[0], d_x=FAKE[1], xc=100, d_fac=FAKE[2], d_xp=FAKE[3], xpc=100,
             d_facp=FAKE[4], B=100):
    c = None if col is None else np.ascontiguousarray(col, dtype=np.uint32)
    return capi.lib().fdg_chain_propose_device(d_grid, n_dim, n_grid, None if c is None else c.ctypes.data, n_col, mask, 1, 0, d_x, xc, d_fac,
                                               d_xp, xpc, d_facp, B, None)


def _step(h, mc=False, d_xp=FAKE[0], xpc=100, d_facp=FAKE[1], n_col=None, n_dim=3, coef=None, gamma=0.5, flags=MEASURE, d_x=FAKE[2], xc=100,
          d_fac=FAKE[3], d_root=FAKE[4], d_a=FAKE[5], d_sum=FAKE[6], d_n_accept=FAKE[7], B=100):
    if n_col is None:
        n_col = h.table.n_leaf if h is not None and not mc else 5
    c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    tail = (d_facp, n_col, n_dim, None if c is None else c.ctypes.data, gamma, 1, 0, flags, d_x, xc, d_fac, d_root, d_a, d_sum, d_n_accept, B,
            None)
    if mc:
        return capi.lib().fdg_mc_chain_step_device(h._h if h else None, d_xp, xpc, 1.0, 2.0, 0.5, *tail)
    return capi.lib().fdg_chain_step_device(h._h if h else None, d_xp, xpc, *tail)


def test_propose_argument_checks_need_no_device(libfdg):
    for kw in (dict(d_grid=None), dict(d_x=None), dict(d_fac=None), dict(d_xp=None), dict(d_facp=None), dict(B=-1), dict(n_dim=0, mask=0),
               dict(n_grid=0), dict(d_xp=FAKE[1]), dict(d_facp=FAKE[2]), dict(mask=0b1000), dict(mask=1 << 63), dict(col=[0, 1, 5]),
               dict(n_col=2), dict(xc=99), dict(xpc=99)):
        assert failed(_propose(**kw), capi.FDG_E_INVALID), kw
    assert failed(_propose(n_grid=capi.FDG_VEGAS_GRID_MAX + 1), capi.FDG_E_UNSUPPORTED)
    assert failed(_propose(n_dim=capi.FDG_VEGAS_DIM_MAX + 1, n_col=100), capi.FDG_E_UNSUPPORTED)
    assert _propose(B=0) == capi.FDG_OK and _propose(mask=0, B=0) == capi.FDG_OK and _propose(col=[4, 0, 2], B=0) == capi.FDG_OK
    assert _propose(n_dim=64, n_col=64, mask=(1 << 64) - 1, B=0) == capi.FDG_OK          # 64 variables: the accept rule's index is 64
    with pytest.raises(ValueError):
        capi.chain_propose_device(FAKE[0], 3, 8, [0, 1], 5, 1, 1, 0, FAKE[1], 100, FAKE[2], FAKE[3], 100, FAKE[4], 100)
    with pytest.raises(capi.FdgError) as e:
        capi.chain_propose_device(FAKE[0], 3, 8, None, 5, 8, 1, 0, FAKE[1], 100, FAKE[2], FAKE[3], 100, FAKE[4], 100)
    assert e.value.code == capi.FDG_E_INVALID


def test_step_argument_checks_need_no_device(libfdg, tmp_path):
    t = workloads.get("sigma2")
    h = capi.GraphHandle(t)
    arrays = ("d_xp", "d_facp", "d_x", "d_fac", "d_root", "d_a", "d_sum")
    for mc in (False, True):
        for name in arrays:
            assert failed(_step(h, mc, **{name: None}), capi.FDG_E_INVALID), name
        for i, a in enumerate(arrays):                      # any two of the state, proposal and sum arrays the same buffer
            for b in arrays[:i]:
                assert failed(_step(h, mc, **{a: FAKE[arrays.index(b)]}), capi.FDG_E_INVALID), (a, b)
        assert failed(_step(h, mc, d_n_accept=FAKE[6]), capi.FDG_E_INVALID)
        for g in (0.0, -1.0, math.inf, -math.inf, math.nan):
            assert failed(_step(h, mc, gamma=g), capi.FDG_E_INVALID), g
        for kw in (dict(B=-1), dict(n_dim=0), dict(flags=4), dict(xc=99), dict(xpc=99), dict(coef=[math.nan] * t.n_root),
                   dict(coef=[1.0] * (t.n_root - 1) + [math.inf])):
            assert failed(_step(h, mc, **kw), capi.FDG_E_INVALID), kw
        assert failed(_step(None, mc), capi.FDG_E_INVALID)
        assert failed(_step(h, mc, n_dim=capi.FDG_VEGAS_DIM_MAX + 1), capi.FDG_E_UNSUPPORTED)
    assert failed(_step(h, n_col=t.n_leaf + 1), capi.FDG_E_INVALID)                 # the leaf form: n_col is the number of leaves
    assert _step(h, B=0) == capi.FDG_OK and _step(h, B=0, d_n_accept=None) == capi.FDG_OK
    assert _step(h, B=0, flags=INIT, d_sum=None) == capi.FDG_OK                       # no sums without FDG_CHAIN_MEASURE
    assert failed(_step(h, True), capi.FDG_E_INVALID)                                # fdg_graph_specialize_fused has not been called
    assert failed(_step(h, True, B=0), capi.FDG_E_INVALID)
    # the Monte-Carlo form after fdg_graph_specialize_fused: two loops in two dimensions and one time are five columns
    a = fd.Graph([])
    t1, _, _ = lower([fd.Graph([a], subgraph_factors=[2.0])])
    tab, _keep = capi.make_leaf_tables([2], [2], [1], [1], [1], np.array([[1.0, -1.0]]), 2, 1)
    h1 = fd.compile_table(t1, specialize="isa", cache_dir=str(tmp_path)).handle
    h1.specialize_fused(tab, str(tmp_path))
    assert failed(_step(h1, True, n_col=4), capi.FDG_E_INVALID) and failed(_step(h1, True, n_col=6), capi.FDG_E_INVALID)
    assert _step(h1, True, n_col=5, B=0) == capi.FDG_OK
    with pytest.raises(ValueError):
        h.chain_step_device(FAKE[0], 100, FAKE[1], t.n_leaf, 3, [1.0], 0.5, 1, 0, MEASURE, FAKE[2], 100, FAKE[3], FAKE[4], FAKE[5], FAKE[6], 0, 100)
    with pytest.raises(capi.FdgError) as e:
        h.mc_chain_step_device(FAKE[0], 100, 1.0, 2.0, 0.5, FAKE[1], 5, 3, None, 0.5, 1, 0, MEASURE, FAKE[2], 100, FAKE[3], FAKE[4], FAKE[5],
                               FAKE[6], 0, 100)
    assert e.value.code == capi.FDG_E_INVALID


def test_reduce_argument_checks_need_no_device(libfdg):
    L = capi.lib()
    assert failed(L.fdg_chain_reduce_device(None, 3, 10, FAKE[1], None), capi.FDG_E_INVALID)
    assert failed(L.fdg_chain_reduce_device(FAKE[0], 3, 10, None, None), capi.FDG_E_INVALID)
    assert failed(L.fdg_chain_reduce_device(FAKE[0], 3, 10, FAKE[0], None), capi.FDG_E_INVALID)
    assert failed(L.fdg_chain_reduce_device(FAKE[0], 3, -1, FAKE[1], None), capi.FDG_E_INVALID)
    assert L.fdg_chain_reduce_device(FAKE[0], 3, 0, FAKE[1], None) == capi.FDG_OK


# ---- the estimate ------------------------------------------------------------------------------------------------------------------- #
def test_chain_estimate_is_the_delta_method_over_the_walkers():
    rng = np.random.default_rng(5)
    R, B = 4, 500
    A = rng.normal(size=(R + 1, B)) * rng.uniform(0.5, 3.0, size=(R + 1, 1))
    A[R] = rng.uniform(1.0, 3.0, size=B)                   # the normalisation is positive
    red = capi.chain_reduce_reference(A)
    assert red.shape == (3 * R + 2,)
    assert np.allclose(red[:R + 1], A.sum(axis=1), rtol=1e-13) and np.allclose(red[R + 1:2 * R + 2], (A * A).sum(axis=1), rtol=1e-13)
    assert np.allclose(red[2 * R + 2:], (A[:R] * A[R]).sum(axis=1), rtol=1e-12, atol=1e-12)
    mean, err = vegas.chain_estimate(red[:R + 1], red[R + 1:2 * R + 2], red[2 * R + 2:], B)
    # directly: the ratio of the sums, its variance from the sample covariance of the walkers' (A_k, A_R)
    for k in range(R):
        m = A[k].sum() / A[R].sum()
        V = B * np.cov(np.stack([A[k], A[R]]), ddof=1)
        var = (V[0, 0] - 2.0 * m * V[0, 1] + m * m * V[1, 1]) / A[R].sum() ** 2
        assert abs(mean[k] - m) <= 1e-13 * abs(m) and abs(err[k] - math.sqrt(var)) <= 1e-10 * math.sqrt(var), k
    # ... which is the jackknife's figure to first order
    jack = np.array([(A[0].sum() - A[0, b]) / (A[R].sum() - A[R, b]) for b in range(B)])
    assert abs(math.sqrt((B - 1.0) / B * ((jack - jack.mean()) ** 2).sum()) - err[0]) < 0.05 * err[0]


def test_chain_estimate_degenerate_cases():
    mean, err = vegas.chain_estimate([2.0, 4.0], [4.0, 16.0], [8.0], 1)      # one walker: no spread to measure
    assert mean[0] == 0.5 and np.isnan(err).all()
    with pytest.raises(ValueError):
        vegas.chain_estimate([2.0, 0.0], [4.0, 0.0], [0.0], 10)              # nothing was measured
    with pytest.raises(ValueError):
        vegas.chain_estimate([2.0, 1.0], [4.0], [0.0], 10)
    mean, err = vegas.chain_estimate([3.0, 3.0], [3.0, 3.0], [3.0], 3)       # every walker the same: the spread is zero, not negative
    assert mean[0] == 1.0 and err[0] == 0.0


# ---- the driver --------------------------------------------------------------------------------------------------------------------- #
def test_driver_refuses_the_excluded_combinations():
    h = capi.GraphHandle(workloads.get("sigma2"))
    kw = dict(n_walker=64, n_step=4, n_therm=1, device="cpu")
    for name, value in (("polar", [vegas.PolarVar(0, (0, 1, 2))]), ("groups", vegas.WeightGroups([0], [[0]])), ("dmap", object()),
                        ("matsubara", object()), ("observables", object()), ("freq_observables", object()),
                        ("strat", vegas.Stratification((1, 1)))):
        with pytest.raises(ValueError, match=name):
            vegas.chain_integrate(h, None, [0, 0], [1, 1], [0, 1], **kw, **{name: value})
    with pytest.raises(TypeError):
        vegas.chain_integrate(h, None, [0, 0], [1, 1], [0, 1], **kw, n_iter=3)
    for bad in (dict(n_therm=4), dict(n_walker=0), dict(n_step=0), dict(gamma=0.0), dict(gamma=math.inf), dict(gamma_rel=-1.0),
                dict(moves=[4]), dict(moves=[]), dict(shard_start=1), dict(n_warm=-1), dict(fixed=[0.0])):
        with pytest.raises(ValueError):
            vegas.chain_integrate(h, None, [0, 0], [1, 1], [0, 1], **dict(kw, **bad))
    with pytest.raises(ValueError):
        vegas.chain_integrate(h, None, [0, 0], [1, 1], [0, 0], **kw)
    assert vegas.chain_moves(3) == [7, 1, 2, 4]
