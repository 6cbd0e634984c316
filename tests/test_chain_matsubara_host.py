"""The Markov chain with a Matsubara-projected weight and measurement, without a device (include/fdg.h:
fdg_chain_step_device_matsubara, fdg_mc_chain_step_device_matsubara; feynmandiagram.jl_amd/vegas.py: chain_integrate(matsubara=...)):
the symbols are declared, exported and bound, every argument check runs before any device work, chain_estimate serves the
2 F R + 1 layout, the driver's complex assembly is the columns it came from, and the numpy mirror of the whole driver
(capi.chain_matsubara_reference step by step: what tests/test_chain_matsubara_accumulate.py compares the device with) meets on the
CPU the statistical conditions that file asserts on the GPU, so that they cannot have been tuned against the device.

The known answers.  Monte-Carlo form, fermionic propagators of order 0, T1 = 0 fixed, k fixed with eps = k^2 - kF^2 = +-1.25
(kF = 1.5, k = sqrt(3.5) or 1), beta = 3, frequencies n = 0, 1, -3, the uniform map, weight_freq = 0:
  one root    r = G(T1->T2) G(T1->T2) G(T2->T1) over tau = T2 in [0, beta]:
              int r e^{i omega_n tau} = -1 / ((1 + e^{-eps beta}) (1 + e^{eps beta}) (eps - i omega_n))
  two roots   the same with the pairs (1, 2) and (1, 3) over (T2, T3) in [0, beta]^2, coef = (1, 0.6): each root's integral is beta
              times the one-root value, and the weight |c_0 r_0 e^{i omega tau_2} + c_1 r_1 e^{i omega tau_3}| is not separable.
The closed form is confirmed against a Gauss-Legendre quadrature of the numpy leaf oracle; the assertions use the quadrature."""
import functools
import math
import re

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from test_chain_host import CHI2_HI, CHI2_LO, FAKE, INIT, MEASURE, failed, fresh_state, known_graph, oracle_roots, step_uniforms
from test_julia_shim import c_class, c_prototypes, jl_ccalls, jl_class
from test_matsubara_accumulate import phase_table
from test_vegas_host import JL

NAMES = ("fdg_chain_step_device_matsubara", "fdg_mc_chain_step_device_matsubara")
KNOWN_MZ = dict(n_walker=2048, n_step=40, n_therm=8, gamma_rel=1.0, n_grid=8, n_seed=32, kF=1.5, beta=3.0, freq=(0, 1, -3),
                k={1.25: math.sqrt(3.5), -1.25: 1.0}, coef2=(1.0, 0.6))


# ---- the known answers ---------------------------------------------------------------------------------------------------------------- #
@functools.lru_cache(maxsize=None)
def known_mz_case(n_root):
    """(table, leaf-table arguments, n_col, col, projection) of the one- or two-root case: root r is the product of three propagator
    leaves, two from T1 to T(2 + r) and one back"""
    roots, leaves, tin, tout = [], [], {}, {}
    for r in range(n_root):
        g = [fd.Graph([]) for _ in range(3)]
        for i, leaf in enumerate(g):
            tin[leaf.id], tout[leaf.id] = (1, 2 + r) if i < 2 else (2 + r, 1)
        leaves += g
        roots.append(fd.Graph(g, operator=fd.Prod()))
    t, leafmap, _ = lower(roots)
    assert t.n_leaf == 3 * n_root and t.n_root == n_root
    ids = [leafmap[i + 1].id for i in range(t.n_leaf)]
    one = np.ones(t.n_leaf, np.int32)
    n_tau = 1 + n_root
    args = (one, np.zeros(t.n_leaf, np.int32), np.array([tin[i] for i in ids], np.int32), np.array([tout[i] for i in ids], np.int32), one,
            np.array([[1.0]]), 3, n_tau)
    mz = vegas.MatsubaraProjection(freq=KNOWN_MZ["freq"], fermionic=True, root_tau_in=(1,) * n_root, root_tau_out=tuple(range(2, 2 + n_root)))
    return t, args, 3 + n_tau, list(range(4, 3 + n_tau)), mz


def known_mz_roots(n_root, k):
    """``eval_roots(xp [n_col, B]) -> [R, B]`` by the numpy leaf oracle and the CPU oracle's graph"""
    t, args, n_col, _, _ = known_mz_case(n_root)

    def ev(xp):
        B = xp.shape[1]
        leaf = oracle.leaf_values(*args[:6], np.ascontiguousarray(xp[:3].T).reshape(B, 1, 3), np.ascontiguousarray(xp[3:].T), KNOWN_MZ["kF"],
                                  KNOWN_MZ["beta"], 0.0)
        return np.ascontiguousarray(oracle.eval_static(t, np.ascontiguousarray(leaf)).T)
    return ev


def known_mz_fixed(n_root, k):
    fixed = np.zeros(known_mz_case(n_root)[2])
    fixed[0] = k
    return fixed


def closed_form(eps, n):
    beta = KNOWN_MZ["beta"]
    return -1.0 / ((1.0 + math.exp(-eps * beta)) * (1.0 + math.exp(eps * beta)) * (eps - 1j * (2 * n + 1) * math.pi / beta))


@functools.lru_cache(maxsize=None)
def quadrature(eps):
    """int_0^beta r(tau) e^{i omega_n tau} dtau per frequency, 96-point Gauss-Legendre on each of 8 panels, r from the leaf oracle"""
    beta, k = KNOWN_MZ["beta"], KNOWN_MZ["k"][eps]
    z, w = np.polynomial.legendre.leggauss(96)
    edges = np.linspace(0.0, beta, 9)
    tau = np.concatenate([0.5 * (b - a) * z + 0.5 * (a + b) for a, b in zip(edges[:-1], edges[1:])])
    wt = np.concatenate([0.5 * (b - a) * w for a, b in zip(edges[:-1], edges[1:])])
    xp = np.repeat(known_mz_fixed(1, k)[:, None], tau.size, axis=1)
    xp[4] = tau
    r = known_mz_roots(1, k)(xp)[0]
    return np.array([np.sum(wt * r * np.exp(1j * (2 * n + 1) * math.pi / beta * tau)) for n in KNOWN_MZ["freq"]])


def known_mz_exact(n_root, eps):
    """[F, R] complex: the quadrature's values (times beta per root in the two-root case: the other time is free)"""
    q = quadrature(eps)
    return np.repeat(q[:, None] * (KNOWN_MZ["beta"] if n_root == 2 else 1.0), n_root, axis=1)


# ---- the numpy mirror of the driver ----------------------------------------------------------------------------------------------------- #
def mirror_chain_mz(eval_roots, grid, col, fixed, R, freq, fermionic, weight_freq, cin, cout, beta, *, n_walker, n_step, n_therm, moves=None,
                    gamma=None, gamma_rel=1.0, seed=0, coef=None, exists=None, each_step=None):
    """vegas.chain_integrate(matsubara=...) after the map's training, on the CPU (tests/test_chain_host.py: mirror_chain)"""
    grid = np.asarray(grid, dtype=np.float64)
    D, B, F = grid.shape[0], int(n_walker), len(freq)
    C = 2 * F * R
    moves = vegas.chain_moves(D) if moves is None else list(moves)
    st = fresh_state(fixed, D, R, B)
    st["sum"] = np.zeros((C + 1, B))
    mz = (freq, fermionic, weight_freq, cin, cout, beta)
    u, ua = step_uniforms(B, D, (1 << D) - 1, seed, 0)
    st = capi.chain_matsubara_reference(grid, col, st, (1 << D) - 1, u, ua, 1.0, INIT, eval_roots, *mz, coef, exists, phase_table)
    if gamma is None:
        gamma = gamma_rel * float(st["a"].sum()) / B
    st["n_accept"][:] = 0
    for t in range(n_step):
        mask, off = moves[t % len(moves)], (t + 1) * B
        u, ua = step_uniforms(B, D, mask, seed, off)
        st = capi.chain_matsubara_reference(grid, col, st, mask, u, ua, gamma, MEASURE if t >= n_therm else 0, eval_roots, *mz, coef, exists,
                                            phase_table)
        if each_step:
            each_step(t, st)
    red = capi.chain_reduce_reference(st["sum"])
    S, Q, X = red[:C + 1], red[C + 1:2 * C + 2], red[2 * C + 2:]
    mean, err = vegas.chain_estimate(S, Q, X, B)
    return dict(mean=vegas.chain_complex(mean, F, R), stderr=vegas.chain_complex(err, F, R), acceptance=float(st["n_accept"].sum()) / (B * n_step),
                gamma=gamma, S=S, Q=Q, X=X, state=st)


def known_mz_mirror(n_root, eps, seed):
    k, kk = KNOWN_MZ, KNOWN_MZ["k"][eps]
    t, args, n_col, col, mz = known_mz_case(n_root)
    D = len(col)
    cin, cout = [3 + i - 1 for i in mz.root_tau_in], [3 + i - 1 for i in mz.root_tau_out]
    return mirror_chain_mz(known_mz_roots(n_root, kk), vegas.uniform_grid([0.0] * D, [k["beta"]] * D, k["n_grid"]), col, known_mz_fixed(n_root, kk),
                           n_root, mz.freq, True, 0, cin, cout, k["beta"], n_walker=k["n_walker"], n_step=k["n_step"], n_therm=k["n_therm"],
                           gamma_rel=k["gamma_rel"], seed=seed, coef=None if n_root == 1 else np.array(k["coef2"]))


def pulls(res, exact):
    """((mean - exact) / sigma) of the real parts and of the imaginary parts, [2, F, R]"""
    return np.stack([(res["mean"].real - exact.real) / res["stderr"].real, (res["mean"].imag - exact.imag) / res["stderr"].imag])


def test_closed_form_is_the_quadrature_of_the_leaf_oracle(libfdg):
    """sign and convention of the expected values: the textbook kernel against the oracle's own propagators, before anything trusts it"""
    for eps in (1.25, -1.25):
        k = KNOWN_MZ["k"][eps]
        assert abs(k * k - KNOWN_MZ["kF"] ** 2 - eps) < 1e-15
        q = quadrature(eps)
        want = np.array([closed_form(eps, n) for n in KNOWN_MZ["freq"]])
        print("eps", eps, "quadrature", q, "closed form", want)
        assert np.allclose(q, want, rtol=1e-10, atol=0)


@pytest.mark.parametrize("n_root", [1, 2])
def test_mirror_meets_the_conditions_of_the_gpu_tests(libfdg, n_root):
    """Conditions, not measurements: the GPU file asserts |mean - exact| <= 5 sigma per component at seed 0; the mirror alone must
    meet that, and over the seeds 0 .. 31 the sum of ((mean - exact) / sigma)^2 of every component must lie inside [10.3, 70.6].
    The values found are recorded in DESIGN 8l."""
    for eps in (1.25, -1.25):
        exact = known_mz_exact(n_root, eps)
        chi2, first = 0.0, None
        for seed in range(KNOWN_MZ["n_seed"]):
            r = known_mz_mirror(n_root, eps, seed)
            first = first or r
            chi2 = chi2 + pulls(r, exact) ** 2
        print("roots", n_root, "eps", eps, "seed 0 mean", first["mean"].ravel(), "stderr", first["stderr"].ravel(), "acceptance", first["acceptance"])
        print("chi2 over 32 seeds, real parts", chi2[0].ravel(), "imaginary parts", chi2[1].ravel())
        assert (np.abs(pulls(first, exact)) <= 5.0).all()
        assert ((CHI2_LO <= chi2) & (chi2 <= CHI2_HI)).all()
        assert 0.3 < first["acceptance"] < 1.0


def test_mirror_with_a_unit_phase_is_the_plain_mirror(libfdg):
    """fermionic = 0 and freq = [0]: the phase is exactly (0, 1), so the state is capi.chain_reference's bit for bit, the even columns
    of the sums are its sums and the odd ones stay zero"""
    t, col, fixed = known_graph()
    grid = vegas.uniform_grid([0, 0], [1, 1], 4)
    B, R, seed, gamma = 70, 2, 3, 0.05
    plain, mz = fresh_state(fixed, 2, R, B), fresh_state(fixed, 2, R, B)
    mz["sum"] = np.zeros((2 * R + 1, B))
    ev = oracle_roots(t)
    for i, (mask, flags) in enumerate([(3, INIT), (3, 0), (1, MEASURE), (2, MEASURE), (3, MEASURE)]):
        u, ua = step_uniforms(B, 2, mask, seed, i * B)
        plain = capi.chain_reference(grid, col, plain, mask, u, ua, gamma, flags, ev, [1.0, -0.5])
        mz = capi.chain_matsubara_reference(grid, col, mz, mask, u, ua, gamma, flags, ev, [0], False, 0, [col[0], col[1]], [col[1], col[0]], 2.0,
                                            [1.0, -0.5])
        for k in ("x", "fac", "root", "a", "n_accept"):
            assert np.array_equal(plain[k], mz[k]), (i, k)
        assert np.array_equal(mz["sum"][0:2 * R:2], plain["sum"][:R]) and np.array_equal(mz["sum"][2 * R], plain["sum"][R])
        assert (mz["sum"][1:2 * R:2] == 0.0).all()
    assert 0 < (plain["n_accept"] < 5).sum() and plain["sum"][R].min() > 0.0


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
        plain = protos[name.replace("_matsubara", "")][1]                     # the plain step's arguments, the descriptor before n_walker
        assert params[:len(plain) - 2] == plain[:-2] and params[-2:] == plain[-2:] and "fdg_chain_matsubara" in params[-3]
    for fn in ("chain_step_device_matsubara!", "mc_chain_step_device_matsubara!"):
        assert fn in export, fn
    import ctypes as C
    fields = [(n, C.sizeof(ty)) for n, ty in capi.ChainMatsubara._fields_]
    assert [n for n, _ in fields] == ["n_freq", "fermionic", "freq", "weight_freq", "root_col_in", "root_col_out", "beta"]
    assert C.sizeof(capi.ChainMatsubara) == 48 and capi.ChainMatsubara.root_col_in.offset == 24 and capi.ChainMatsubara.beta.offset == 40
    for h in (capi.GraphHandle.chain_step_device_matsubara, capi.GraphHandle.mc_chain_step_device_matsubara, capi.chain_matsubara_reference,
              capi.make_chain_matsubara, vegas.chain_complex):
        assert callable(h)


# ---- argument errors, no device present ----------------------------------------------------------------------------------------------- #
def mz_desc(R, n_col, **kw):
    """a valid descriptor of R roots over n_col columns with the fields of ``kw`` replaced (a None array: a NULL pointer)"""
    freq = kw.pop("freq", [0, 1, -3])
    cin, cout = kw.pop("cin", [0] * R), kw.pop("cout", [n_col - 1] * R)
    keep = [None if v is None else np.ascontiguousarray(v, dtype=dt) for v, dt in ((freq, np.int32), (cin, np.uint32), (cout, np.uint32))]
    ptr = [None if v is None else v.ctypes.data for v in keep]
    n_freq = kw.pop("n_freq", 0 if freq is None else len(freq))
    d = capi.ChainMatsubara(n_freq, kw.pop("fermionic", 1), ptr[0], kw.pop("weight_freq", 0), ptr[1], ptr[2], kw.pop("beta", 2.0))
    assert not kw
    return d, keep


MZ_INVALID = (dict(freq=None, n_freq=3), dict(cin=None), dict(cout=None), dict(n_freq=0), dict(weight_freq=3), dict(weight_freq=1 << 31),
              dict(beta=0.0), dict(beta=-1.0), dict(beta=math.inf), dict(beta=math.nan))


def _step_mz(h, desc, mc=False, d_xp=FAKE[0], xpc=100, d_facp=FAKE[1], n_col=None, n_dim=3, coef=None, gamma=0.5, flags=MEASURE, d_x=FAKE[2],
             xc=100, d_fac=FAKE[3], d_root=FAKE[4], d_a=FAKE[5], d_sum=FAKE[6], d_n_accept=FAKE[7], B=100):
    import ctypes as C
    if n_col is None:
        n_col = h.table.n_leaf if h is not None and not mc else 5
    c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    tail = (d_facp, n_col, n_dim, None if c is None else c.ctypes.data, gamma, 1, 0, flags, d_x, xc, d_fac, d_root, d_a, d_sum, d_n_accept,
            None if desc is None else C.addressof(desc), B, None)
    if mc:
        return capi.lib().fdg_mc_chain_step_device_matsubara(h._h if h else None, d_xp, xpc, 1.0, 2.0, 0.5, *tail)
    return capi.lib().fdg_chain_step_device_matsubara(h._h if h else None, d_xp, xpc, *tail)


def test_step_argument_checks_need_no_device(libfdg, tmp_path):
    t = workloads.get("sigma2")
    h = capi.GraphHandle(t)
    R, L = t.n_root, t.n_leaf
    good, _k = mz_desc(R, L)
    for mc in (False, True):
        n_col = 5 if mc else L
        ok, _k0 = mz_desc(R, n_col)
        # everything the plain step refuses
        for name in ("d_xp", "d_facp", "d_x", "d_fac", "d_root", "d_a", "d_sum"):
            assert failed(_step_mz(h, ok, mc, **{name: None}), capi.FDG_E_INVALID), name
        for kw in (dict(d_x=FAKE[0]), dict(d_n_accept=FAKE[6]), dict(gamma=0.0), dict(gamma=math.nan), dict(B=-1), dict(n_dim=0), dict(flags=4),
                   dict(xc=99), dict(xpc=99), dict(coef=[math.nan] * R)):
            assert failed(_step_mz(h, ok, mc, **kw), capi.FDG_E_INVALID), kw
        assert failed(_step_mz(None, ok, mc), capi.FDG_E_INVALID)
        assert failed(_step_mz(h, ok, mc, n_dim=capi.FDG_VEGAS_DIM_MAX + 1), capi.FDG_E_UNSUPPORTED)
        # the descriptor
        assert failed(_step_mz(h, None, mc), capi.FDG_E_INVALID)
        for kw in MZ_INVALID:
            d, _k1 = mz_desc(R, n_col, **kw)
            assert failed(_step_mz(h, d, mc), capi.FDG_E_INVALID), kw
            assert failed(_step_mz(h, d, mc, B=0), capi.FDG_E_INVALID), kw           # refused with nothing to do, too
        for kw in (dict(cin=[0] * (R - 1) + [n_col]), dict(cout=[n_col] + [0] * (R - 1)), dict(cin=[1 << 31] * R)):
            d, _k1 = mz_desc(R, n_col, **kw)
            assert failed(_step_mz(h, d, mc), capi.FDG_E_INVALID), kw
        d, _k1 = mz_desc(R, n_col, freq=list(range(capi.FDG_MATSUBARA_FREQ_MAX + 1)))
        assert failed(_step_mz(h, d, mc), capi.FDG_E_UNSUPPORTED)
    assert failed(_step_mz(h, good, n_col=L + 1), capi.FDG_E_INVALID)                # the leaf form: n_col is the number of leaves
    assert _step_mz(h, good, B=0) == capi.FDG_OK and _step_mz(h, good, B=0, flags=INIT, d_sum=None) == capi.FDG_OK
    d, _k1 = mz_desc(R, L, freq=list(range(capi.FDG_MATSUBARA_FREQ_MAX)), weight_freq=capi.FDG_MATSUBARA_FREQ_MAX - 1)
    assert _step_mz(h, d, B=0) == capi.FDG_OK                                        # 64 frequencies, the last one the weight's
    ok5, _k2 = mz_desc(R, 5)
    assert failed(_step_mz(h, ok5, True), capi.FDG_E_INVALID)                        # fdg_graph_specialize_fused has not been called
    # the Monte-Carlo form after fdg_graph_specialize_fused: two loops in two dimensions and one time are five columns
    a = fd.Graph([])
    t1, _, _ = lower([fd.Graph([a], subgraph_factors=[2.0])])
    tab, _keep = capi.make_leaf_tables([2], [2], [1], [1], [1], np.array([[1.0, -1.0]]), 2, 1)
    h1 = fd.compile_table(t1, specialize="isa", cache_dir=str(tmp_path)).handle
    h1.specialize_fused(tab, str(tmp_path))
    d1, _k3 = mz_desc(1, 5, cin=[4], cout=[4])
    assert failed(_step_mz(h1, d1, True, n_col=4), capi.FDG_E_INVALID) and _step_mz(h1, d1, True, n_col=5, B=0) == capi.FDG_OK
    with pytest.raises(capi.FdgError) as e:
        h.chain_step_device_matsubara(FAKE[0], 100, FAKE[1], L, 3, None, 0.5, 1, 0, MEASURE, FAKE[2], 100, FAKE[3], FAKE[4], FAKE[5], FAKE[6], 0,
                                      None, 100)
    assert e.value.code == capi.FDG_E_INVALID
    with pytest.raises(ValueError):
        capi.make_chain_matsubara([0], True, 0, [0, 1], [1], 2.0)


def test_a_missing_root_may_name_any_time_column(libfdg):
    from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT
    a, b = fd.Graph([]), fd.Graph([])
    g = fd.Graph([a, b], operator=fd.Prod())
    t, _, _ = lower([g], root=[g.id, 424_242])
    assert t.n_root == 2 and int(t.root_slot[1]) == FDG_NO_ROOT
    h = capi.GraphHandle(t)
    d, _k = mz_desc(2, t.n_leaf, cin=[0, 1 << 30], cout=[1, 77])
    assert _step_mz(h, d, B=0) == capi.FDG_OK
    d, _k = mz_desc(2, t.n_leaf, cin=[t.n_leaf, 0], cout=[1, 1])
    assert failed(_step_mz(h, d, B=0), capi.FDG_E_INVALID)


# ---- the estimate on the 2 F R + 1 layout ------------------------------------------------------------------------------------------------ #
def test_chain_estimate_and_the_complex_assembly_on_the_projected_layout():
    rng = np.random.default_rng(11)
    F, R, B = 3, 2, 400
    C = 2 * F * R
    A = rng.normal(size=(C + 1, B)) * rng.uniform(0.5, 3.0, size=(C + 1, 1))
    A[C] = rng.uniform(1.0, 3.0, size=B)
    red = capi.chain_reduce_reference(A)
    S, Q, X = red[:C + 1], red[C + 1:2 * C + 2], red[2 * C + 2:]
    mean, err = vegas.chain_estimate(S, Q, X, B)
    assert mean.shape == err.shape == (C,)
    zm, ze = vegas.chain_complex(mean, F, R), vegas.chain_complex(err, F, R)
    assert zm.shape == ze.shape == (F, R) and zm.dtype == np.complex128
    for f in range(F):
        for k in range(R):
            for part, c in ((0, 2 * (f * R + k)), (1, 2 * (f * R + k) + 1)):
                # by hand: the ratio of the sums and the delta method on the walkers' sample covariance of (A_c, A_C)
                m = A[c].sum() / A[C].sum()
                V = B * np.cov(np.stack([A[c], A[C]]), ddof=1)
                sd = math.sqrt((V[0, 0] - 2.0 * m * V[0, 1] + m * m * V[1, 1]) / A[C].sum() ** 2)
                got_m, got_e = (zm[f, k].real, ze[f, k].real) if part == 0 else (zm[f, k].imag, ze[f, k].imag)
                assert got_m == mean[c] and got_e == err[c]                     # the assembly: the very columns
                assert abs(got_m - m) <= 1e-13 * abs(m) and abs(got_e - sd) <= 1e-10 * sd, (f, k, part)
    e = np.arange(4.0)
    e[1] = np.nan                                            # a nan of one part stays in that part
    z = vegas.chain_complex(e, 1, 2)
    assert z[0, 0].real == 0.0 and np.isnan(z[0, 0].imag) and z[0, 1] == 2.0 + 3.0j


# ---- the driver ------------------------------------------------------------------------------------------------------------------------ #
def test_driver_argument_checks():
    h = capi.GraphHandle(workloads.get("sigma2"))
    R = h.table.n_root
    kw = dict(n_walker=64, n_step=4, n_therm=1, device="cpu", beta=2.0)
    good = vegas.MatsubaraProjection((0, 1), True, (1,) * R, (2,) * R)
    run = lambda **more: vegas.chain_integrate(h, None, [0, 0], [1, 1], [0, 1], **dict(kw, **more))
    assert "matsubara" not in vegas._CHAIN_EXCLUDED
    for bad in (vegas.MatsubaraProjection((), True, (1,) * R, (2,) * R), vegas.MatsubaraProjection(tuple(range(65)), True, (1,) * R, (2,) * R),
                vegas.MatsubaraProjection((0,), True, (1,), (2,) * R), vegas.MatsubaraProjection((0,), True, (0,) * R, (2,) * R),
                vegas.MatsubaraProjection((0,), True, (1,) * R, (h.table.n_leaf + 1,) * R), object()):
        with pytest.raises(ValueError, match="matsubara"):
            run(matsubara=bad)
    for wf in (-1, 2):
        with pytest.raises(ValueError, match="weight_freq"):
            run(matsubara=good, weight_freq=wf)
    with pytest.raises(ValueError, match="beta"):
        run(matsubara=good, beta=0.0)
    # what stays refused, with the projection too
    for name, value in (("polar", [vegas.PolarVar(0, (0, 1, 2))]), ("groups", vegas.WeightGroups([0], [[0]])), ("dmap", object()),
                        ("observables", object()), ("freq_observables", object()), ("strat", vegas.Stratification((1, 1)))):
        with pytest.raises(ValueError, match=name):
            run(matsubara=good, **{name: value})
    with pytest.raises(ValueError):
        run(matsubara=good, n_therm=4)                       # the plain checks still run
