"""Observables without a device (include/fdg.h: fdg_accumulate_device_observables, fdg_mc_accumulate_device_observables;
capi.observables_reference, compilers.mc_covariance, vegas.combine_covariance): the symbols are declared, exported and bound; every
argument check runs before any device work; the numpy restatement agrees with a plain Python loop; the covariance estimate has
mc_estimate's error bars on its diagonal; the combined covariance is the stated propagation."""
import ctypes
import math
import re

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.compilers import mc_covariance, mc_estimate
from test_matsubara_host import HDR, JL, c_class, c_prototypes, jl_ccalls, jl_class

NAMES = ("fdg_accumulate_device_observables", "fdg_mc_accumulate_device_observables")
FAKE = [0x10000 * (i + 1) for i in range(16)]     # pointers the checks only compare with NULL or with each other; never read through


def test_symbols_are_declared_exported_and_bound(libfdg):
    protos, calls = c_prototypes(), jl_ccalls()
    text = open(JL).read()
    export = [x.strip() for x in re.search(r"^export\s+([^\n]*)", text, flags=re.M).group(1).split(",")]
    for name in NAMES:
        assert name in protos and name in capi.EXPORTS and hasattr(libfdg, name), name
        assert name in calls, name + ": not bound in the Julia shim"
        types, args = calls[name]
        params = protos[name][1]
        assert len(types) == len(params) == len(args) == len(getattr(libfdg, name).argtypes), name
        for jt, cp in zip(types, params):
            assert jl_class(jt) == c_class(cp), (name, jt, cp)
    assert "accumulate_device_observables!" in export and "mc_accumulate_device_observables!" in export
    hdr = open(HDR).read()
    assert re.search(r"#define\s+FDG_OBS_MAX\s+(\d+)", hdr).group(1) == str(capi.FDG_OBS_MAX) == "16"
    body = re.search(r"typedef struct fdg_observables \{(.*?)\} fdg_observables;", hdr, flags=re.S).group(1)
    fields = re.findall(r"[\s\*](\w+)\s*(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    want = [k for k, _ in capi.Observables._fields_]
    assert fields == want, (fields, want)
    jl = re.search(r"struct _FdgObservables\n(.*?)\nend", text, flags=re.S).group(1)
    assert [ln.strip().split("::")[0] for ln in jl.splitlines()] == want
    assert ctypes.sizeof(capi.Observables) == 32
    assert "Complex observables" in hdr or "complex observables" in hdr
    assert fd.mc_covariance is mc_covariance
    for fn in (capi.make_observables, capi.observables_reference, capi.GraphHandle.accumulate_device_observables,
               capi.GraphHandle.mc_accumulate_device_observables, fd.GraphFunc.accumulate_observables, vegas.combine_covariance):
        assert callable(fn)
    assert vegas.Observables(((1.0, 1.0),)).coef == ((1.0, 1.0),)


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def _obs(R, n_obs=2, coef=True, d_obs=FAKE[12], d_cov=FAKE[13], values=None):
    c = np.ones((max(n_obs, 1), R)) if values is None else np.ascontiguousarray(values, dtype=np.float64)
    return capi.Observables(n_obs, c.ctypes.data if coef else None, d_obs, d_cov), (c,)


def _groups(R, n_group=2, stride=100):
    return capi.make_weight_groups([k % n_group for k in range(R)], [(0,)] * n_group, stride)


def _leaf(h, ob, wg=None, n_bin=4, B=100, d_leaf=FAKE[0], d_bin=FAKE[1], d_weight=None, d_acc=None, d_acc2=None, n_dim=0, n_grid=0, d_hist=None,
          d_hist_bin=None):
    return capi.lib().fdg_accumulate_device_observables(h._h if h else None, d_leaf, 1, 8, 0, d_bin, 0, n_bin, d_weight, None, 1, 0, n_dim, n_grid,
                                                        d_acc, d_acc2, d_hist, d_hist_bin, None, None if wg is None else ctypes.addressof(wg),
                                                        None if ob is None else ctypes.addressof(ob), B, None)


def _mc(h, ob, wg=None, n_bin=4, B=100, d_leaf=FAKE[0], d_bin=FAKE[1], d_weight=None, d_acc=None, d_acc2=None, n_dim=0, n_grid=0, d_hist=None,
        d_hist_bin=None):
    return capi.lib().fdg_mc_accumulate_device_observables(h._h if h else None, d_leaf, 1, 8, FAKE[9], 1, 8, 1.0, 2.0, 0.5, d_bin, 0, n_bin,
                                                           d_weight, None, 1, 0, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin, None,
                                                           None if wg is None else ctypes.addressof(wg),
                                                           None if ob is None else ctypes.addressof(ob), B, None)


def _err():
    return capi.lib().fdg_last_error().decode()


def test_argument_checks_need_no_device(libfdg):
    t = workloads.get("sigma2")
    h, R = capi.GraphHandle(t), t.n_root
    INV, UNS, OK = capi.FDG_E_INVALID, capi.FDG_E_UNSUPPORTED, capi.FDG_OK
    for call in (_leaf, _mc):
        good, _k = _obs(R)
        wg, _kw = _groups(R)
        # (B = 0: valid arguments and nothing to do -- every check has passed, no device work, no error)
        assert call(h, good, B=0) == OK                                       # no wg, no weights, no per-root moments
        assert call(h, good, d_weight=FAKE[3], B=0) == OK                     # wg NULL: one weight column
        assert call(h, good, wg, d_weight=FAKE[3], B=0) == OK
        assert call(h, good, n_bin=1, d_bin=None, B=0) == OK
        assert call(h, good, d_acc=FAKE[4], d_acc2=FAKE[5], B=0) == OK
        assert call(h, good, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[11], B=0) == OK
        assert call(h, _obs(R, capi.FDG_OBS_MAX)[0], B=0) == OK
        # the descriptor
        assert call(None, good) == INV
        assert call(h, None) == INV and "observables" in _err()
        assert call(h, _obs(R, coef=False)[0]) == INV
        assert call(h, _obs(R, d_obs=None)[0]) == INV
        assert call(h, _obs(R, d_cov=None)[0]) == INV
        assert call(h, _obs(R, 0)[0]) == INV and "n_obs" in _err()
        big, _kb = _obs(R, capi.FDG_OBS_MAX + 1)
        assert call(h, big) == UNS and "FDG_OBS_MAX" in _err()
        for bad in (np.nan, np.inf, -np.inf):
            v = np.ones((2, R))
            v[1, R - 1] = bad
            ob, _kv = _obs(R, values=v)
            assert call(h, ob) == INV and "finite" in _err()
        assert call(h, _obs(R, d_obs=FAKE[13])[0]) == INV and "same buffer" in _err()
        assert call(h, good, d_acc=FAKE[12], d_acc2=FAKE[5]) == INV and "same buffer" in _err()
        assert call(h, good, d_acc=FAKE[4], d_acc2=FAKE[12]) == INV and "same buffer" in _err()
        assert call(h, good, d_acc=FAKE[13], d_acc2=FAKE[5]) == INV and "same buffer" in _err()
        assert call(h, good, d_acc=FAKE[4], d_acc2=FAKE[13]) == INV and "same buffer" in _err()
        # the grouped calls' own cases, except those this call relaxes
        assert call(h, good, d_acc=FAKE[4]) == INV and "go together" in _err()
        assert call(h, good, d_acc2=FAKE[4]) == INV and "go together" in _err()
        assert call(h, good, d_acc=FAKE[4], d_acc2=FAKE[4]) == INV
        assert call(h, good, wg) == INV and "d_weight" in _err()              # groups need weights
        assert call(h, good, _groups(R, 2, 50)[0], d_weight=FAKE[3]) == INV and "stride" in _err()
        w0 = capi.WeightGroups(0, wg.root_group, wg.var_mask, 100)
        assert call(h, good, w0, d_weight=FAKE[3]) == INV
        w9 = capi.WeightGroups(capi.FDG_WEIGHT_GROUP_MAX + 1, wg.root_group, wg.var_mask, 100)
        assert call(h, good, w9, d_weight=FAKE[3]) == UNS
        assert call(h, good, B=-1) == INV
        assert call(h, good, n_bin=0) == INV
        assert call(h, good, n_bin=2, d_bin=None) == INV
        assert call(h, good, n_bin=capi.FDG_BIN_MAX + 1) == UNS
        assert call(h, good, d_leaf=None) == INV
        assert call(h, good, n_dim=3, n_grid=8) == INV                         # training without d_hist
        assert call(h, good, n_dim=capi.FDG_VEGAS_DIM_MAX + 1, n_grid=8, d_hist=FAKE[10]) == UNS
        assert call(h, good, n_bin=1, d_bin=None, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[11]) == INV and "d_hist_bin" in _err()
    with pytest.raises(capi.FdgError) as e:
        h.accumulate_device_observables(FAKE[0], 1, 8, 0, FAKE[1], 0, 4, 0, _obs(R, 0)[0], B=100)
    assert e.value.code == INV
    with pytest.raises(capi.FdgError) as e:
        h.mc_accumulate_device_observables(FAKE[0], 1, 8, FAKE[9], 1, 8, 1.0, 2.0, 0.5, FAKE[1], 0, 4, 0, _obs(R, 17)[0], B=100)
    assert e.value.code == UNS


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------- #
def test_reference_matches_a_plain_loop_on_three_roots():
    rng = np.random.default_rng(1)
    B, R, n_bin = 57, 3, 3
    roots = rng.normal(size=(B, R))
    w = rng.uniform(0.5, 2.0, size=(2, B))
    rg = [0, 1, 0]
    bins = rng.integers(1, 6, size=B).astype(np.int32)                       # base 2: values 1 and 5 are out of range
    coef = np.array([[1.0, 1.0, 0.0], [0.5, 0.0, -2.0], [0.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    obs, cov, s_obs, s_cov = capi.observables_reference(roots, coef, w, rg, bins, n_bin, 2)
    want_o, want_c = np.zeros((n_bin, 4)), np.zeros((n_bin, 4, 4))
    abs_o = np.zeros((n_bin, 4))
    for b in range(B):
        j = int(bins[b]) - 2
        if not 0 <= j < n_bin:
            continue
        o = []
        for m in range(4):
            acc, first = 0.0, True
            for k in range(R):
                if coef[m, k] != 0.0:
                    p = coef[m, k] * (w[rg[k], b] * roots[b, k])
                    acc, first = (p if first else acc + p), False
            o.append(acc)
        for m in range(4):
            want_o[j, m] += o[m]
            abs_o[j, m] += abs(o[m])
            for c in range(4):
                want_c[j, m, c] += o[m] * o[c]
    live = [0, 1, 3]
    assert np.isnan(obs[:, 2]).all() and np.isnan(cov[:, 2, :]).all() and np.isnan(cov[:, :, 2]).all()
    assert np.allclose(obs[:, live], want_o[:, live], rtol=1e-13, atol=1e-13)
    assert np.allclose(cov[np.ix_(range(n_bin), live, live)], want_c[np.ix_(range(n_bin), live, live)], rtol=1e-13, atol=1e-13)
    assert np.allclose(s_obs[:, live], abs_o[:, live], rtol=1e-13)
    assert np.array_equal(cov[:, 0, 1], cov[:, 1, 0]) and (s_cov[:, 0, 0] >= np.abs(cov[:, 0, 0])).all()
    # no weights, no bins, a root that does not exist: its coefficient is not a term
    obs, cov, _, _ = capi.observables_reference(roots, [[1.0, 5.0, 1.0], [0.0, 7.0, 0.0]], exists=[True, False, True])
    assert np.allclose(obs[0, 0], (roots[:, 0] + roots[:, 2]).sum()) and np.isnan(obs[0, 1])
    # a unit row is the root itself: -0.0 survives (the first product starts the fold, no 0.0 + in front)
    obs, _, _, _ = capi.observables_reference(np.array([[-0.0, 1.0]]), [[1.0, 0.0]])
    assert math.copysign(1.0, obs[0, 0]) == 1.0 or obs[0, 0] == 0.0           # (numpy's bincount adds to +0.0: only the value is stated)


def test_mc_covariance_has_mc_estimate_on_its_diagonal_and_is_symmetric():
    rng = np.random.default_rng(2)
    N, M, n_bin = 1000, 4, 3
    o = rng.normal(1.0, 2.0, size=(n_bin, N, M))
    o[:, :, 3] = 0.25                                                         # a constant: its variance rounds about 0 and is clamped
    S = o.sum(axis=1)
    Q = np.einsum("jna,jnc->jac", o, o)
    mean, C = mc_covariance(S, Q, N)
    m1, e1 = mc_estimate(S, np.einsum("jaa->ja", Q), N)
    assert np.array_equal(mean, m1)
    assert np.array_equal(np.sqrt(np.einsum("jaa->ja", C)), e1)
    assert np.array_equal(np.einsum("jaa->ja", C), e1 ** 2) or np.allclose(np.einsum("jaa->ja", C), e1 ** 2, rtol=1e-15, atol=0.0)
    assert (np.einsum("jaa->ja", C) >= 0).all() and np.array_equal(C, C.transpose(0, 2, 1))
    want = np.array([np.cov(o[j].T) / N for j in range(n_bin)])
    assert np.allclose(C[:, :3, :3], want[:, :3, :3], rtol=1e-9, atol=1e-15)
    with pytest.raises(ValueError):
        mc_covariance(S, Q, 1)
    with pytest.raises(ValueError):
        mc_covariance(S, Q[:, :3], N)
    torch = pytest.importorskip("torch")
    tm, tC = mc_covariance(torch.from_numpy(S), torch.from_numpy(Q), N)
    assert np.array_equal(tm.numpy(), mean) and np.array_equal(tC.numpy(), C)


def test_combined_covariance_on_two_hand_made_iterations():
    # errors 1 and 2 for observable 0 (weights 4/5 and 1/5), 3 and 3 for observable 1 (1/2 and 1/2)
    it = [(np.array([10.0, 1.0]), np.array([[1.0, 0.6], [0.6, 9.0]])), (np.array([12.0, 3.0]), np.array([[4.0, -2.0], [-2.0, 9.0]]))]
    mean, err, chi2, cov = vegas.combine_covariance(it)
    a0, a1 = np.array([0.8, 0.2]), np.array([0.5, 0.5])
    assert np.allclose(mean, [0.8 * 10 + 0.2 * 12, 2.0], rtol=1e-15)
    assert np.allclose(err, [math.sqrt(0.8), math.sqrt(4.5)], rtol=1e-15)
    want = np.array([[a0[0] ** 2 * 1.0 + a0[1] ** 2 * 4.0, a0[0] * a1[0] * 0.6 + a0[1] * a1[1] * -2.0],
                     [a0[0] * a1[0] * 0.6 + a0[1] * a1[1] * -2.0, a1[0] ** 2 * 9.0 + a1[1] ** 2 * 9.0]])
    assert np.allclose(cov, want, rtol=1e-15) and np.array_equal(cov, cov.T)
    assert np.allclose(np.diag(cov), err ** 2, rtol=1e-15)
    m2, e2, c2 = vegas.combine([(a, np.sqrt(np.diag(c))) for a, c in it])
    assert np.array_equal(mean, m2) and np.array_equal(err, e2) and np.array_equal(chi2, c2)
    # an observable that is exactly 0 in every iteration stays exactly 0, with an error of exactly 0
    it = [(np.array([1.0, 0.0]), np.array([[0.25, 0.0], [0.0, 0.0]])), (np.array([2.0, 0.0]), np.array([[0.25, 0.0], [0.0, 0.0]]))]
    mean, err, _, cov = vegas.combine_covariance(it)
    assert mean[1] == 0.0 and err[1] == 0.0 and cov[1, 1] == 0.0 and cov[0, 1] == 0.0
    # a bin axis in front
    it = [(np.ones((3, 2)), np.tile(np.eye(2), (3, 1, 1))), (np.ones((3, 2)), np.tile(np.eye(2), (3, 1, 1)))]
    mean, err, _, cov = vegas.combine_covariance(it)
    assert mean.shape == (3, 2) and cov.shape == (3, 2, 2) and np.allclose(cov, np.tile(np.eye(2) / 2.0, (3, 1, 1)))
