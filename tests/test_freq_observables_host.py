"""Frequency observables without a device (include/fdg.h: fdg_accumulate_device_freq_observables,
fdg_mc_accumulate_device_freq_observables; capi.freq_observables_reference, vegas.FrequencyObservables, vegas.complex_components):
the symbols are declared, exported and bound in ctypes and in the Julia shim; every argument check runs before any device work and
leaves a telling fdg_last_error; the accepted optional combinations pass; the numpy restatement agrees with a plain Python loop; the
driver refuses what it must; the complex fields are assembled from the 2 M components as stated."""
import ctypes
import re

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from test_matsubara_host import HDR, JL, c_class, c_prototypes, jl_ccalls, jl_class

NAMES = ("fdg_accumulate_device_freq_observables", "fdg_mc_accumulate_device_freq_observables")
FAKE = [0x10000 * (i + 1) for i in range(24)]     # pointers the checks only compare with NULL or with each other; never read through


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
        # the arguments of the _observables call plus fo, placed after ob
        base = protos[name.replace("freq_", "")][1]
        at = [i for i, p in enumerate(base) if p.endswith("*ob")][0]
        assert [c_class(p) for p in params] == [c_class(p) for p in base[:at + 1]] + ["pointer"] + [c_class(p) for p in base[at + 1:]]
        assert "fdg_freq_observables" in params[at + 1] and params[at + 1].endswith("*fo")
    assert "accumulate_device_freq_observables!" in export and "mc_accumulate_device_freq_observables!" in export
    hdr = open(HDR).read()
    assert re.search(r"#define\s+FDG_FREQ_OBS_MAX\s+(\d+)", hdr).group(1) == str(capi.FDG_FREQ_OBS_MAX) == "8"
    assert 2 * capi.FDG_FREQ_OBS_MAX <= capi.FDG_OBS_MAX                      # 2 M components: the observables pass's largest shape
    body = re.search(r"typedef struct fdg_freq_observables \{(.*?)\} fdg_freq_observables;", hdr, flags=re.S).group(1)
    fields = re.findall(r"[\s\*](\w+)\s*(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    want = [k for k, _ in capi.FreqObservables._fields_]
    assert fields == want == ["n_obs", "coef", "d_fobs", "d_fcov"], (fields, want)
    jl = re.search(r"struct _FdgFreqObservables\n(.*?)\nend", text, flags=re.S).group(1)
    assert [ln.strip().split("::")[0] for ln in jl.splitlines()] == want
    assert ctypes.sizeof(capi.FreqObservables) == 32 == ctypes.sizeof(capi.Observables)
    for fn in (capi.make_freq_observables, capi.freq_observables_reference, capi.matsubara_phase_table,
               capi.GraphHandle.accumulate_device_freq_observables, capi.GraphHandle.mc_accumulate_device_freq_observables,
               fd.GraphFunc.accumulate_freq_observables, vegas.complex_components):
        assert callable(fn)
    assert vegas.FrequencyObservables(((1.0, 1.0),)).coef == ((1.0, 1.0),)
    fo, keep = capi.make_freq_observables([[1.0, 2.0], [0.0, 3.0], [4.0, 0.0]], FAKE[0], FAKE[1])
    assert (fo.n_obs, fo.d_fobs, fo.d_fcov) == (3, FAKE[0], FAKE[1]) and fo.coef == keep[0].ctypes.data
    with pytest.raises(ValueError):
        capi.make_freq_observables([1.0, 2.0], FAKE[0], FAKE[1])


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def _fo(R, n_obs=2, coef=True, d_fobs=FAKE[14], d_fcov=FAKE[15], values=None):
    c = np.ones((max(n_obs, 1), R)) if values is None else np.ascontiguousarray(values, dtype=np.float64)
    return capi.FreqObservables(n_obs, c.ctypes.data if coef else None, d_fobs, d_fcov), (c,)


def _ob(R, d_obs=FAKE[12], d_cov=FAKE[13]):
    c = np.ones((2, R))
    return capi.Observables(2, c.ctypes.data, d_obs, d_cov), (c,)


def _mz(R, arrays=(FAKE[5], FAKE[6], FAKE[7], FAKE[8]), n_freq=3, d_T=FAKE[9]):
    return capi.make_matsubara(list(range(n_freq)), True, [1] * R, [2] * R, 2.0, 2, *arrays, d_T, 2, 1)


def _groups(R, n_group=2, stride=100):
    return capi.make_weight_groups([k % n_group for k in range(R)], [(0,)] * n_group, stride)


def _addr(x):
    return None if x is None else ctypes.addressof(x)


def _leaf(h, fo, mz, ob=None, wg=None, n_bin=4, B=100, d_leaf=FAKE[0], d_bin=FAKE[1], d_weight=None, d_acc=None, d_acc2=None, n_dim=0, n_grid=0,
          d_hist=None, d_hist_bin=None):
    return capi.lib().fdg_accumulate_device_freq_observables(h._h if h else None, d_leaf, 1, 8, 0, d_bin, 0, n_bin, d_weight, None, 1, 0, n_dim,
                                                             n_grid, d_acc, d_acc2, d_hist, d_hist_bin, _addr(mz), _addr(wg), _addr(ob),
                                                             _addr(fo), B, None)


def _mc(h, fo, mz, ob=None, wg=None, n_bin=4, B=100, d_leaf=FAKE[0], d_bin=FAKE[1], d_weight=None, d_acc=None, d_acc2=None, n_dim=0, n_grid=0,
        d_hist=None, d_hist_bin=None):
    return capi.lib().fdg_mc_accumulate_device_freq_observables(h._h if h else None, d_leaf, 1, 8, FAKE[9], 1, 8, 1.0, 2.0, 0.5, d_bin, 0, n_bin,
                                                                d_weight, None, 1, 0, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin,
                                                                _addr(mz), _addr(wg), _addr(ob), _addr(fo), B, None)


def _err():
    return capi.lib().fdg_last_error().decode()


def test_argument_checks_need_no_device(libfdg):
    t = workloads.get("sigma2")
    h, R = capi.GraphHandle(t), t.n_root
    INV, UNS, OK = capi.FDG_E_INVALID, capi.FDG_E_UNSUPPORTED, capi.FDG_OK
    for call in (_leaf, _mc):
        good, _k = _fo(R)
        mz, _km = _mz(R)
        bare, _kb = _mz(R, arrays=(0, 0, 0, 0))
        ob, _ko = _ob(R)
        wg, _kw = _groups(R)
        # (B = 0: valid arguments and nothing to do -- every check has passed, no device work, no error)
        assert call(h, good, mz, B=0) == OK                                   # ob NULL, wg NULL, no weights, no per-root moments
        assert call(h, good, bare, B=0) == OK                                 # mz's four arrays all NULL: no per-root projection
        assert call(h, good, mz, ob, B=0) == OK
        assert call(h, good, mz, ob, wg, d_weight=FAKE[3], B=0) == OK
        assert call(h, good, mz, None, wg, d_weight=FAKE[3], B=0) == OK       # ob NULL beside groups
        assert call(h, good, mz, ob, d_weight=FAKE[3], B=0) == OK             # wg NULL: one weight column
        assert call(h, good, mz, n_bin=1, d_bin=None, B=0) == OK              # d_bin NULL with one bin
        assert call(h, good, mz, d_acc=FAKE[4], d_acc2=FAKE[2], B=0) == OK
        assert call(h, good, mz, ob, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[11], B=0) == OK
        assert call(h, _fo(R, capi.FDG_FREQ_OBS_MAX)[0], mz, B=0) == OK
        # the descriptor
        assert call(None, good, mz) == INV
        assert call(h, None, mz) == INV and "frequency observables" in _err()
        assert call(h, _fo(R, coef=False)[0], mz) == INV and "frequency observables" in _err()
        assert call(h, _fo(R, d_fobs=None)[0], mz) == INV and "frequency observables" in _err()
        assert call(h, _fo(R, d_fcov=None)[0], mz) == INV and "frequency observables" in _err()
        assert call(h, _fo(R, 0)[0], mz) == INV and "n_obs" in _err()
        big, _kbig = _fo(R, capi.FDG_FREQ_OBS_MAX + 1)
        assert call(h, big, mz) == UNS and "FDG_FREQ_OBS_MAX" in _err()
        for bad in (np.nan, np.inf, -np.inf):
            v = np.ones((2, R))
            v[1, R - 1] = bad
            assert call(h, _fo(R, values=v)[0], mz) == INV and "finite" in _err()
        # the projection it stands on
        assert call(h, good, None) == INV and "mz" in _err()
        for i in range(4):
            some = [FAKE[5], FAKE[6], FAKE[7], FAKE[8]]
            some[i] = 0
            assert call(h, good, _mz(R, arrays=some)[0]) == INV and "some but not all" in _err(), i
        assert call(h, good, _mz(R, arrays=(FAKE[5], 0, 0, 0))[0]) == INV and "some but not all" in _err()
        many, _kmany = _mz(R, n_freq=5)
        assert call(h, good, many, n_bin=capi.FDG_BIN_MAX // 4) == UNS and "n_bin * n_freq" in _err()
        # d_fobs or d_fcov the same buffer as any other output of the call
        assert call(h, _fo(R, d_fobs=FAKE[15])[0], mz) == INV and "same buffer" in _err()
        for mine in ("d_fobs", "d_fcov"):
            for other in (FAKE[5], FAKE[6], FAKE[7], FAKE[8]):                  # the four arrays of mz
                assert call(h, _fo(R, **{mine: other})[0], mz) == INV and "same buffer" in _err(), (mine, other)
            for other in (FAKE[12], FAKE[13]):                                  # ob's arrays
                assert call(h, _fo(R, **{mine: other})[0], mz, ob) == INV and "same buffer" in _err(), (mine, other)
            alias = _fo(R, **{mine: FAKE[20]})[0]
            assert call(h, alias, mz, d_acc=FAKE[20], d_acc2=FAKE[2]) == INV and "same buffer" in _err()
            assert call(h, alias, mz, d_acc=FAKE[4], d_acc2=FAKE[20]) == INV and "same buffer" in _err()
            assert call(h, alias, mz, n_dim=3, n_grid=8, d_hist=FAKE[20]) == INV and "same buffer" in _err()
            assert call(h, alias, mz, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[20]) == INV and "same buffer" in _err()
        # the _observables calls' own cases
        assert call(h, good, mz, _ob(R, d_obs=None)[0]) == INV and "observables" in _err()
        assert call(h, good, mz, _ob(R, d_obs=FAKE[13])[0]) == INV and "same buffer" in _err()
        assert call(h, good, mz, d_acc=FAKE[4]) == INV and "go together" in _err()
        assert call(h, good, mz, ob, d_acc2=FAKE[4]) == INV and "go together" in _err()
        assert call(h, good, mz, ob, wg) == INV and "d_weight" in _err()      # groups need weights
        assert call(h, good, mz, None, _groups(R, 2, 50)[0], d_weight=FAKE[3]) == INV and "stride" in _err()
        w9 = capi.WeightGroups(capi.FDG_WEIGHT_GROUP_MAX + 1, wg.root_group, wg.var_mask, 100)
        assert call(h, good, mz, ob, w9, d_weight=FAKE[3]) == UNS
        assert call(h, good, mz, B=-1) == INV
        assert call(h, good, mz, n_bin=0) == INV
        assert call(h, good, mz, n_bin=2, d_bin=None) == INV
        assert call(h, good, mz, n_bin=capi.FDG_BIN_MAX + 1) == UNS
        assert call(h, good, mz, d_leaf=None) == INV
        assert call(h, good, mz, n_dim=3, n_grid=8) == INV                     # training without d_hist
        assert call(h, good, mz, n_dim=capi.FDG_VEGAS_DIM_MAX + 1, n_grid=8, d_hist=FAKE[10]) == UNS
        assert call(h, good, mz, n_bin=1, d_bin=None, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[11]) == INV and "d_hist_bin" in _err()
        late, _kl = capi.make_matsubara([0], True, [1] * R, [3] * R, 2.0, 2, 0, 0, 0, 0, FAKE[9], 2, 1)
        assert call(h, good, late) == INV and "time label" in _err()
    # the existing calls still ask for all four arrays
    bare, _kb = _mz(R, arrays=(0, 0, 0, 0))
    assert capi.lib().fdg_accumulate_device_matsubara(h._h, FAKE[0], 1, 8, 0, FAKE[1], 0, 4, None, None, 1, 0, 0, 0, None, None, None, None,
                                                      ctypes.addressof(bare), 0, None) == INV
    with pytest.raises(capi.FdgError) as e:
        h.accumulate_device_freq_observables(FAKE[0], 1, 8, 0, FAKE[1], 0, 4, 0, _fo(R, 0)[0], _mz(R)[0], B=100)
    assert e.value.code == INV
    with pytest.raises(capi.FdgError) as e:
        h.mc_accumulate_device_freq_observables(FAKE[0], 1, 8, FAKE[9], 1, 8, 1.0, 2.0, 0.5, FAKE[1], 0, 4, 0, _fo(R, 9)[0], _mz(R)[0], B=100)
    assert e.value.code == UNS


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------- #
def test_reference_matches_a_plain_loop(libfdg):
    rng = np.random.default_rng(1)
    B, R, n_bin, beta = 57, 4, 3, 2.5
    roots = rng.normal(size=(B, R))
    T = rng.uniform(0.0, beta, size=(B, 3))
    tin, tout = [1, 1, 2, 1], [2, 3, 2, 2]                                    # roots 0 and 3 share a pair; root 2's times coincide
    w = rng.uniform(0.5, 2.0, size=(2, B))
    rg = [0, 1, 0, 1]
    bins = rng.integers(1, 6, size=B).astype(np.int32)                       # base 2: values 1 and 5 are out of range
    coef = np.array([[1.0, 1.0, 0.0, 1.0], [0.5, 0.0, -2.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    M = coef.shape[0]
    for fermionic, freq in ((True, (0, -2, 3)), (False, (0, 1))):
        F = len(freq)
        fobs, fcov, s_obs, s_cov = capi.freq_observables_reference(roots, T, tin, tout, freq, beta, fermionic, coef, w, rg, bins, n_bin, 2)
        assert fobs.shape == s_obs.shape == (n_bin, F, 2 * M) and fcov.shape == s_cov.shape == (n_bin, F, 2 * M, 2 * M)
        want_o, want_c, abs_o = np.zeros((n_bin, F, 2 * M)), np.zeros((n_bin, F, 2 * M, 2 * M)), np.zeros((n_bin, F, 2 * M))
        for b in range(B):
            j = int(bins[b]) - 2
            if not 0 <= j < n_bin:
                continue
            for f, n in enumerate(freq):
                z = [0.0] * (2 * M)
                for m in range(M):
                    first = True
                    for k in range(R):
                        if coef[m, k] != 0.0:
                            t = w[rg[k], b] * roots[b, k]
                            s, c = capi.matsubara_phase(float(T[b, tout[k] - 1] - T[b, tin[k] - 1]), beta, n, fermionic)
                            pa, pb = coef[m, k] * (t * c), coef[m, k] * (t * s)
                            z[m], z[M + m], first = (pa, pb, False) if first else (z[m] + pa, z[M + m] + pb, False)
                for p in range(2 * M):
                    want_o[j, f, p] += z[p]
                    abs_o[j, f, p] += abs(z[p])
                    for q in range(2 * M):
                        want_c[j, f, p, q] += z[p] * z[q]
        live = [0, 1, 3, 4]                                                   # row 2 has no term: components 2 and 5
        assert np.isnan(fobs[:, :, [2, 5]]).all() and np.isnan(fcov[:, :, [2, 5], :]).all() and np.isnan(fcov[:, :, :, [2, 5]]).all()
        assert np.allclose(fobs[:, :, live], want_o[:, :, live], rtol=1e-13, atol=1e-13)
        ix = np.ix_(range(n_bin), range(F), live, live)
        assert np.allclose(fcov[ix], want_c[ix], rtol=1e-13, atol=1e-13)
        assert np.allclose(s_obs[:, :, live], abs_o[:, :, live], rtol=1e-13)
        assert np.array_equal(fcov[ix], fcov[ix].transpose(0, 1, 3, 2)) and (s_cov[:, :, 0, 0] >= np.abs(fcov[:, :, 0, 0])).all()
    # a bosonic n = 0 has the phase (0, 1) exactly: the imaginary components are 0 and the real ones the unprojected observables
    fobs, fcov, _, _ = capi.freq_observables_reference(roots, T, tin, tout, (0,), beta, False, coef[:2], w, rg, bins, n_bin, 2)
    obs, cov, _, _ = capi.observables_reference(roots, coef[:2], w, rg, bins, n_bin, 2)
    assert (fobs[:, 0, 2:] == 0.0).all() and (fcov[:, 0, 2:, :] == 0.0).all() and (fcov[:, 0, :, 2:] == 0.0).all()
    assert np.allclose(fobs[:, 0, :2], obs, rtol=1e-13, atol=1e-13) and np.allclose(fcov[:, 0, :2, :2], cov, rtol=1e-13, atol=1e-13)
    # no weights, no bins, a root that does not exist: its coefficient is not a term; ready-made phase tables give the same bits
    ex = [True, False, True, True]
    a = capi.freq_observables_reference(roots, T, tin, tout, (1, 2), beta, True, [[1.0, 5.0, 1.0, 0.0], [0.0, 7.0, 0.0, 0.0]], exists=ex)
    assert np.isnan(a[0][0, :, [1, 3]]).all() and np.isfinite(a[0][0, :, [0, 2]]).all()
    tables = {(1, 2): capi.matsubara_phase_table(T[:, 1] - T[:, 0], beta, (1, 2), True),
              (2, 2): capi.matsubara_phase_table(T[:, 1] - T[:, 1], beta, (1, 2), True)}
    b = capi.freq_observables_reference(roots, T, tin, tout, (1, 2), beta, True, [[1.0, 5.0, 1.0, 0.0], [0.0, 7.0, 0.0, 0.0]], exists=ex,
                                        phases=tables)
    assert np.array_equal(a[0][:, :, [0, 2]], b[0][:, :, [0, 2]])
    s, c = tables[(1, 2)]
    assert (s[5, 1], c[5, 1]) == capi.matsubara_phase(float(T[5, 1] - T[5, 0]), beta, 2, True)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------ #
def test_driver_refusals():
    fo = vegas.FrequencyObservables(((1.0,),))
    args = (object(), None, [0, 0], [1, 1], [0, 1])
    with pytest.raises(ValueError, match="freq_observables needs matsubara"):
        vegas.vegas_integrate(*args, freq_observables=fo)
    with pytest.raises(ValueError, match="freq_observables needs matsubara"):
        vegas.vegas_integrate_binned(*args, object(), freq_observables=fo)
    mz = vegas.MatsubaraProjection((0,), True, (1,), (1,))
    with pytest.raises(ValueError, match="strat cannot be combined"):
        vegas.vegas_integrate(*args, strat=vegas.Stratification((2, 2)), freq_observables=fo)
    with pytest.raises(ValueError, match="strat cannot be combined"):
        vegas.vegas_integrate(*args, strat=vegas.Stratification((2, 2)), matsubara=mz, freq_observables=fo)
    with pytest.raises(ValueError, match="strat cannot be combined"):
        vegas.vegas_integrate_binned(*args, object(), strat=vegas.Stratification((2, 2)), matsubara=mz, freq_observables=fo)
    with pytest.raises(Exception):
        fo.coef = ()                                                         # frozen


def test_complex_fields_are_assembled_from_the_components():
    """What the driver reports: combine_covariance on the 2 M real components of every iteration, then component m in the real part and
    component M + m in the imaginary part of entry m -- for the mean, the error bar and chi2/dof alike."""
    rng = np.random.default_rng(4)
    F, M, n_it = 3, 2, 4
    its = []
    for _ in range(n_it):
        a = rng.normal(size=(F, 2 * M, 2 * M))
        its.append((rng.normal(size=(F, 2 * M)), a @ a.transpose(0, 2, 1) + 0.1 * np.eye(2 * M)))
    mean, err, chi2, cov = vegas.combine_covariance(its)
    assert mean.shape == err.shape == chi2.shape == (F, 2 * M) and cov.shape == (F, 2 * M, 2 * M)
    cm, ce, cc = (vegas.complex_components(v) for v in (mean, err, chi2))
    assert cm.shape == (F, M) and np.iscomplexobj(cm)
    assert np.array_equal(cm.real, mean[:, :M]) and np.array_equal(cm.imag, mean[:, M:])
    assert np.array_equal(ce.real, err[:, :M]) and np.array_equal(ce.imag, err[:, M:])
    assert np.array_equal(cc.real, chi2[:, :M]) and np.array_equal(cc.imag, chi2[:, M:])
    # the real and the imaginary parts are combined each on its own, as matsubara= reports them: combine on the components alone agrees
    for p in range(2 * M):
        m1, e1, c1 = vegas.combine([(a[:, p], np.sqrt(c[:, p, p])) for a, c in its])
        part = (lambda v: v.real) if p < M else (lambda v: v.imag)
        assert np.array_equal(part(cm)[:, p % M], m1) and np.array_equal(part(ce)[:, p % M], e1) and np.array_equal(part(cc)[:, p % M], c1)
    assert np.allclose(np.einsum("fpp->fp", cov), err ** 2, rtol=1e-13)
    # a bin axis in front, and nan (chi2/dof of a constant) survives in either part
    x = np.arange(24.0).reshape(2, 3, 4)
    x[1, 2, 3] = np.nan
    y = vegas.complex_components(x)
    assert y.shape == (2, 3, 2) and y[0, 1, 1] == 5.0 + 7.0j and np.isnan(y[1, 2, 1].imag) and y[1, 2, 1].real == 21.0
