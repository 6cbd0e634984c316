"""The Matsubara projection without a device (include/fdg.h: fdg_matsubara_phase, fdg_accumulate_device_matsubara,
fdg_mc_accumulate_device_matsubara; csrc/fdg_matsubara.h; workloads.root_times, vegas.MatsubaraProjection): the three symbols are declared,
exported and bound; fdg_matsubara_phase carries the bits of a numpy restatement of the header's operation order and stays within
(4 pi |2n+1| + 16) 2^-53 of a long-double exponential; every argument check of the accumulate calls runs before any device work.  The
mirrors written here are what tests/test_matsubara_accumulate.py restates.  The helpers are copies of tests/test_julia_shim.py's and
tests/test_vegas_polar_host.py's."""
import ctypes
import os
import re

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, frontends, vegas, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fdg.h")
JL = os.path.join(ROOT, "feynmandiagram.jl_amd", "julia", "hip_compiler.jl")
NAMES = ("fdg_matsubara_phase", "fdg_accumulate_device_matsubara", "fdg_mc_accumulate_device_matsubara")
FAKE = [0x10000 * (i + 1) for i in range(12)]     # pointers the checks only compare with NULL or with each other; never read through
UNIT = 2.0 ** -53


# ---- the static readers of the header and of the Julia shim (copies) ---------------------------------------------------------------- #
def c_prototypes():
    text = open(HDR).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    protos = {}
    for m in re.finditer(r"\b(int|void|const\s+char\s*\*)\s*(fdg_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        params = [p.strip() for p in m.group(3).replace("\n", " ").split(",")]
        protos[m.group(2)] = (m.group(1).strip(), [] if params in (["void"], [""]) else params)
    return protos


def c_class(param):
    p = re.sub(r"\s+", " ", param)
    if "*" in p:
        return "cstring" if re.match(r"const char \*\s*\w*$", p) else "pointer"
    base = re.sub(r"\b(const|volatile)\b", "", p).split()
    ty = " ".join(base[:-1]) if len(base) > 1 else base[0]
    return {"int64_t": "i64", "uint64_t": "u64", "uint32_t": "u32", "unsigned": "u32", "unsigned int": "u32", "int": "i32", "double": "f64",
            "size_t": "u64", "int32_t": "i32"}.get(ty, "?" + ty)


JL_CLASS = {"Int64": "i64", "UInt64": "u64", "Csize_t": "u64", "UInt32": "u32", "Cuint": "u32", "Cint": "i32", "Int32": "i32", "Cdouble": "f64",
            "Float64": "f64", "Cstring": "cstring"}


def jl_class(ty):
    ty = ty.strip()
    return "pointer" if ty.startswith(("Ptr{", "Ref{")) else JL_CLASS.get(ty, "?" + ty)


def split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += (ch in "([{") - (ch in ")]}")
        if ch == "," and depth == 0:
            out.append(cur.strip()); cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def jl_ccalls():
    text = re.sub(r"#[^\n]*", "", open(JL).read())
    calls = {}
    for m in re.finditer(r"ccall\(", text):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        parts = split_top(text[m.end():i - 1])
        sym = re.match(r"\(\s*:(\w+)\s*,\s*_libfdg\s*\)", parts[0]).group(1)
        calls[sym] = ([t for t in split_top(parts[2].strip()[1:-1]) if t], parts[3:])
    return calls


# ---- numpy mirrors ------------------------------------------------------------------------------------------------------------------ #
TWO_OVER_PI, P1, P1T = np.float64(0.6366197723675814), np.float64(1.5707963267341256), np.float64(6.077100506506192e-11)
S = [np.float64(v) for v in (-0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06,
                             -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15)]
CC = [np.float64(v) for v in (0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
                              2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14)]


def mirror_sincos(x):
    """(s, c) of csrc/fdg_sincos.h for doubles in [0, 2 pi]: the header's operations, one numpy operation each, in its order"""
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


def mirror_phase(tau, beta, n, fermionic):
    """(s, c, th) of csrc/fdg_matsubara.h: one numpy operation per line of the header's recipe"""
    tau, beta = np.asarray(tau, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    mult = (2 * np.asarray(n, dtype=np.int64) + (1 if fermionic else 0)).astype(np.float64)
    x = tau / beta
    m = x * mult
    h = m * 0.5
    fl = np.floor(h)
    r = h - fl
    th = r * np.float64(6.283185307179586)
    s, c = mirror_sincos(th)
    return s, c, th


def phase_points():
    """1e4 random (tau in (-beta, beta), beta, |n| <= 1000) and the edges tau = 0, +-beta (1 - 2^-53), n = 0, n = -1 at several beta"""
    rng = np.random.default_rng(20_250_101)
    beta = rng.uniform(0.1, 40.0, 10_000)
    tau = rng.uniform(-1.0, 1.0, 10_000) * beta
    tau = np.clip(tau, -beta * (1 - UNIT), beta * (1 - UNIT))
    n = rng.integers(-1000, 1001, 10_000)
    eb = np.array([0.1, 1.0, 3.0, 25.0, 40.0])
    et = np.concatenate([np.zeros(5), eb * (1 - UNIT), -eb * (1 - UNIT), -np.zeros(5), eb * 2.0 ** -60, -eb * 2.0 ** -60])
    ebb = np.tile(eb, 6)
    for en in (0, -1, 1, 1000, -1000):
        tau, beta, n = np.concatenate([tau, et]), np.concatenate([beta, ebb]), np.concatenate([n, np.full(et.shape, en)])
    assert (np.abs(tau) < beta).all()
    return tau, beta, n.astype(np.int64)


def lib_phase(tau, beta, n, fermionic):
    got = np.array([capi.matsubara_phase(float(t), float(b), int(k), fermionic) for t, b, k in zip(tau, beta, n)])
    return got[:, 0], got[:, 1]


# ---- declared, exported, bound ------------------------------------------------------------------------------------------------------ #
def test_symbols_are_declared_exported_and_bound(libfdg):
    protos, calls = c_prototypes(), jl_ccalls()
    text = open(JL).read()
    export = [x.strip() for x in re.search(r"^export\s+([^\n]*)", text, flags=re.M).group(1).split(",")]
    for name in NAMES:
        assert name in protos, name
        assert name in capi.EXPORTS, name
        assert hasattr(libfdg, name), name
        assert name in calls, name + ": not bound in the Julia shim"
        types, args = calls[name]
        params = protos[name][1]
        assert len(types) == len(params) == len(args) == len(getattr(libfdg, name).argtypes), name
        for jt, cp in zip(types, params):
            assert jl_class(jt) == c_class(cp), (name, jt, cp)
    for fn in ("fdg_matsubara_phase", "accumulate_device_matsubara!", "mc_accumulate_device_matsubara!"):
        assert fn in export, fn
    hdr = open(HDR).read()
    assert re.search(r"#define\s+FDG_MATSUBARA_FREQ_MAX\s+(\d+)", hdr).group(1) == str(capi.FDG_MATSUBARA_FREQ_MAX) == "64"
    assert re.search(r"#define\s+FDG_VERSION\s+102\b", hdr) and libfdg.fdg_version() == 102
    assert "test/ver4.jl:193" in hdr
    # the struct: the header's fields in the header's order, in the ctypes mirror and in the shim
    body = re.search(r"typedef struct fdg_matsubara \{(.*?)\} fdg_matsubara;", hdr, flags=re.S).group(1)
    fields = re.findall(r"[\s\*](\w+)\s*(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    want = [k for k, _ in capi.Matsubara._fields_]
    assert fields == want, (fields, want)
    jl = re.search(r"struct _FdgMatsubara\n(.*?)\nend", text, flags=re.S).group(1)
    assert [ln.strip().split("::")[0] for ln in jl.splitlines()] == want
    assert ctypes.sizeof(capi.Matsubara) == 104
    assert fd.MatsubaraProjection is vegas.MatsubaraProjection
    assert callable(capi.matsubara_phase) and callable(capi.GraphHandle.accumulate_device_matsubara)
    assert callable(capi.GraphHandle.mc_accumulate_device_matsubara) and callable(fd.GraphFunc.accumulate_matsubara)


# ---- fdg_matsubara_phase ------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("fermionic", [True, False])
def test_phase_matches_the_numpy_restatement_bit_for_bit(libfdg, fermionic):
    tau, beta, n = phase_points()
    gs, gc = lib_phase(tau, beta, n, fermionic)
    ws, wc, th = mirror_phase(tau, beta, n, fermionic)
    assert th.min() >= 0.0 and th.max() <= 6.283185307179586                  # inside fdg_sincos' domain
    assert (th == 6.283185307179586).any() and (th == 0.0).any()              # ... whose two ends the edge cases reach
    bad = (gs.view(np.uint64) != ws.view(np.uint64)) | (gc.view(np.uint64) != wc.view(np.uint64))
    assert not bad.any(), (tau[bad][:4], beta[bad][:4], n[bad][:4])


@pytest.mark.parametrize("fermionic", [True, False])
def test_phase_accuracy(libfdg, fermionic):
    """|s - sin|, |c - cos| <= (4 pi |2n+1| + 16) 2^-53 against exp(i omega_n tau) in long double: x = tau / beta and m = x * mult are
    each off by a relative 2^-53, i.e. the angle pi m by at most 2 pi |mult| 2^-53 in all (|x| <= 1; h, fl and r are exact); th = r * 2 pi
    adds one rounding and the constant's own error (4 more units at th <= 2 pi), and fdg_sincos its stated 4 units: 16 covers the rest.
    |2n+1| is used for both statistics (|2n| is smaller).  The reference's own error, an angle of up to 2001 pi held in 64 bits, is
    about 3 units: nothing next to a bound of hundreds at the |n| where it matters."""
    assert np.finfo(np.longdouble).nmant >= 63, "the reference needs at least 63 mantissa bits"
    tau, beta, n = phase_points()
    gs, gc = lib_phase(tau, beta, n, fermionic)
    pi = 4 * np.arctan(np.longdouble(1))
    omega = (2 * n + (1 if fermionic else 0)).astype(np.longdouble) * pi / beta.astype(np.longdouble)
    ref = np.exp(1j * (omega * tau.astype(np.longdouble)))                    # complex long double
    es = np.abs(gs.astype(np.longdouble) - ref.imag).astype(np.float64)
    ec = np.abs(gc.astype(np.longdouble) - ref.real).astype(np.float64)
    bound = (4 * np.pi * np.abs(2 * n + 1) + 16) * UNIT
    print("fdg_matsubara_phase: max error / bound =", (es / bound).max(), (ec / bound).max())
    assert (es <= bound).all() and (ec <= bound).all()


def test_bosonic_zero_frequency_is_exactly_one(libfdg):
    for tau, beta in ((0.0, 1.0), (-0.0, 1.0), (0.3, 1.0), (-0.3, 1.0), (24.9, 25.0), (-24.9, 25.0), (1e-300, 1.0)):
        s, c = capi.matsubara_phase(tau, beta, 0, False)
        assert (s, c) == (0.0, 1.0) and not np.signbit(s), (tau, beta, s, c)
    # the sign convention: e^{+i omega_n tau}; a fermionic phase at tau = beta is -1 up to the rounding of the angle
    s, c = capi.matsubara_phase(0.25, 1.0, 0, True)                           # omega_0 tau = pi / 4
    assert abs(s - np.sqrt(0.5)) < 4 * UNIT and abs(c - np.sqrt(0.5)) < 4 * UNIT
    s, c = capi.matsubara_phase(0.25, 1.0, -1, True)                          # omega_{-1} = -omega_0
    assert abs(s + np.sqrt(0.5)) < 4 * UNIT and abs(c - np.sqrt(0.5)) < 4 * UNIT


# ---- argument errors, no device present --------------------------------------------------------------------------------------------- #
def _desc(R, n_freq=3, freq=True, tin=True, tout=True, beta=2.0, n_tau=4, d_T=FAKE[4], outs=(FAKE[5], FAKE[6], FAKE[7], FAKE[8]), labels=None):
    f = np.arange(n_freq, dtype=np.int32) if n_freq else np.zeros(1, np.int32)
    ti = np.ones(R, np.int32) if labels is None else np.asarray(labels[0], np.int32)
    to = np.full(R, n_tau, np.int32) if labels is None else np.asarray(labels[1], np.int32)
    m = capi.Matsubara(n_freq, 1, f.ctypes.data if freq else None, ti.ctypes.data if tin else None, to.ctypes.data if tout else None, beta,
                       d_T, 1, 100, n_tau, *outs)
    return m, (f, ti, to)


def _leaf(h, m, n_bin=4, B=100, d_leaf=FAKE[0], d_bin=FAKE[1], d_acc=None, d_acc2=None, n_dim=0, n_grid=0, d_hist=None, d_hist_bin=None, lts=0):
    return capi.lib().fdg_accumulate_device_matsubara(h._h if h else None, d_leaf, 1, 8, lts, d_bin, 0, n_bin, None, None, 1, 0, n_dim, n_grid,
                                                      d_acc, d_acc2, d_hist, d_hist_bin, None if m is None else ctypes.addressof(m), B, None)


def _mc(h, m, n_bin=4, B=100, d_K=FAKE[0], d_T=FAKE[9], d_bin=FAKE[1], d_acc=None, d_acc2=None, n_dim=0, n_grid=0, d_hist=None,
        d_hist_bin=None):
    return capi.lib().fdg_mc_accumulate_device_matsubara(h._h if h else None, d_K, 1, 8, d_T, 1, 8, 1.0, 2.0, 0.5, d_bin, 0, n_bin, None, None,
                                                         1, 0, n_dim, n_grid, d_acc, d_acc2, d_hist, d_hist_bin,
                                                         None if m is None else ctypes.addressof(m), B, None)


def _err():
    return capi.lib().fdg_last_error().decode()


def test_argument_checks_need_no_device(libfdg):
    t = workloads.get("sigma2")
    h, R = capi.GraphHandle(t), t.n_root
    INV, UNS, OK = capi.FDG_E_INVALID, capi.FDG_E_UNSUPPORTED, capi.FDG_OK
    FM, BM = capi.FDG_MATSUBARA_FREQ_MAX, capi.FDG_BIN_MAX
    for call in (_leaf, _mc):
        good, _k = _desc(R)
        # (B = 0: valid arguments and nothing to do -- every check has passed, no device work, no error)
        assert call(h, good, B=0) == OK
        assert call(h, good, n_bin=1, d_bin=None, B=0) == OK
        assert call(h, good, d_acc=FAKE[2], d_acc2=FAKE[3], B=0) == OK
        assert call(h, good, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[11], B=0) == OK
        assert call(h, good, n_bin=1, d_bin=None, n_dim=3, n_grid=8, d_hist=FAKE[10], B=0) == OK
        assert call(h, _desc(R, n_freq=FM)[0], n_bin=BM // FM, B=0) == OK
        assert call(None, good) == INV and "handle" in _err()
        assert call(h, None) == INV and "descriptor" in _err()
        assert call(h, good, B=-1) == INV
        for i in range(4):                                                    # a NULL output; two outputs in one buffer
            outs = [FAKE[5], FAKE[6], FAKE[7], FAKE[8]]
            outs[i] = None
            assert call(h, _desc(R, outs=outs)[0]) == INV and "null device buffer" in _err()
            outs[i] = FAKE[5 + (i + 1) % 4]
            assert call(h, _desc(R, outs=outs)[0]) == INV and "same buffer" in _err()
        assert call(h, good, d_acc=FAKE[5], d_acc2=FAKE[3]) == INV and "same buffer" in _err()
        assert call(h, good, d_acc=FAKE[2], d_acc2=FAKE[2]) == INV and "same buffer" in _err()
        assert call(h, good, n_dim=3, n_grid=8, d_hist=FAKE[8]) == INV and "same buffer" in _err()
        assert call(h, good, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[10]) == INV and "same buffer" in _err()
        assert call(h, good, d_acc=FAKE[2]) == INV and "go together" in _err()
        assert call(h, good, d_acc2=FAKE[2]) == INV and "go together" in _err()
        for kw in ({"freq": False}, {"tin": False}, {"tout": False}):
            assert call(h, _desc(R, **kw)[0]) == INV and "host array" in _err()
        assert call(h, _desc(R, n_freq=0)[0]) == INV and "n_freq == 0" in _err()
        assert call(h, _desc(R, n_freq=FM + 1)[0], n_bin=1) == UNS and "FDG_MATSUBARA_FREQ_MAX" in _err()
        assert call(h, _desc(R, n_freq=FM)[0], n_bin=BM // FM + 1) == UNS and "n_bin * n_freq" in _err()
        assert call(h, good, n_bin=0) == INV and "n_bin == 0" in _err()
        assert call(h, good, n_bin=4, d_bin=None) == INV and "n_bin == 1" in _err()
        assert call(h, good, n_bin=BM + 1) == UNS
        for beta in (0.0, -1.0, float("nan")):
            assert call(h, _desc(R, beta=beta)[0]) == INV and "beta" in _err()
        for labels in (([0] * R, [1] * R), ([1] * R, [5] * R), ([1] * R, [1] * (R - 1) + [-2])):
            assert call(h, _desc(R, labels=labels)[0]) == INV and "time label" in _err()
        # the training block: a histogram without a map, a map without a histogram, limits, hist_bin without bins
        assert call(h, good, d_hist=FAKE[10]) == INV
        assert call(h, good, n_dim=3, n_grid=8) == INV and "null device buffer" in _err()
        assert call(h, good, n_dim=capi.FDG_VEGAS_DIM_MAX + 1, n_grid=8, d_hist=FAKE[10]) == UNS
        assert call(h, good, n_dim=3, n_grid=capi.FDG_VEGAS_GRID_MAX + 1, d_hist=FAKE[10]) == UNS
        assert call(h, good, n_bin=1, d_bin=None, n_dim=3, n_grid=8, d_hist=FAKE[10], d_hist_bin=FAKE[11]) == INV and "d_hist_bin" in _err()
    good, _k = _desc(R)
    assert _leaf(h, good, d_leaf=None) == INV
    assert _leaf(h, _desc(R, d_T=None)[0]) == INV and "null device buffer" in _err()
    assert _leaf(h, good, lts=8 * 64) == UNS and "tile-major" in _err()      # a tile-major batch on a handle without FDG_SPEC_ISA
    assert _mc(h, good, d_K=None) == INV
    assert _mc(h, _desc(R, d_T=None)[0], d_T=None) == INV and "null device buffer" in _err()
    # the descriptor's T may be NULL in the Monte-Carlo form; a handle that never met fdg_graph_specialize_fused is refused after the checks
    assert _mc(h, _desc(R, d_T=None)[0]) == INV and "fdg_graph_specialize_fused" in _err()
    assert _mc(h, good) == INV and "fdg_graph_specialize_fused" in _err()


def test_python_methods_forward_the_error_code(libfdg):
    t = workloads.get("sigma2")
    h, R = capi.GraphHandle(t), t.n_root
    for kw, n_bin, code in (({"n_freq": 0}, 4, capi.FDG_E_INVALID), ({"n_freq": 65}, 1, capi.FDG_E_UNSUPPORTED), ({"beta": 0.0}, 4, capi.FDG_E_INVALID)):
        m, _k = _desc(R, **kw)
        with pytest.raises(capi.FdgError) as e:
            h.accumulate_device_matsubara(FAKE[0], 1, 8, 0, FAKE[1], 0, n_bin, 0, m, B=100)
        assert e.value.code == code, kw
        with pytest.raises(capi.FdgError) as e:
            h.mc_accumulate_device_matsubara(FAKE[0], 1, 8, FAKE[9], 1, 8, 1.0, 2.0, 0.5, FAKE[1], 0, n_bin, 0, m, B=100)
        assert e.value.code == code, kw
    m, keep = capi.make_matsubara([0, 1, -3], True, [1] * R, [2] * R, 2.0, 4, *FAKE[5:9], FAKE[4], 1, 100)
    assert (m.n_freq, m.fermionic, m.n_tau, m.beta, m.t_comp_stride) == (3, 1, 4, 2.0, 100)
    assert keep[0].tolist() == [0, 1, -3]


# ---- the tables come from the graphs ------------------------------------------------------------------------------------------------- #
def test_root_times_come_from_the_rows():
    for name in ("parquet_sigma2", "parquet_sigma4", "sigma2"):
        tin, tout = workloads.root_times(name)
        t = workloads.get(name)
        _, rows = workloads.parquet_graphs("parquet_sigma2" if name == "sigma2" else name)
        assert tin.dtype == tout.dtype == np.int32 and tin.shape == tout.shape == (t.n_root,)
        assert [(int(a), int(b)) for a, b in zip(tin, tout)] == [tuple(r["extT"]) for r in rows]
    tin, tout = workloads.root_times("parquet_sigma4")
    assert tin.tolist() == [1, 1, 1, 1] and tout.tolist() == [1, 2, 3, 4]     # the instantaneous row: tin == tout
    tin3, tout3 = workloads.root_times("parquet_sigma4_taylor2")
    assert tin3.tolist() == [1] * 12 and tout3.tolist() == [1, 2, 3, 4] * 3
    graphs, rows = workloads.parquet_graphs("parquet_ver4_4")
    a, b = frontends.root_times(graphs[:5], pair=(0, 3))
    assert list(zip(a, b)) == [(r["extT"][0], r["extT"][3]) for r in rows[:5]]
    with pytest.raises(ValueError):
        frontends.root_times(workloads.parquet_graphs("parquet_sigma2")[0], pair=(0, 2))
