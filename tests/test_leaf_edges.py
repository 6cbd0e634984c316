"""The leaf formulas at their edges, against 60-digit values (tests/golden/leaf_edges.npz, make_leaf_edges.py).

Every other leaf test draws K ~ U(-2, 2), T ~ U(0, beta) and compares with the float64 oracle at 1e-13 (900 ulp).  Here the
arguments are the edges -- w == 0 exactly (green() tests w > 0, green_derive w >= 0), w a few ulp either side of the Fermi
surface, tau = 0, +-1e-300, +-beta, tau_in == tau_out, exponent arguments down to -5e7, q^2 = 0 and 1e6 -- the reference is
the definition in 60 digits, stored as pairs of doubles, and the bars are a few ulp:

  u = 2^-53, x = w a the exponent's argument, v the exact value, S = oracle.green_derive_scale
  order 0              (2|x| + 8) u |v| + 4 2^-1074     2|x| u: the roundings of a and of w a; 8: exp <= 2 u, 1 + e <= 2.5 u,
                                                        the quotient <= 1 u (Newton form), product and division 0.5 u each, margin
  interaction order n  (4 + 2.5 n) u |v|                ((5 + 3.5 n) u with FDG_MC_RCP_NEWTON)
  green_derive n >= 1  (2|x| + E_n) u S + 4 2^-1074     E_n: twice the oracle's own worst err / (u S) - 2|x| on this grid (below)

One term is wider than 4 2^-1074: where A = exp(x) itself is subnormal (x < -708.4), the floor of the derivative orders is
4 2^-1074 max(1, (|a| + beta)^n / n!).  A subnormal A carries an absolute error of up to one unit of 2^-1074 whatever computes it
(the exp bar below), and green_derive multiplies A by sum_k C(n,k) Q_k(g) a^(n-k) b^k / n!, at most (|a| + beta)^n / n! in
magnitude since |Q_k| <= 1 on [0, 1]: that error cannot stay below 4 units in float64.  Measured with the flat floor: the oracle
itself is 14 units off at kF = 1.5, beta = 8, k = 9.766, tau = 0, order 2 (value -9e-323), 197 entries of that parameter set
alike.  Where A is normal the floor is the flat one.

No route gets a wider bar than another.  The CPU part pins the oracle, the one-kernel route's program (replayed with numpy) and a
numpy restatement of that route's hand-written exp; the GPU part runs the table-driven and the specialised leaf kernel and the
fused, split and one-kernel routes (the latter also with FDG_MC_RCP_NEWTON) on the same grid, and ties the device's exp to the
restatement bit for bit."""
import functools
import glob
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi
from test_random_graphs import leaves_table, same

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -53
TINY = 2.0 ** -1074
SENTINEL = -7.0
FACT = [1.0, 1.0, 2.0, 6.0, 24.0, 120.0]

# green_derive: the oracle's own worst err / (u S) - 2|x| against the golden values over the grid (test_oracle_on_the_grid prints
# it), and the bar's E_n = twice that, rounded up.  (1e-12 / u = 9 000 is the project's bar elsewhere.)
ORACLE_WORST = {1: 1.11, 2: 1.49, 3: 8.17, 4: 67.2, 5: 306.3}
E_N = {1: 2.3, 2: 3.0, 3: 16.4, 4: 134.4, 5: 612.6}


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLD, "leaf_edges.npz")))


def leaf_tables(z, clip=False):
    """the fixture's tables; clip: interaction orders <= 3 (what the specialised leaf kernel and the fused kernel cover), as
    test_random_graphs.random_leaf_tables clips them"""
    ty, od = z["leaf_type"], z["leaf_order"]
    if clip:
        od = np.where(ty == 2, np.minimum(od, 3), od).astype(np.int32)
    return dict(leaf_type=ty, leaf_order=od, tau_in=z["tau_in"], tau_out=z["tau_out"], loop_index=z["loop_index"], basis=z["basis"])


def tab_args(tb):
    return (tb["leaf_type"], tb["leaf_order"], tb["tau_in"], tb["tau_out"], tb["loop_index"], tb["basis"], 3, 3)


def golden_values(z, p, tb):
    """(hi, lo) [B, L] of parameter set p for the tables tb (a clipped leaf takes the column of the leaf that has its order)"""
    col = {(int(t), int(n), int(a), int(b), int(m)): i for i, (t, n, a, b, m) in
           enumerate(zip(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"]))}
    src = [col[(int(t), int(n), int(a), int(b), int(m))] for t, n, a, b, m in
           zip(tb["leaf_type"], tb["leaf_order"], tb["tau_in"], tb["tau_out"], tb["loop_index"])]
    idx = z["val_idx"][p][:, src]
    hi = np.where(idx >= 0, z["val_hi"][idx], 1.0)
    lo = np.where(idx >= 0, z["val_lo"][idx], 0.0)
    return hi, lo


def leaf_arguments(z, p, tb, i):
    """(tau as the table gives it, tau with 0 -> -1e-10, w, a, x = w a) of fermionic leaf i, in float64 like every route"""
    beta = float(z["beta"][p])
    T = z["T"][p]
    w = z["w"][p][:, int(tb["loop_index"][i]) - 1]
    tau0 = T[:, int(tb["tau_out"][i]) - 1] - T[:, int(tb["tau_in"][i]) - 1]
    tau = np.where(tau0 == 0.0, -1e-10, tau0)
    pos = (w > 0.0) if int(tb["leaf_order"][i]) == 0 else (w >= 0.0)          # green() / green_derive
    a = np.where(pos, np.where(tau > 0.0, -tau, -(tau + beta)), np.where(tau > 0.0, beta - tau, -tau))
    return tau0, tau, w, a, w * a


def bars(z, p, tb, newton=False):
    """[B, L] absolute bars of parameter set p (0 for a leaf without a formula: its value is 1.0 exactly), and per leaf the pair
    (2|x|, unit) that turns an error into the `excess` figures of the module docstring"""
    hi, _ = golden_values(z, p, tb)
    bar = np.zeros_like(hi)
    unit = []
    for i in range(hi.shape[1]):
        ty, n = int(tb["leaf_type"][i]), int(tb["leaf_order"][i])
        if ty == 2:
            bar[:, i] = ((5 + 3.5 * n) if newton else (4 + 2.5 * n)) * U * np.abs(hi[:, i])
            unit.append((np.zeros(hi.shape[0]), U * np.abs(hi[:, i])))
        elif ty == 1:
            tau0, _, w, a, x = leaf_arguments(z, p, tb, i)
            floor = np.full(hi.shape[0], 4 * TINY)
            if n == 0:
                s, e = np.abs(hi[:, i]), 8.0
            else:
                beta = float(z["beta"][p])
                with np.errstate(under="ignore"):
                    s, e = oracle.green_derive_scale(tau0, w, beta, n), E_N[n]
                    floor *= np.where(np.exp(x) < 2.0 ** -1022, np.maximum(1.0, (np.abs(a) + beta) ** n / FACT[n]), 1.0)
            with np.errstate(under="ignore"):
                bar[:, i] = (2 * np.abs(x) + e) * U * s + floor
                unit.append((2 * np.abs(x), U * s))
        else:
            unit.append((np.zeros(hi.shape[0]), np.zeros(hi.shape[0])))
    return bar, unit


def check_values(z, p, tb, got, what, newton=False, stats=None):
    """got [B, L] against the golden values within the bars; `stats` collects, per (type, order), the worst err / unit - 2|x| over the
    entries whose unit is a normal number (what the derivations of the bars speak about)"""
    hi, lo = golden_values(z, p, tb)
    bar, unit = bars(z, p, tb, newton)
    assert got.shape == hi.shape
    with np.errstate(invalid="ignore", under="ignore"):
        err = np.abs((got - hi) - lo)
    formula = tb["leaf_type"] != 0
    assert (got[:, ~formula] == 1.0).all(), (what, "a leaf without a formula is not 1.0")
    if stats is not None:
        for i in np.nonzero(formula)[0]:
            two_x, s = unit[i]
            ok = s >= 2.0 ** -1022
            if ok.any():
                key = (int(tb["leaf_type"][i]), int(tb["leaf_order"][i]))
                with np.errstate(invalid="ignore"):
                    stats[key] = max(stats.get(key, -np.inf), float(np.max(err[ok, i] / s[ok] - two_x[ok])))
    bad = ~(err <= bar)                                   # (a NaN fails)
    if bad.any():
        b, i = np.argwhere(bad)[0]
        raise AssertionError((what, "parameter set", p, int(bad.sum()), "entries outside their bar; first: sample", int(b), "leaf", int(i),
                              "type/order", int(tb["leaf_type"][i]), int(tb["leaf_order"][i]), "got", float(got[b, i]), "want", float(hi[b, i]),
                              "err/bar", float(err[b, i] / bar[b, i]) if bar[b, i] else np.inf, "K", z["K"][p][b, :, 0].tolist(), "T", z["T"][p][b].tolist()))


def show(what, stats):
    print(what, "worst err/unit - 2|x| per (type, order):", {k: round(v, 2) for k, v in sorted(stats.items())})


# --------------------------------------------------------------------------- #
# the one-kernel route's exp (fdg_isa.cpp, case M_EXP), one rounded operation per line
# --------------------------------------------------------------------------- #
_fh = float.fromhex
K_LOG2E, K_LN2HI, K_LN2LO = _fh("0x1.71547652b82fep+0"), _fh("0x1.62e42fefa39efp-1"), _fh("0x1.abc9e3b39803fp-56")
K_EXPC = [_fh(s) for s in ("0x1.0000000000000p+0", "0x1.0000000000000p+0", "0x1.0000000000011p-1", "0x1.555555555555ap-3",
                           "0x1.555555554f0a5p-5", "0x1.111111110f218p-7", "0x1.6c16c18804745p-10", "0x1.a01a01b148c00p-13",
                           "0x1.a019919593233p-16", "0x1.71ddf5667e394p-19", "0x1.28b41ab9f014bp-22", "0x1.af63371ef88d9p-26")]


def isa_exp(x, with_r=False):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        tA = x * K_LOG2E                                                  # v_mul_f64
        tA = np.rint(tA)                                                  # v_rndne_f64
        tB = oracle.fma(tA, -K_LN2HI, x)                                  # v_fma_f64
        tB = oracle.fma(tA, -K_LN2LO, tB)                                 # v_fma_f64
        d = tB * K_EXPC[11]                                               # v_mul_f64
        d = d + K_EXPC[10]                                                # v_add_f64
        for k in range(9, -1, -1):
            d = oracle.fma(d, tB, K_EXPC[k])                              # v_fma_f64
        n = np.clip(tA, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int32)       # v_cvt_i32_f64 (saturates)
        d = np.ldexp(d, n)                                                # v_ldexp_f64
    return (d, tB) if with_r else d


def test_isa_exp_restated_against_golden():
    """The sequence and constants of M_EXP in numpy against the 60-digit exp: 5 000 random arguments in [-746, 0] and the steering
    arguments (both sides of every rounding tie of the range reduction below n = -1020 and of every 16th above, of the ends of the
    subnormal range, of -1e4, -1e6, -1e9).  Bars: 2 u relative where exp(x) is normal (the figure the order-0 bar assumes), 1 unit
    of 2^-1074 where it is subnormal, exactly 0 from -745.14 down to -4e15.
    Measured here: 1.89 u in the normal range (at a tie; 1.22 u over the random arguments alone), 0.50 units in the subnormal
    range, max |r| = 0.3465736."""
    z = golden()
    x, hi, lo, units = z["exp_x"], z["exp_hi"], z["exp_lo"], z["exp_units"]
    assert len(x) > 5500 and x.min() < -1e9 and (x > -1.0).any()
    got, r = isa_exp(x, with_r=True)
    normal = np.isnan(units)
    rel = np.abs((got[normal] - hi[normal]) - lo[normal]) / hi[normal] / U
    sub = ~normal
    un = np.abs(got[sub] * 2.0 ** 537 * 2.0 ** 537 - units[sub])
    in_range = x >= -746.0
    print("isa_exp: worst error", float(rel.max()), "u (normal range,", int(normal.sum()), "points),", float(un.max()),
          "units of 2^-1074 (subnormal range,", int(sub.sum()), "points); max |r| =", float(np.abs(r[in_range]).max()))
    assert rel.max() <= 2.0                                           # measured 1.89
    assert un.max() <= 1.0                                            # measured 0.50
    assert np.abs(r[in_range]).max() <= 0.34658                       # measured 0.3465736
    below = np.concatenate([x[x <= -745.14], [-745.14, -746.0, -1e3, -1e4, -1e6, -1e9, -1e12, -4e15]])
    assert (isa_exp(below) == 0.0).all() and not np.signbit(isa_exp(below)).any()
    # the ties are really met: arguments whose product with log2 e is exactly n + 1/2, and arguments on both sides of them
    frac = x * K_LOG2E - np.floor(x * K_LOG2E)
    assert (frac[x > -746.0] == 0.5).sum() >= 20 and (frac < 0.5).any() and (frac > 0.5).any()


def test_emitted_exp_is_the_restated_sequence(libfdg, fdgopt, no_shipped_cache, tmp_path):
    """What ties isa_exp to fdg_isa.cpp without a device: the one-kernel route's listing for the fixture's tables (assembled on the host),
    read back.  Every v_rndne_f64 sits in the instruction sequence restated above, and the constant operand of each instruction -- an
    SGPR pair filled by s_mov_b32 literals, or an inline 1.0 -- is the restated constant, bit for bit."""
    import re
    import struct
    z = golden()
    tb = leaf_tables(z)
    os.chmod(tmp_path, 0o700)
    fdgopt.set("FDG_MC_ROUTE", "isa")
    f = fd.compile_table(leaves_table(len(tb["leaf_type"])), specialize="isa", cache_dir=str(tmp_path))
    tab, _keep = capi.make_leaf_tables(*tab_args(tb))
    f.handle.specialize_fused(tab, str(tmp_path), capi.FDG_SPEC_KEEP_SOURCE)
    text = [open(os.path.join(tmp_path, n)).read() for n in os.listdir(tmp_path) if n.endswith(".s")]
    text = [t for t in text if "v_rndne_f64" in t]
    assert len(text) == 1
    sreg, valu = {}, []                                   # SGPR -> its last literal; (mnemonic, constant operand or None) of every VALU line
    for line in text[0].splitlines():
        line = line.strip()
        m = re.match(r"s_mov_b32 s(\d+), (0x[0-9a-f]+)$", line)
        if m:
            sreg[int(m.group(1))] = int(m.group(2), 16)
        if not line.startswith("v_"):
            continue
        const = []
        for lo, hi in re.findall(r"s\[(\d+):(\d+)\]", line):
            const.append(struct.unpack("<d", struct.pack("<II", sreg[int(lo)], sreg[int(hi)]))[0] if int(lo) in sreg and int(hi) in sreg else None)
        const += [float(c) for c in re.findall(r", (-?\d+\.\d+)(?=,|$)", line)]
        valu.append((line.split()[0], const))
    want = [("v_mul_f64", K_LOG2E), ("v_rndne_f64_e32", None), ("v_fma_f64", -K_LN2HI), ("v_fma_f64", -K_LN2LO), ("v_mul_f64", K_EXPC[11]),
            ("v_add_f64", K_EXPC[10])] + [("v_fma_f64", K_EXPC[k]) for k in range(9, -1, -1)] + [("v_cvt_i32_f64_e32", None), ("v_ldexp_f64", None)]
    at = [i for i, (op, _) in enumerate(valu) if op == "v_rndne_f64_e32"]
    assert len(at) >= 6                                  # one Fermi factor per momentum, one exponential per (momentum, time pair, select)
    for i in at:
        got = valu[i - 1:i - 1 + len(want)]
        assert [op for op, _ in got] == [op for op, _ in want], (i, got)
        for (op, const), (_, c) in zip(got, want):
            assert const == ([] if c is None else [c]), (i, op, [x.hex() if x is not None else x for x in const], c if c is None else c.hex())


# --------------------------------------------------------------------------- #
# CPU: the oracle and the one-kernel route's program
# --------------------------------------------------------------------------- #
def test_fixture_inputs_are_what_every_route_forms():
    """q^2, w and tau of the fixture are the oracle's own float64 values (so the golden values are evaluated at the arguments the
    kernels see); the count of samples is no multiple of the tile; the edges are on the grid."""
    z = golden()
    P, B = z["K"].shape[:2]
    assert P == 5 and (P * B) % 64 != 0 and B % 64 != 0 and 1500 <= P * B <= 3000 and len(z["steer_k"]) % 64 != 0
    for p in range(P):
        K = z["K"][p]
        q2 = (np.einsum("bjd,nj->bnd", K, z["basis"]) ** 2).sum(axis=2)
        assert np.array_equal(q2, z["q2"][p]) and np.array_equal(q2 - z["kF"][p] * z["kF"][p], z["w"][p])
        assert (z["w"][p] == 0.0).any() and (np.abs(z["w"][p][z["w"][p] != 0]).min() < 1e-14)
        assert (z["T"][p][:, 1] == z["beta"][p]).any() and (z["T"][p][:, 1] == -z["beta"][p]).any() and (z["T"][p][:, 1] == 0).any()
        assert (z["q2"][p] == 0.0).any() and (z["q2"][p] == 1e6).any()
    ty, tin, tout = z["leaf_type"], z["tau_in"], z["tau_out"]
    assert ((ty == 1) & (tin == tout)).sum() == 2 and (ty == 0).sum() == 1 and z["leaf_order"][ty == 2].max() == 7


def test_oracle_on_the_grid():
    """oracle.leaf_values against the golden values with the module's bars: the first high-precision pin of its order-0 propagator and
    its interaction leaf, and green_derive at w == 0, tau = 0, +-beta.  Prints the figures behind ORACLE_WORST / E_N."""
    z = golden()
    tb = leaf_tables(z)
    stats = {}
    for p in range(len(z["kF"])):
        with np.errstate(all="ignore"):
            got = oracle.leaf_values(*tab_args(tb)[:6], z["K"][p], z["T"][p], float(z["kF"][p]), float(z["beta"][p]), float(z["lam"][p]))
        got[:, tb["leaf_type"] == 0] = 1.0                    # (the oracle leaves them NaN: untouched)
        check_values(z, p, tb, got, "oracle", stats=stats)
    show("oracle", stats)
    for n in range(1, 6):
        assert stats[(1, n)] <= ORACLE_WORST[n] * 1.0001 + 1e-9 and E_N[n] >= 2 * ORACLE_WORST[n] and E_N[n] < 1e-12 / U, (n, stats[(1, n)])


class _EmulatedExp:
    """numpy for replay_mc, with the one-kernel route's own exp in the place of numpy's"""

    def __getattr__(self, name):
        return isa_exp if name == "exp" else getattr(np, name)


def program_leaves(z, p, options=(), exp="numpy"):
    """fdg_graph_mc_program of the leaves-as-roots graph over the fixture's tables, replayed on parameter set p's samples"""
    import test_next_rows
    tb = leaf_tables(z)
    L = len(tb["leaf_type"])
    tab, _keep = capi.make_leaf_tables(*tab_args(tb), float(z["kF"][p]), float(z["beta"][p]), float(z["lam"][p]))
    h = capi.GraphHandle(leaves_table(L))
    for k, v in options:
        h.set_option(k, v)
    ops, nr, nl, nm = h.mc_program(tab, n_reg=40, n_lds=8)
    B = z["K"].shape[1]
    X = np.concatenate([z["K"][p].reshape(B, -1), z["T"][p]], axis=1)
    saved = test_next_rows.np
    try:
        if exp == "isa":
            test_next_rows.np = _EmulatedExp()
        with np.errstate(all="ignore"):
            return test_next_rows.replay_mc(ops, nr, nl, nm, 0, X, L), ops
    finally:
        test_next_rows.np = saved


@pytest.mark.parametrize("exp", ["numpy", "isa"])
@pytest.mark.parametrize("newton", [False, True])
def test_mc_program_on_the_grid(libfdg, exp, newton):
    """The one-kernel route's program replayed without a device (test_next_rows.replay_mc: numpy's exp, or the restated exp of this
    route) against the golden values: the selects, M_FIXZ and M_SELC at w == 0, tau == 0 and tau = +-beta, the order of the operations
    of every formula.  FDG_MC_RCP_NEWTON really swaps the division for the reciprocal op (both replay as 1 / x here; the device's
    Newton form runs in the GPU part)."""
    z = golden()
    tb = leaf_tables(z)
    stats = {}
    for p in range(len(z["kF"])):
        got, ops = program_leaves(z, p, (("FDG_MC_RCP_NEWTON", "1"),) if newton else (), exp)
        assert bool((ops["kind"] == 18).any()) == newton and bool((ops["kind"] == 23).any()) != newton
        check_values(z, p, tb, got, ("program", exp, newton), newton=newton, stats=stats)
    show(("program", exp, newton), stats)


def test_mc_program_selects_at_the_fermi_surface(libfdg):
    """green() tests w > 0 and green_derive w >= 0: at w == 0 exactly the two take different branches (a = beta - tau or -tau against
    -tau or -(tau + beta)).  The value hides it there (exp(0 a) = 1), so the program's own `a` and w a (FDG_MC_DEBUG_STAGE) are
    compared with the definition's, bit for bit, on the whole grid; the samples with w == 0 are on it."""
    z = golden()
    tb = leaf_tables(z)
    fermionic = np.nonzero(tb["leaf_type"] == 1)[0]
    n_zero = 0
    for p in range(len(z["kF"])):
        a_got, _ = program_leaves(z, p, (("FDG_MC_DEBUG_STAGE", "a"),))
        x_got, _ = program_leaves(z, p, (("FDG_MC_DEBUG_STAGE", "wa"),))
        for i in fermionic:
            _, _, w, a, x = leaf_arguments(z, p, tb, i)
            assert np.array_equal(a_got[:, i], a), (p, int(i), np.argwhere(a_got[:, i] != a)[:4].ravel())
            assert np.array_equal(x_got[:, i], x), (p, int(i))
            n_zero += int((w == 0.0).sum())
    assert n_zero >= 100


# --------------------------------------------------------------------------- #
# GPU: every route on the grid
# --------------------------------------------------------------------------- #
def device_inputs(cuda, K, T):
    import torch
    B = K.shape[0]
    return (torch.from_numpy(np.ascontiguousarray(K.reshape(B, -1).T)).to(cuda), torch.from_numpy(np.ascontiguousarray(T.T)).to(cuda))


def leaf_kernel_values(cuda, z, p, tb):
    """fdg_leaf_eval_device on parameter set p: [B, L], the column of the leaf without a formula (left alone by the kernel) set to 1.0"""
    import torch
    K, T = z["K"][p], z["T"][p]
    B, L = K.shape[0], len(tb["leaf_type"])
    dK, dT = device_inputs(cuda, K, T)
    buf = torch.full((L, B), SENTINEL, dtype=torch.float64, device=cuda)
    capi.leaf_eval_device(*tab_args(tb), float(z["kF"][p]), float(z["beta"][p]), float(z["lam"][p]), dK.data_ptr(), 1, B, dT.data_ptr(), 1, B,
                          buf.data_ptr(), 1, B, B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy().T.copy()
    own = tb["leaf_type"] != 0
    assert (got[:, ~own] == SENTINEL).all()
    got[:, ~own] = 1.0
    return got


def mc_values(cuda, handle, K, T, kF, beta, lam, L):
    """fdg_mc_eval_device of a leaves-as-roots handle: [B, L]"""
    import torch
    B = K.shape[0]
    dK, dT = device_inputs(cuda, K, T)
    root = torch.full((B, L), SENTINEL, dtype=torch.float64, device=cuda)
    handle.mc_eval_device(dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, kF, beta, lam, root.data_ptr(), L, 1, B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return root.cpu().numpy()


def mc_handle(tb, spec, cache_dir=None, flags=0):
    f = fd.compile_table(leaves_table(len(tb["leaf_type"])), specialize=spec)
    tab, _keep = capi.make_leaf_tables(*tab_args(tb))
    f.handle.specialize_fused(tab, cache_dir, flags)
    return f


def grid_through(cuda, z, tb, run, what, newton=False):
    """run(p) -> [B, L] for every parameter set, checked against the golden values; returns the values"""
    stats, out = {}, []
    for p in range(len(z["kF"])):
        got = run(p)
        check_values(z, p, tb, got, what, newton=newton, stats=stats)
        out.append(got)
    show(what, stats)
    return out


@pytest.mark.gpu
def test_table_driven_leaf_kernel_on_the_grid(libfdg, cuda, fdgopt):
    z = golden()
    tb = leaf_tables(z)
    fdgopt.set("FDG_LEAF_GENERIC", "1")
    grid_through(cuda, z, tb, lambda p: leaf_kernel_values(cuda, z, p, tb), "fdg_leaf_kernel")


@pytest.mark.gpu
def test_specialised_leaf_kernel_on_the_grid(libfdg, cuda, fdgopt, no_shipped_cache, tmp_path):
    """fdg_leaf_spec (interaction orders clipped to 3): the bars, the bits of the table-driven kernel, and it really ran (a failed
    compilation falls back to the table-driven kernel)."""
    z = golden()
    tb = leaf_tables(z, clip=True)
    os.chmod(tmp_path, 0o700)
    fdgopt.set("FDG_CACHE_DIR", str(tmp_path))
    fdgopt.unset("FDG_LEAF_GENERIC")
    spec = grid_through(cuda, z, tb, lambda p: leaf_kernel_values(cuda, z, p, tb), "fdg_leaf_spec")
    assert glob.glob(str(tmp_path / "fdg_leaf_*.hsaco"))
    fdgopt.set("FDG_LEAF_GENERIC", "1")
    for p, got in enumerate(spec):
        assert same(got, leaf_kernel_values(cuda, z, p, tb)), (p, "specialised kernel differs from the table-driven one")


@pytest.mark.gpu
def test_fused_route_on_the_grid(libfdg, cuda, fdgopt):
    z = golden()
    tb = leaf_tables(z, clip=True)
    fdgopt.set("FDG_MC_ROUTE", "fused")
    f = mc_handle(tb, True)
    L = len(tb["leaf_type"])
    grid_through(cuda, z, tb, lambda p: mc_values(cuda, f.handle, z["K"][p], z["T"][p], float(z["kF"][p]), float(z["beta"][p]), float(z["lam"][p]), L),
                 "FDG_MC_ROUTE=fused")


@pytest.mark.gpu
def test_split_route_on_the_grid(libfdg, cuda, fdgopt):
    """FDG_MC_ROUTE=split: the bars, and the bits of the table-driven leaf kernel."""
    z = golden()
    tb = leaf_tables(z)
    fdgopt.set("FDG_MC_ROUTE", "split")
    f = mc_handle(tb, True)
    L = len(tb["leaf_type"])
    got = grid_through(cuda, z, tb, lambda p: mc_values(cuda, f.handle, z["K"][p], z["T"][p], float(z["kF"][p]), float(z["beta"][p]), float(z["lam"][p]), L),
                       "FDG_MC_ROUTE=split")
    fdgopt.set("FDG_LEAF_GENERIC", "1")
    for p, g in enumerate(got):
        assert same(g, leaf_kernel_values(cuda, z, p, tb)), (p, "split route differs from the table-driven leaf kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("newton", [False, True])
def test_one_kernel_route_on_the_grid(libfdg, cuda, fdgopt, no_shipped_cache, tmp_path, newton):
    """FDG_MC_ROUTE=isa, with the correctly rounded division and with FDG_MC_RCP_NEWTON (v_rcp_f64 + two Newton steps; the listing shows
    that the option took).  With the division every operation of the kernel is an IEEE operation or the restated exp: the values are,
    bit for bit, the program replayed on the CPU with isa_exp (test_mc_program_on_the_grid's own subject)."""
    z = golden()
    tb = leaf_tables(z)
    os.chmod(tmp_path, 0o700)
    fdgopt.set("FDG_MC_ROUTE", "isa")
    if newton:
        fdgopt.set("FDG_MC_RCP_NEWTON", "1")
    f = mc_handle(tb, "isa", str(tmp_path), capi.FDG_SPEC_KEEP_SOURCE)
    text = "".join(open(os.path.join(tmp_path, n)).read() for n in os.listdir(tmp_path) if n.endswith(".s"))
    assert ("v_rcp_f64_e64" in text) == newton and ("v_div_fixup_f64" in text) != newton
    L = len(tb["leaf_type"])
    got = grid_through(cuda, z, tb, lambda p: mc_values(cuda, f.handle, z["K"][p], z["T"][p], float(z["kF"][p]), float(z["beta"][p]), float(z["lam"][p]), L),
                       ("FDG_MC_ROUTE=isa", newton), newton=newton)
    if not newton:
        for p, g in enumerate(got):
            want = program_leaves(z, p, (), "isa")[0]
            assert same(g, want), (p, "device differs from the replayed program", np.argwhere(g != want)[:4].tolist())


@pytest.mark.gpu
def test_one_kernel_route_exp_is_the_restated_sequence(libfdg, cuda, fdgopt):
    """The exponential alone: the one-kernel route run with FDG_MC_DEBUG_STAGE=wa (the exponent's argument of every fermionic leaf) and
    =A (its exp), over the whole grid and the steering block (arguments at the rounding ties, in the subnormal range and down to -1e9).
    A is isa_exp(wa) bit for bit -- so what test_isa_exp_restated_against_golden shows of the restatement holds for the device's
    v_rndne / v_fma / v_cvt / v_ldexp sequence -- and wa is the definition's w a.  Stage `a` on the grid: the device's selects take the
    definition's branch at w == 0, where green() and green_derive differ and the value cannot show it."""
    z = golden()
    tb = leaf_tables(z)
    L = len(tb["leaf_type"])
    fermionic = np.nonzero(tb["leaf_type"] == 1)[0]
    kF, beta, lam, tau = (float(v) for v in z["steer_param"])
    Bs = len(z["steer_k"])
    Ks = np.zeros((Bs, 2, 3)); Ks[:, 0, 0] = z["steer_k"]
    Tsr = np.zeros((Bs, 3)); Tsr[:, 1] = tau
    blocks = [(z["K"][p], z["T"][p], float(z["kF"][p]), float(z["beta"][p]), float(z["lam"][p])) for p in range(len(z["kF"]))]
    blocks.append((Ks, Tsr, kF, beta, lam))
    fdgopt.set("FDG_MC_ROUTE", "isa")
    stage = {}
    for s in ("wa", "A", "a"):
        fdgopt.set("FDG_MC_DEBUG_STAGE", s)
        f = mc_handle(tb, "isa")
        stage[s] = [mc_values(cuda, f.handle, *blk, L)[:, fermionic] for blk in (blocks if s != "a" else blocks[:-1])]
    for k, (wa, A) in enumerate(zip(stage["wa"], stage["A"])):
        want = isa_exp(wa)
        assert same(A, want), (k, "device exp differs from the restated sequence", np.argwhere(A != want)[:4].tolist())
    for p in range(len(z["kF"])):
        for c, i in enumerate(fermionic):
            _, _, _, a, x = leaf_arguments(z, p, tb, i)
            assert np.array_equal(stage["wa"][p][:, c], x), (p, int(i))
            assert np.array_equal(stage["a"][p][:, c], a), (p, int(i))
    first = list(fermionic).index(0)                    # leaf 0: momentum 1, order 0, (tau_in, tau_out) = (1, 2)
    assert np.array_equal(stage["wa"][-1][:, first], z["steer_x"])
