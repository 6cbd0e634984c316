"""Golden vectors for the leaf formulas at their edges (tests/test_leaf_edges.py): the fermionic propagator of
example/benchmark.jl:113-127, its green_derive orders 1..5 (benchmark.jl:93-111) and the interaction leaf
8 pi / invK (lambda invK)^n, from mpmath at 60 digits -- the DEFINITIONS evaluated at the float64 q^2, w and tau that every
device route forms, taken as exact.  Derivatives are mpmath's numerical derivatives of the closed form (as in
make_green_derive.py) and are cross-checked here against the Leibniz sum.  Run here (needs mpmath); only the .npz travels.

Inputs.  n_loop = 2, dim = 3, every momentum along the first axis, basis rows [1, 0], [0, 1], [1, -1]: q = K1, K2 and
fl(K1 - K2), q^2 = fl(q q) (the other components add exact zeros), w = fl(q^2 - fl(kF kF)) whatever the order of a route's
operations.  T = (0, tau, t3): a leaf with (tau_in, tau_out) = (1, 2) sees tau exactly, its twin (2, 1) sees -tau, a leaf with
tau_in == tau_out sees 0 (taken as -1e-10 like green()).

Every value v is stored as two doubles, hi = float(v) and lo = float(v - hi) (lo kept to 24 bits: 2^-24 of half an ulp of
hi is far below anything a test resolves, and the file stays small); tests form (got - hi) - lo.  The values are stored once
per distinct argument tuple, `val_idx[p, b, leaf]` points into them (-1: a leaf without a formula).

The second block steers the exponent's argument: kF = 0, beta = 2, tau = 1 make it -fl(k k) on the first momentum; k runs
over the doubles next to sqrt(|x|) for x at the rounding ties of the one-kernel route's range reduction (x log2 e = n + 1/2),
at the ends of the subnormal range and far below.  `exp_*` holds exp(x) for those arguments and for 5 000 random x in
[-746, 0]; `exp_units` is exp(x) / 2^-1074 where exp(x) is subnormal (a pair of doubles cannot resolve that range)."""
import io
import os
import zipfile

import numpy as np
import mpmath as mp

mp.mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))

PARAMS = [(1.919, 3.0), (1.5, 8.0), (1.0, 0.5), (1.919, 25.0), (2.0, 50.0)]        # (kF, beta)
LAMBDAS = [1.2, 0.7, 1e-3, 50.0]                                                    # parameter set p runs with LAMBDAS[p % 4]
C8PI = 8.0 * 3.141592653589793                                                      # the double the kernels multiply by
BASIS = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, -1.0]])
STEER = dict(kF=0.0, beta=2.0, lam=1.2, tau=1.0)
K2_SHIFT, T3_SHIFT = 7, 5


def moduli(kF, beta):
    root = lambda x: float(np.sqrt(kF * kF + x / beta))
    return [0.0, 1e-160, 1e-8, 0.5 * kF, kF * (1 - 1e-8), float(np.nextafter(kF, 0.0)), kF, float(np.nextafter(kF, np.inf)), kF * (1 + 1e-8),
            1.05 * kF, 2 * kF, root(700.0), root(708.4), root(745.0), root(1000.0), 10 * kF, 100 * kF, 1e3]


def times(beta):
    b1 = float(np.nextafter(beta, 0.0))
    t = [0.0]
    for x in (1e-300, 1e-10, 1e-3, 0.3 * beta, 0.5 * beta, 0.7 * beta, b1, beta):
        t += [x, -x]
    return t


def leaf_table():
    """(type, order, tau_in, tau_out, loop_index), 1-based like FrontEnds.leafstates"""
    rows = []
    for m in (1, 2, 3):
        for n in range(6):
            rows.append((1, n, 1, 2, m))
            rows.append((1, n, 2, 1, m))
        if m == 1:
            rows.append((0, 0, 1, 1, 1))                 # a leaf without a formula, in the middle of the table
    for m in (1, 3):
        for n in range(8):
            rows.append((2, n, 1, 1, m))
    rows.append((1, 0, 3, 3, 2))                         # tau_in == tau_out
    rows.append((1, 4, 2, 2, 1))
    return np.array(rows, dtype=np.int32)


def kernel(tau, w, beta):
    if tau > 0:
        return mp.e ** (-w * tau) / (1 + mp.e ** (-w * beta))
    return -mp.e ** (-w * (tau + beta)) / (1 + mp.e ** (-w * beta))


_Q = [[0, 1], [0, 1, -1], [0, 1, -3, 2], [0, 1, -7, 12, -6], [0, 1, -15, 50, -60, 24], [0, 1, -31, 180, -390, 360, -120]]


def leibniz(tau, w, beta, n):
    """the closed form the kernels evaluate, in 60 digits: only the generator's own cross-check"""
    neg, pos = tau < 0, w >= 0
    a = (-(tau + beta) if neg else -tau) if pos else (-tau if neg else beta - tau)
    A = mp.e ** (w * a)
    g = 1 / (1 + mp.e ** (-abs(w) * beta))
    b = beta if pos else -beta
    total = mp.mpf(0)
    for k in range(n + 1):
        total += mp.binomial(n, k) * mp.polyval(list(reversed(_Q[k])), g) * a ** (n - k) * b ** k
    scale = A * (abs(a) + beta) ** n / mp.factorial(n)
    return (-1 if neg else 1) * A * total * (-1) ** n / mp.factorial(n), scale


def green_exact(tau, w, beta, n):
    tau, w, beta = mp.mpf(tau), mp.mpf(w), mp.mpf(beta)
    if n == 0:
        return kernel(tau, w, beta)
    v = (-1) ** n * mp.diff(lambda x: kernel(tau, x, beta), w, n) / mp.factorial(n)
    ref, scale = leibniz(tau, w, beta, n)
    assert abs(v - ref) <= mp.mpf(10) ** -40 * scale, (tau, w, beta, n, v, ref)
    return v


def interaction_exact(q2, lam, n):
    s = mp.mpf(q2) + mp.mpf(lam)
    return mp.mpf(C8PI) * s * (mp.mpf(lam) / s) ** n


def split(v):
    hi = float(v)
    lo = np.array([float(v - mp.mpf(hi))])
    lo = (lo.view(np.uint64) & np.uint64(0xFFFFFFFFE0000000)).view(np.float64)      # 24 significant bits
    return hi, float(lo[0])


def grid_inputs(kF, beta):
    ks, ts = moduli(kF, beta), times(beta)
    K, T = [], []
    for i, k in enumerate(ks):
        for j, t in enumerate(ts):
            K.append([[k, 0.0, 0.0], [ks[(i + K2_SHIFT) % len(ks)], 0.0, 0.0]])
            T.append([0.0, t, ts[(j + T3_SHIFT) % len(ts)]])
    return np.array(K), np.array(T)


def steering():
    ln2 = mp.log(2)
    targets = [(n + mp.mpf(0.5)) * ln2 for n in list(range(-1075, -1020)) + list(range(-1020, 0, 16))]
    targets += [mp.mpf(-708.3964185322641), mp.mpf(-745.1332191019411), mp.mpf(-1e4), mp.mpf(-1e6), mp.mpf(-1e9)]
    ks = []
    for t in targets:
        k = float(mp.sqrt(-t))
        lo = hi = k
        for _ in range(2):
            lo, hi = float(np.nextafter(lo, 0.0)), float(np.nextafter(hi, np.inf))
        cand = [lo, float(np.nextafter(lo, np.inf)), k, float(np.nextafter(k, np.inf)), hi]
        assert min(c * c for c in cand) < -t < max(c * c for c in cand), t            # the argument lands on both sides
        ks += cand
    return np.array(ks)


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    tab = leaf_table()
    L = len(tab)
    index, hi, lo = {}, [], []

    def value(key, fn):
        if key not in index:
            h, l = split(fn())
            index[key] = len(hi)
            hi.append(h)
            lo.append(l)
        return index[key]

    Ks, Ts, q2s, ws, idxs = [], [], [], [], []
    for p, (kF, beta) in enumerate(PARAMS):
        lam = LAMBDAS[p % len(LAMBDAS)]
        K, T = grid_inputs(kF, beta)
        q = np.stack([K[:, 0, 0], K[:, 1, 0], K[:, 0, 0] - K[:, 1, 0]], axis=1)      # fp64, in the documented order
        q2 = q * q
        w = q2 - kF * kF
        idx = np.full((K.shape[0], L), -1, dtype=np.int32)
        for b in range(K.shape[0]):
            for i, (ty, n, tin, tout, li) in enumerate(tab.tolist()):
                if ty == 1:
                    tau = float(T[b, tout - 1] - T[b, tin - 1])
                    if tau == 0.0:
                        tau = -1e-10
                    wv = float(w[b, li - 1])
                    idx[b, i] = value(("g", n, wv, tau, beta), lambda: green_exact(tau, wv, beta, n))
                elif ty == 2:
                    qv = float(q2[b, li - 1])
                    idx[b, i] = value(("v", n, qv, lam), lambda: interaction_exact(qv, lam, n))
        Ks.append(K); Ts.append(T); q2s.append(q2); ws.append(w); idxs.append(idx)
        print("parameter set", p, "done:", len(hi), "distinct values so far", flush=True)
    n_grid = sum(k.shape[0] for k in Ks)
    assert n_grid % 64 != 0 and Ks[0].shape[0] % 64 != 0

    steer_k = steering()
    assert len(steer_k) % 64 != 0
    steer_x = -(steer_k * steer_k)
    rng = np.random.default_rng(2025)
    exp_x = np.concatenate([np.unique(steer_x), -rng.uniform(0.0, 746.0, 5000)])
    exp_hi, exp_lo, exp_units = [], [], []
    for x in exp_x:
        e = mp.e ** mp.mpf(float(x))
        h, l = split(e)
        exp_hi.append(h); exp_lo.append(l)
        exp_units.append(float(e * mp.mpf(2) ** 1074) if e < mp.mpf(2) ** -1022 else np.nan)

    out = dict(kF=np.array([p[0] for p in PARAMS]), beta=np.array([p[1] for p in PARAMS]),
               lam=np.array([LAMBDAS[p % len(LAMBDAS)] for p in range(len(PARAMS))]),
               K=np.stack(Ks), T=np.stack(Ts), q2=np.stack(q2s), w=np.stack(ws), val_idx=np.stack(idxs),
               val_hi=np.array(hi), val_lo=np.array(lo),
               leaf_type=tab[:, 0], leaf_order=tab[:, 1], tau_in=tab[:, 2], tau_out=tab[:, 3], loop_index=tab[:, 4], basis=BASIS,
               steer_k=steer_k, steer_x=steer_x, steer_param=np.array([STEER["kF"], STEER["beta"], STEER["lam"], STEER["tau"]]),
               exp_x=exp_x, exp_hi=np.array(exp_hi), exp_lo=np.array(exp_lo), exp_units=np.array(exp_units))
    path = os.path.join(HERE, "leaf_edges.npz")
    write_npz(path, out)
    print("leaf_edges.npz:", n_grid, "grid samples x", L, "leaves,", len(hi), "distinct values,", len(steer_k), "steering samples,",
          len(exp_x), "exp arguments,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
