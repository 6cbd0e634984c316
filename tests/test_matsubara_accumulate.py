"""The Matsubara projection on the device (include/fdg.h: fdg_accumulate_device_matsubara, fdg_mc_accumulate_device_matsubara;
GraphFunc.accumulate_matsubara; vegas.MatsubaraProjection).  With t = w[b] root_k(b), tau = T[b][tout_k] - T[b][tin_k] and
(s, c) = fdg_matsubara_phase(tau, beta, freq[f], fermionic), the samples of bin j add t c, t s and the squares of both to entry [j, f, k].

Host reference: the oracle's roots (in the Monte-Carlo form the same handle's mc_eval_device roots) projected in numpy.  The phases of the
reference are fdg_matsubara_phase's bits: they are formed by the numpy restatement of csrc/fdg_matsubara.h -- a call of
capi.matsubara_phase per (sample, time pair, frequency) costs 9 microseconds and a table has up to 1.6 million entries -- and every
table is compared bit for bit with capi.matsubara_phase on every 97th entry before it is used (tests/test_matsubara_host.py compares
the two on 10^4 points and the edges).  Tolerance, as in tests/test_moments_accumulate.py: |d| <= 1e-12 max(1, sum |t|) per entry for
the sums of t c and t s, 1e-12 max(1, sum (t c)^2) (resp. (t s)^2) for the second moments.  The helpers are copies of that file's and of
tests/test_matsubara_host.py's."""
import functools
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-12
SPECS = {"interp": False, "hip": True, "isa": "isa"}
B0, BETA, N_TAU = 8_229, 3.0, 4
FREQ = tuple(int(v) for v in np.random.default_rng(99).permutation(np.arange(-32, 32)))      # 64 distinct n of both signs, 0 and -1 among them
CASES = [(1, 1), (7, 3), (1, 64), (256, 64)]                                                  # (n_bin, n_freq); the last: n_bin n_freq = FDG_BIN_MAX


# ---- numpy mirrors (copies of tests/test_matsubara_host.py's) ------------------------------------------------------------------------ #
TWO_OVER_PI, P1, P1T = np.float64(0.6366197723675814), np.float64(1.5707963267341256), np.float64(6.077100506506192e-11)
S = [np.float64(v) for v in (-0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06,
                             -2.505210838544172e-08, 1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15)]
CC = [np.float64(v) for v in (0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07,
                              2.08767569878681e-09, -1.1470745597729725e-11, 4.779477332387385e-14)]


def mirror_sincos(x):
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


def phase_table(tau, beta, freq, fermionic):
    """(s, c) [B, F] of fdg_matsubara_phase(tau[b], beta, freq[f], fermionic): the header's recipe in numpy, one operation per line,
    checked bit for bit against the library's routine on every 97th entry"""
    mult = (2 * np.asarray(freq, dtype=np.int64) + (1 if fermionic else 0)).astype(np.float64)
    x = np.asarray(tau, dtype=np.float64) / np.float64(beta)
    m = x[:, None] * mult[None, :]
    h = m * 0.5
    fl = np.floor(h)
    r = h - fl
    th = r * np.float64(6.283185307179586)
    s, c = mirror_sincos(th)
    for i in range(0, s.size, 97):
        b, f = divmod(i, s.shape[1])
        gs, gc = capi.matsubara_phase(float(tau[b]), float(beta), int(freq[f]), fermionic)
        assert np.float64(gs).view(np.uint64) == s[b, f].view(np.uint64) and np.float64(gc).view(np.uint64) == c[b, f].view(np.uint64), (b, f)
    return s, c


def host_projection(roots, T, tin, tout, freq, beta, fermionic, bins, n_bin, w=None, base=0, live=None):
    """(re, im, re2, im2, scale) [n_bin, F, R]: the sums over the samples whose bin is in range of t c, t s and their squares, and of |t|;
    columns of roots outside ``live`` stay 0.  Roots with the same time pair share their phases (the same bits)."""
    B, R = roots.shape
    F = len(freq)
    j = np.zeros(B, dtype=np.int64) if bins is None else bins.astype(np.int64) - base
    ok = (j >= 0) & (j < n_bin)
    out = np.zeros((5, n_bin, F, R))
    onehot = np.zeros((n_bin, int(ok.sum())))                                 # [bin, sample in range]: a sum per bin is one product
    onehot[j[ok], np.arange(onehot.shape[1])] = 1.0
    phases = {}
    for k in (range(R) if live is None else live):
        pair = (int(tin[k]), int(tout[k]))
        if pair not in phases:
            phases[pair] = phase_table(T[ok, pair[1] - 1] - T[ok, pair[0] - 1], beta, freq, fermionic)
        s, c = phases[pair]
        t = roots[ok, k] if w is None else w[ok] * roots[ok, k]
        tre, tim = t[:, None] * c, t[:, None] * s
        for i, v in enumerate((tre, tim, tre * tre, tim * tim, np.broadcast_to(np.abs(t)[:, None], tre.shape))):
            out[i, :, :, k] = onehot @ v
    return out


def assert_projection(got, want, what):
    """got [4, n_bin, F, R] against host_projection's five arrays, with the tolerances of the module docstring"""
    for i, scale in enumerate((want[4], want[4], want[2], want[3])):
        d = np.abs(got[i] - want[i])
        bad = d > TOL * np.maximum(1.0, scale)
        assert not bad.any(), (what, i, np.argwhere(bad)[:4], d.max())


def make_bins(rng, B, n_bin, base=0):
    """uniform bins in [base, base + n_bin), 1 % out of range on each side"""
    b = rng.integers(0, n_bin, size=B)
    out = rng.random(B)
    b = np.where(out < 0.01, -1, np.where(out < 0.02, n_bin, b))
    return (b + base).astype(np.int32)


def to_tiles(x):
    B, C = x.shape
    T = (B + 63) // 64
    full = np.full((T * 64, C), np.nan)
    full[:B] = x
    return np.ascontiguousarray(full.reshape(T, 64, C).transpose(0, 2, 1))


def leaves(cuda, h_leaf, layout):
    import torch
    if layout == "row":
        return torch.from_numpy(h_leaf).to(cuda)
    if layout == "leaf_major":
        return torch.from_numpy(np.ascontiguousarray(h_leaf.T)).to(cuda).t()
    return torch.from_numpy(to_tiles(h_leaf)).to(cuda)


# ---- the shared inputs and references of the parity cases: computed once, never written to ------------------------------------------- #
@functools.lru_cache(maxsize=None)
def batch(name):
    t = workloads.get(name)
    h_leaf = oracle.philox_uniform(B0, t.n_leaf, 31)
    rng = np.random.default_rng(7)
    T = rng.uniform(0.0, BETA, size=(B0, N_TAU))
    T[:, 0] = 0.0                                                             # T[1] = 0, as the examples fix it
    w = rng.uniform(-1.0, 2.0, size=B0)
    bins = {n_bin: make_bins(rng, B0, n_bin, base=1) for n_bin, _ in CASES if n_bin > 1}
    tin, tout = workloads.root_times(name)
    assert (tin == tout).any() and (tin != tout).any()                        # one root whose two times coincide: its phase is 1 at every frequency
    return t, h_leaf, oracle.eval_static(t, h_leaf), T, w, bins, tin, tout


@functools.lru_cache(maxsize=None)
def reference(name, n_bin, n_freq, weighted, fermionic):
    t, _, roots, T, w, bins, tin, tout = batch(name)
    return host_projection(roots, T, tin, tout, FREQ[:n_freq], BETA, fermionic, bins.get(n_bin), n_bin, w if weighted else None, base=1)


@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("name", ["sigma2", "parquet_sigma4"])
def test_projection_parity(libfdg, cuda, name, spec):
    import torch
    t, h_leaf, _, h_T, h_w, h_bins, tin, tout = batch(name)
    f = fd.compile_table(t, specialize=SPECS[spec])
    w = torch.from_numpy(h_w).to(cuda)
    d_T = torch.from_numpy(h_T).to(cuda)
    d_bins = {n: torch.from_numpy(b).to(cuda) for n, b in h_bins.items()}
    for layout in ["row", "leaf_major"] + (["tiled"] if spec == "isa" else []):
        leaf = leaves(cuda, h_leaf, layout)
        for n_bin, n_freq in CASES:
            for weighted in (False, True):
                for fermionic in (True, False):
                    acc, q_re, q_im = f.accumulate_matsubara(leaf, d_T, FREQ[:n_freq], tin, tout, BETA, fermionic, d_bins.get(n_bin), n_bin,
                                                             w if weighted else None, bin_base=1, n_sample=B0)
                    assert acc.shape == q_re.shape == q_im.shape == (n_bin, n_freq, t.n_root) and acc.dtype == torch.complex128
                    got = np.stack([acc.real.cpu().numpy(), acc.imag.cpu().numpy(), q_re.cpu().numpy(), q_im.cpu().numpy()])
                    assert_projection(got, reference(name, n_bin, n_freq, weighted, fermionic), (layout, n_bin, n_freq, weighted, fermionic))


def random_table(rng, n_leaf=6, n_root=19, missing=7):
    """n_root roots over n_leaf leaves -- sums and products of two or three of them with random factors --, root ``missing`` naming no graph"""
    lv = [fd.Graph([]) for _ in range(n_leaf)]
    gs = []
    for k in range(n_root - 1):
        ch = [lv[i] for i in rng.choice(n_leaf, size=2 + k % 2, replace=False)]
        gs.append(fd.Graph(ch, subgraph_factors=[float(x) for x in rng.uniform(-1.5, 1.5, len(ch))], operator=fd.Prod() if k % 3 else fd.Sum()))
    ids = [g.id for g in gs]
    ids.insert(missing, 424_242)
    t, _, _ = lower(gs, root=ids)
    assert t.n_root == n_root and int(t.root_slot[missing]) == FDG_NO_ROOT
    return t


def test_chunks_root_slices_missing_root_and_poisoned_samples(libfdg, cuda):
    """FDG_ROOT_SCRATCH_MB = 1 with 19 roots: chunks of 6 848 samples, eleven of them; two slices of 16 roots; the column of the root that
    does not exist keeps its sentinels in all four arrays; inf and nan leaves on samples whose bin is out of range reach no sum."""
    import torch
    rng = np.random.default_rng(5)
    t = random_table(rng)
    R, B, n_bin, n_tau, missing = t.n_root, 70_003, 3, 5, 7
    freq, live = (0, 2, -1, -7, 11), [k for k in range(R) if k != missing]
    f = fd.compile_table(t, specialize="isa", options={"FDG_ROOT_SCRATCH_MB": "1"})
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 17) + 0.25
    h_bins = make_bins(rng, B, n_bin)
    out_of_range = np.flatnonzero((h_bins < 0) | (h_bins >= n_bin))
    assert out_of_range.size > 1000
    h_leaf[out_of_range[0::2]] = np.inf
    h_leaf[out_of_range[1::2]] = np.nan
    h_T = rng.uniform(0.0, BETA, size=(B, n_tau))
    pairs = [(1, 2), (3, 5), (4, 4)]                                          # three distinct time pairs over the 19 roots
    tin, tout = [pairs[k % 3][0] for k in range(R)], [pairs[k % 3][1] for k in range(R)]
    tin[missing], tout[missing] = 0, 99                                       # (the labels of a root that does not exist are not read)
    h_w = rng.uniform(0.0, 1.0, size=B)
    sums = torch.zeros((4, n_bin, len(freq), R), dtype=torch.float64, device=cuda)
    sums[:, :, :, missing] = torch.tensor([-7.0, 5.0, 3.0, -2.0], dtype=torch.float64, device=cuda)[:, None, None]
    f.accumulate_matsubara(leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_T).to(cuda), freq, tin, tout, BETA, True,
                           torch.from_numpy(h_bins).to(cuda), n_bin, torch.from_numpy(h_w).to(cuda), sums=sums, n_sample=B)
    got = sums.cpu().numpy()
    assert np.isfinite(got).all()
    for i, v in enumerate((-7.0, 5.0, 3.0, -2.0)):
        assert (got[i, :, :, missing] == v).all()
    with np.errstate(invalid="ignore"):
        roots = oracle.eval_static(t, h_leaf)
    want = host_projection(roots, h_T, tin, tout, freq, BETA, True, h_bins, n_bin, h_w, live=live)
    assert_projection(got[:, :, :, live], want[:, :, :, live], "19 roots")


def test_repeatable_additive_and_shards(libfdg, cuda):
    import torch
    name, n_bin, n_freq = "parquet_sigma4", 7, 3
    t, h_leaf, _, h_T, h_w, h_bins, tin, tout = batch(name)
    f = fd.compile_table(t, specialize="isa")
    leaf, d_T, w, bins = leaves(cuda, h_leaf, "row"), torch.from_numpy(h_T).to(cuda), torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins[n_bin]).to(cuda)
    want = reference(name, n_bin, n_freq, True, True)
    rng = np.random.default_rng(3)
    h0 = rng.uniform(-3.0, 3.0, size=(4, n_bin, n_freq, t.n_root))
    h0[2:] = np.abs(h0[2:])
    p0 = torch.from_numpy(h0).to(cuda)

    def run(sums, lo=0, hi=B0):
        f.accumulate_matsubara(leaf[lo:hi], d_T[lo:hi], FREQ[:n_freq], tin, tout, BETA, True, bins[lo:hi], n_bin, w[lo:hi], sums=sums, bin_base=1)
        return sums

    a, b = run(p0.clone()), run(p0.clone())
    torch.cuda.synchronize()
    assert torch.equal(a, b)                                                  # no atomics: the same arguments give the same bits
    on_top = want.copy()
    on_top[:4] += h0
    on_top[4] += np.abs(h0[:2]).max(axis=0)                                   # (the scale of the first moments grows by what was there)
    assert_projection(a.cpu().numpy(), on_top, "on top")
    run(a)                                                                    # a second call into the same buffers adds again
    twice = on_top.copy()
    twice[:4] += want[:4]
    twice[4] += want[4]
    assert_projection(a.cpu().numpy(), twice, "twice")
    whole = run(torch.zeros_like(p0))
    half = B0 // 2 + 13                                                       # (not a multiple of the tile)
    shards = run(run(torch.zeros_like(p0), 0, half), half, B0)
    assert_projection(whole.cpu().numpy(), want, "whole")
    both = want.copy()
    both[:4] = whole.cpu().numpy()
    assert_projection(shards.cpu().numpy(), both, "two shards")


@pytest.mark.parametrize("route", ["fused", "split", "isa"])
def test_mc_projection_routes(libfdg, cuda, fdgopt, route):
    import torch
    z = dict(np.load(os.path.join(GOLD, "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    R, B, dim, n_loop, n_tau = t.n_root, B0, 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam, n_bin, freq = 1.919, BETA, 1.2, 5, (0, -1, 3)
    rng = np.random.default_rng(13)
    h_K, h_T = rng.uniform(-2.0, 2.0, size=(B, n_loop * dim)), rng.uniform(0.0, beta, size=(B, n_tau))
    tin, tout = [1] * R, [1 + k % n_tau for k in range(R)]
    st = torch.cuda.current_stream().cuda_stream
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    fdgopt.set("FDG_MC_ROUTE", route)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    h_w, h_bins = rng.uniform(0.0, 1.0, size=B), make_bins(rng, B, n_bin, base=1)
    w, bins = torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins).to(cuda)
    want = None
    for major in ("component", "sample"):
        if major == "component":
            dK, dT = torch.from_numpy(np.ascontiguousarray(h_K.T)).to(cuda), torch.from_numpy(np.ascontiguousarray(h_T.T)).to(cuda)
            ks, kc, ts, tc = 1, B, 1, B
        else:
            dK, dT = torch.from_numpy(h_K).to(cuda), torch.from_numpy(h_T).to(cuda)
            ks, kc, ts, tc = n_loop * dim, 1, n_tau, 1
        if want is None:
            root = torch.zeros((B, R), dtype=torch.float64, device=cuda)
            f.handle.mc_eval_device(dK.data_ptr(), ks, kc, dT.data_ptr(), ts, tc, kF, beta, lam, root.data_ptr(), R, 1, B, st)
            want = host_projection(root.cpu().numpy(), h_T, tin, tout, freq, beta, True, h_bins, n_bin, h_w, base=1)
        sums = torch.zeros((4, n_bin, len(freq), R), dtype=torch.float64, device=cuda)
        desc, _k = capi.make_matsubara(freq, True, tin, tout, beta, n_tau, *[sums[i].data_ptr() for i in range(4)])
        f.handle.mc_accumulate_device_matsubara(dK.data_ptr(), ks, kc, dT.data_ptr(), ts, tc, kF, beta, lam, bins.data_ptr(), 1, n_bin,
                                                w.data_ptr(), desc, B=B, stream=st)
        torch.cuda.synchronize()
        assert_projection(sums.cpu().numpy(), want, (route, major))


def test_training_histograms_and_moments_tie_bit_for_bit(libfdg, cuda):
    """With the VEGAS block on, d_hist and d_hist_bin are accumulate_vegas[_binned]'s bits, and d_acc, d_acc2 the moments calls'."""
    import torch
    name, n_bin, n_freq, D, G, seed, off = "parquet_sigma4", 7, 3, 5, 16, 77, 1_000
    t, h_leaf, _, h_T, h_w, h_bins, tin, tout = batch(name)
    R = t.n_root
    f = fd.compile_table(t, specialize="isa")
    leaf, d_T, w = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_T).to(cuda), torch.from_numpy(h_w).to(cuda)
    bins = torch.from_numpy(h_bins[n_bin]).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    strides = (leaf.stride(2), leaf.stride(1), leaf.stride(0))
    coef = np.linspace(-1.0, 2.0, R)
    for binned in (False, True):
        nb = n_bin if binned else 1
        d_bin = bins.data_ptr() if binned else 0
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
        acc, acc2, hist, hist_bin = z(nb, R), z(nb, R), z(D, G), z(nb)
        if binned:
            f.handle.accumulate_device_vegas_binned(leaf.data_ptr(), *strides, d_bin, 1, nb, w.data_ptr(), coef, seed, off, D, G,
                                                    acc.data_ptr(), acc2.data_ptr(), hist.data_ptr(), hist_bin.data_ptr(), B0, st)
        else:
            f.handle.accumulate_device_vegas(leaf.data_ptr(), *strides, w.data_ptr(), coef, seed, off, D, G, acc.data_ptr(), acc2.data_ptr(),
                                             hist.data_ptr(), B0, st)
        for with_moments in (True, False):
            m_acc, m_acc2, m_hist, m_hist_bin, sums = z(nb, R), z(nb, R), z(D, G), z(nb), z(4, nb, n_freq, R)
            desc, _k = capi.make_matsubara(FREQ[:n_freq], True, tin, tout, BETA, N_TAU, *[sums[i].data_ptr() for i in range(4)],
                                           d_T.data_ptr(), d_T.stride(0), d_T.stride(1))
            f.handle.accumulate_device_matsubara(leaf.data_ptr(), *strides, d_bin, 1, nb, w.data_ptr(), desc, coef, seed, off, D, G,
                                                 m_acc.data_ptr() if with_moments else 0, m_acc2.data_ptr() if with_moments else 0,
                                                 m_hist.data_ptr(), m_hist_bin.data_ptr() if binned else 0, B0, st)
            torch.cuda.synchronize()
            assert torch.equal(m_hist, hist) and hist.abs().sum().item() > 0, (binned, with_moments)
            if binned:
                assert torch.equal(m_hist_bin, hist_bin) and hist_bin.abs().sum().item() > 0
            if with_moments:
                assert torch.equal(m_acc, acc) and torch.equal(m_acc2, acc2)
            assert_projection(sums.cpu().numpy(), reference(name, nb, n_freq, True, True), (binned, with_moments))


def test_known_answer_through_the_driver(libfdg, cuda):
    """One fermionic order-0 propagator from T[1] = 0 to T[2] = tau, integrated over tau in [0, beta] against e^{i omega_n tau}:
    1 / (eps - i omega_n), eps = k^2 - kF^2, for both signs of eps and n = 0, 1, -3.  This pins the sign convention, the 1-based labels
    and the fermionic frequencies.  Sample count: with plain uniform sampling of tau (the map of the first iteration) the standard
    deviation of beta G cos / sin is at most 0.94, and 1 % of the smallest |1 / (eps - i omega_n)| (0.19, n = -3) asks for 2.31e5
    samples (numpy mirror of the integrand on the host, 4e5 uniform samples per case); the next power of two is taken.  The generator
    is counter-based and the seed fixed: the same samples every run."""
    a = fd.Graph([])
    t, _, _ = lower([fd.Graph([a], subgraph_factors=[1.0])])
    assert t.n_leaf == 1 and t.n_root == 1
    kF, beta, N = 1.0, BETA, 1 << 18
    one = np.array([1], np.int32)
    tab, _keep = capi.make_leaf_tables(one, np.array([0], np.int32), one, np.array([2], np.int32), one, np.array([[1.0]]), 3, 2)
    mz = vegas.MatsubaraProjection(freq=(0, 1, -3), fermionic=True, root_tau_in=(1,), root_tau_out=(2,))
    for k in (1.5, 0.5):
        eps = k * k - kF * kF
        f = fd.compile_table(t, specialize="isa")
        res = vegas.vegas_integrate(f, tab, [0.0], [beta], [4], kF, beta, 0.0, n_iter=2, n_sample=N, n_grid=32, seed=2_025, fixed=[k, 0.0, 0.0, 0.0, 0.0],
                                    device=cuda, matsubara=mz)
        assert res.mean.shape == res.stderr.shape == (3, 1) and np.iscomplexobj(res.mean)
        for i, n in enumerate(mz.freq):
            exact = 1.0 / (eps - 1j * (2 * n + 1) * np.pi / beta)
            got, err = res.mean[i, 0], res.stderr[i, 0]
            for j in range(2):                                                # the first iteration alone: the uniform map the count was sized for
                e = res.iterations[j][1][i, 0]
                print(f"eps {eps:+.2f} n {n:+d} iteration {j}: {res.iterations[j][0][i, 0]:.6f} +- ({e.real:.2e}, {e.imag:.2e})")
            print(f"eps {eps:+.2f} n {n:+d}: {got:.6f} +- ({err.real:.2e}, {err.imag:.2e}); exact {exact:.6f}")
            e0 = res.iterations[0][1][i, 0]
            assert max(e0.real, e0.imag) < 0.01 * abs(exact) and max(err.real, err.imag) < 0.01 * abs(exact), (eps, n, e0, err)
            assert abs(got.real - exact.real) <= 5 * err.real and abs(got.imag - exact.imag) <= 5 * err.imag, (eps, n, got, exact, err)
