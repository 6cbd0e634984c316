"""Frequency observables on the device (include/fdg.h: fdg_accumulate_device_freq_observables,
fdg_mc_accumulate_device_freq_observables; GraphFunc.accumulate_freq_observables, vegas.FrequencyObservables): with tre_k, tim_k the
parts of w_g(k) root_k times the phase of its own time pair at frequency f, a_m / b_m the left folds over k of coef[m][k] tre_k /
coef[m][k] tim_k and z = (a, b), d_fobs[j][f][p] += z_p and d_fcov[j][f][p][q] += z_p z_q over the samples of bin j.

Host reference: capi.freq_observables_reference on the oracle's roots (on the handle's own mc_eval_device roots for the Monte-Carlo
form); its phases are the library's fdg_matsubara_phase, so the per-sample z carries the kernel's bits and only the order of the sums
differs.  A call of that routine per (sample, time pair, frequency) costs microseconds, so the large tables (64 frequencies, 70 003
samples) are handed to the reference ready-made by tests/test_matsubara_accumulate.py's phase_table -- the header's recipe in numpy,
compared bit for bit with the library's routine on every 97th entry -- and the smaller cases go through the routine itself.  Tolerance, the convention of tests/test_moments_accumulate.py: |got - want| <= 1e-12 max(1, sum |terms|), the terms |z_p| of
an entry of d_fobs and |z_p z_q| of an entry of d_fcov.  The other blocks of a call carry the bits of the same call without fo."""
import functools
import math
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from test_matsubara_accumulate import BETA, FREQ, batch, leaves, make_bins, phase_table, random_table
from test_observables_accumulate import obs_call, random_coef, twin_roots
from test_weight_groups_accumulate import D0, G0, SETS, assert_bits, leaf_strides

pytestmark = pytest.mark.gpu

TOL = 1e-12
B0 = 8_229
SENTINEL = -7.0
CASES = [(1, 1, 1), (7, 3, 2), (1, 64, 8), (256, 64, 3)]          # (n_bin, n_freq, M): the last is FDG_BIN_MAX rows, (1, 64, 8) all 152 columns


def fobs_call(f, leaf, B, cuda, coef, mz, w=None, rg=None, sets=None, bins=None, n_bin=1, bin_base=0, train=None, tcoef=None, ocoef=None,
              moments=False, proj=False, out=None, fill=0.0):
    """One fdg_accumulate_device_freq_observables call.  mz: (T tensor, freq, fermionic, tin, tout); w: None, a [B] or (with rg and
    sets) a [n_group, B] CUDA tensor; train: (seed, offset, D, G) or None; ocoef: the coefficients of an ob block or None; proj: the
    four per-root arrays of mz too; out: the dict of a previous call, added to; fill: what fobs and fcov start from.  Returns the dict
    of output tensors."""
    import torch
    R, M = f.n_root, len(coef)
    T, freq, fermionic, tin, tout = mz
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=cuda)
    if out is None:
        out = {"fobs": z(n_bin, len(freq), 2 * M) + fill, "fcov": z(n_bin, len(freq), 2 * M, 2 * M) + fill}
        if ocoef is not None:
            out.update(obs=z(n_bin, len(ocoef)), cov=z(n_bin, len(ocoef), len(ocoef)))
        if moments:
            out.update(acc=z(n_bin, R), acc2=z(n_bin, R))
        if train:
            out["hist"] = z(train[2], train[3])
            if bins is not None:
                out["hist_bin"] = z(n_bin)
        if proj:
            out["mz"] = z(4, n_bin, len(freq), R)
    wg = None
    if rg is not None:
        wg, _keep = capi.make_weight_groups(rg, sets, w.stride(0))
    p = [out["mz"][i].data_ptr() if "mz" in out else 0 for i in range(4)]
    desc, _keep2 = capi.make_matsubara(freq, fermionic, tin, tout, BETA, T.shape[1], *p, T.data_ptr(), T.stride(0), T.stride(1))
    ob = None
    if ocoef is not None:
        ob, _keep3 = capi.make_observables(ocoef, out["obs"].data_ptr(), out["cov"].data_ptr())
    fo, _keep4 = capi.make_freq_observables(coef, out["fobs"].data_ptr(), out["fcov"].data_ptr())
    seed, off, D, G = train or (0, 0, 0, 0)
    f.handle.accumulate_device_freq_observables(leaf.data_ptr(), *leaf_strides(leaf), 0 if bins is None else bins.data_ptr(), bin_base, n_bin,
                                                0 if w is None else w.data_ptr(), fo, desc, ob, wg, tcoef, seed, off, D, G,
                                                out["acc"].data_ptr() if "acc" in out else 0, out["acc2"].data_ptr() if "acc2" in out else 0,
                                                out["hist"].data_ptr() if train else 0, out["hist_bin"].data_ptr() if "hist_bin" in out else 0,
                                                B, torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    return out


def assert_fobs(got, want, what, fill=0.0):
    """got: the dict of fobs_call (or a pair of arrays); want: capi.freq_observables_reference's tuple.  Entries of rows without a term
    (nan in the reference) must hold ``fill`` untouched; the others ``fill`` plus the reference within the tolerance."""
    o, c = (got["fobs"].cpu().numpy(), got["fcov"].cpu().numpy()) if isinstance(got, dict) else got
    for key, g, ref, scale in (("fobs", o, want[0], want[2]), ("fcov", c, want[1], want[3])):
        dead = np.isnan(ref)
        assert (g[dead] == fill).all(), (what, key, "a row without a term was written")
        err = np.abs(g[~dead] - fill - ref[~dead])
        bound = TOL * np.maximum(1.0, scale[~dead])
        print(what, key, "max |got - want| / bound:", float((err / bound).max()) if err.size else 0.0)
        assert (err <= bound).all(), (what, key, float((err / bound).max()))
    assert_bits(c, c.transpose(0, 1, 3, 2), (what, "fcov and its mirror"))


# ---- the shared inputs and references of the parity cases: computed once, never written to ------------------------------------------- #
NAME = "parquet_sigma4"


@functools.lru_cache(maxsize=None)
def phase_tables(fermionic):
    """{(tin, tout): (s, c) [B0, 64]} over all of FREQ for the time pairs of the workload's roots, once"""
    _, _, _, T, _, _, tin, tout = batch(NAME)
    pairs = sorted(set(zip((int(v) for v in tin), (int(v) for v in tout))))
    return {p: phase_table(T[:, p[1] - 1] - T[:, p[0] - 1], BETA, FREQ, fermionic) for p in pairs}


@functools.lru_cache(maxsize=None)
def case_coef(n_bin, n_freq, M):
    R = workloads.get(NAME).n_root
    zero_row = None if M == 1 else M // 2
    c = random_coef(np.random.default_rng(1000 * M + n_freq), M, R, zero_row)
    assert M == 1 or ((c == 0.0).any() and not c[zero_row].any())
    return c


@functools.lru_cache(maxsize=None)
def reference(n_bin, n_freq, M, weighted, fermionic):
    _, _, roots, T, w, bins, tin, tout = batch(NAME)
    tables = {p: (s[:, :n_freq], c[:, :n_freq]) for p, (s, c) in phase_tables(fermionic).items()}
    return capi.freq_observables_reference(roots, T, tin, tout, FREQ[:n_freq], BETA, fermionic, case_coef(n_bin, n_freq, M),
                                           w if weighted else None, None, bins.get(n_bin), n_bin, 1, phases=tables)


# ---- 1. against numpy ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("case", CASES, ids=lambda c: "bins%d-freq%d-M%d" % c)
def test_parity(libfdg, cuda, case):
    import torch
    n_bin, n_freq, M = case
    t, h_leaf, _, h_T, h_w, h_bins, tin, tout = batch(NAME)
    f = fd.compile_table(t, specialize="isa")
    leaf, d_T, w = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_T).to(cuda), torch.from_numpy(h_w).to(cuda)
    bins = None if n_bin == 1 else torch.from_numpy(h_bins[n_bin]).to(cuda)
    coef = case_coef(*case)
    zero_row = None if M == 1 else M // 2
    for weighted in (False, True):
        for fermionic in (True, False):
            fobs = torch.full((n_bin, n_freq, 2 * M), SENTINEL, dtype=torch.float64, device=cuda)
            fcov = torch.full((n_bin, n_freq, 2 * M, 2 * M), SENTINEL, dtype=torch.float64, device=cuda)
            o, c = f.accumulate_freq_observables(leaf, d_T, FREQ[:n_freq], tin, tout, BETA, coef, fermionic, bins, n_bin, w if weighted else None,
                                                 fobs=fobs, fcov=fcov, bin_base=1, n_sample=B0)
            torch.cuda.synchronize(cuda)
            assert o is fobs and c is fcov
            want = reference(n_bin, n_freq, M, weighted, fermionic)
            if zero_row is not None:                                          # its components keep the sentinel
                assert np.isnan(want[0][:, :, [zero_row, M + zero_row]]).all()
                assert (o[:, :, [zero_row, M + zero_row]] == SENTINEL).all().item()
            assert np.isfinite(np.delete(want[0], [] if zero_row is None else [zero_row, M + zero_row], axis=2)).all()
            assert_fobs((o.cpu().numpy(), c.cpu().numpy()), want, (case, weighted, fermionic), fill=SENTINEL)


def test_parity_with_a_missing_root(libfdg, cuda):
    """19 roots of which root 7 names no graph, three time pairs, (n_bin, n_freq, M) = (7, 3, 2) and a row whose only factor sits on the
    missing root: that row has no term."""
    import torch
    rng = np.random.default_rng(21)
    t = random_table(rng)
    R, missing, n_bin, freq = t.n_root, 7, 7, (2, -1, 0)
    exists = np.arange(R) != missing
    f = fd.compile_table(t, specialize="isa")
    h_leaf = oracle.philox_uniform(B0, t.n_leaf, 41) + 0.25
    roots = oracle.eval_static(t, h_leaf)
    h_T, h_w, h_bins = rng.uniform(0.0, BETA, size=(B0, 5)), rng.uniform(-1.0, 2.0, size=B0), make_bins(rng, B0, n_bin, base=1)
    pairs = [(1, 2), (3, 5), (4, 4)]
    tin, tout = [pairs[k % 3][0] for k in range(R)], [pairs[k % 3][1] for k in range(R)]
    tin[missing], tout[missing] = 0, 99                                       # (the labels of a root that does not exist are not read)
    coef = random_coef(rng, 3, R)
    coef[1] = 0.0
    coef[1, missing] = 2.0
    coef[:, missing] = np.where(coef[:, missing] == 0.0, 1.5, coef[:, missing])   # every row names the missing root: never a term
    leaf, d_T, w, bins = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_T).to(cuda), torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins).to(cuda)
    for fermionic in (True, False):
        want = capi.freq_observables_reference(roots, h_T, tin, tout, freq, BETA, fermionic, coef, h_w, None, h_bins, n_bin, 1, exists)
        assert np.isnan(want[0][:, :, [1, 4]]).all() and np.isfinite(want[0][:, :, [0, 2, 3, 5]]).all()
        got = fobs_call(f, leaf, B0, cuda, coef, (d_T, freq, fermionic, tin, tout), w=w, bins=bins, n_bin=n_bin, bin_base=1, fill=SENTINEL)
        assert_fobs(got, want, ("missing root", fermionic), fill=SENTINEL)


# ---- 2. exact ties ------------------------------------------------------------------------------------------------------------------------ #
def test_bosonic_zero_frequency_is_the_unprojected_observable(libfdg, cuda):
    """One bosonic frequency n = 0: the phase is exactly (0, 1), so every imaginary component and every product with one is exactly 0,
    and the real components and their products are the _observables call's d_obs / d_cov for the same coefficients."""
    import torch
    t, h_leaf, roots, h_T, h_w, h_bins, tin, tout = batch(NAME)
    f = fd.compile_table(t, specialize="isa")
    M, n_bin = 3, 7
    coef = random_coef(np.random.default_rng(77), M, t.n_root)
    leaf, d_T, w = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_T).to(cuda), torch.from_numpy(h_w).to(cuda)
    bins = torch.from_numpy(h_bins[n_bin]).to(cuda)
    got = fobs_call(f, leaf, B0, cuda, coef, (d_T, (0,), False, tin, tout), w=w, bins=bins, n_bin=n_bin, bin_base=1)
    o, c = got["fobs"].cpu().numpy()[:, 0], got["fcov"].cpu().numpy()[:, 0]
    assert (o[:, M:] == 0).all() and (c[:, M:, :] == 0).all() and (c[:, :, M:] == 0).all()
    ref = obs_call(f, leaf, B0, cuda, coef, w=w, bins=bins, n_bin=n_bin, bin_base=1)
    want = capi.observables_reference(roots, coef, h_w, None, h_bins[n_bin], n_bin, 1)
    for key, g, r, scale in (("obs", o[:, :M], ref["obs"].cpu().numpy(), want[2]), ("cov", c[:, :M, :M], ref["cov"].cpu().numpy(), want[3])):
        assert np.abs(r).max() > 0
        ratio = np.abs(g - r) / (TOL * np.maximum(1.0, scale))
        print("n = 0 against the observables call,", key, "max |d| / bound:", float(ratio.max()))
        assert (ratio <= 1.0).all(), key


# ---- 3. beside the other blocks ---------------------------------------------------------------------------------------------------------- #
def test_other_blocks_keep_their_bits(libfdg, cuda):
    """Training, d_hist_bin, per-root moments, the four arrays of mz and a real ob all present: each is bit-equal to the _observables
    call without fo; and with mz's four arrays left out, fobs and fcov keep their own bits."""
    import torch
    t, h_leaf, roots, h_T, h_w1, h_bins, tin, tout = batch(NAME)
    f = fd.compile_table(t, specialize="isa")
    R, n_bin, freq = t.n_root, 7, (0, -3, 5)
    rg = [0, 1, 1, 2]
    h_w = np.abs(np.random.default_rng(7).uniform(-1.0, 2.0, size=(3, B0))) + 0.1
    w, bins, d_T = torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins[n_bin]).to(cuda), torch.from_numpy(h_T).to(cuda)
    leaf = leaves(cuda, h_leaf, "tiled")
    ocoef = random_coef(np.random.default_rng(9), 3, R)
    coef = random_coef(np.random.default_rng(10), 2, R)
    tcoef = [0.5, -1.25, 2.0, 1.0]
    mz = (d_T, freq, True, tin, tout)
    blocks = dict(bins=bins, n_bin=n_bin, bin_base=1, train=(9, 4_000, D0, G0))
    ref = obs_call(f, leaf, B0, cuda, ocoef, w=w, rg=rg, sets=SETS, tcoef=tcoef, moments=True, mz=mz, **blocks)
    got = fobs_call(f, leaf, B0, cuda, coef, mz, w=w, rg=rg, sets=SETS, tcoef=tcoef, ocoef=ocoef, moments=True, proj=True, **blocks)
    assert set(ref) == set(got) - {"fobs", "fcov"} == {"obs", "cov", "acc", "acc2", "hist", "hist_bin", "mz"}
    for key in ref:
        assert np.abs(ref[key].cpu().numpy()).max() > 0, key
        assert_bits(got[key].cpu().numpy(), ref[key].cpu().numpy(), ("beside the frequency observables", key))
    want = capi.freq_observables_reference(roots, h_T, tin, tout, freq, BETA, True, coef, h_w, rg, h_bins[n_bin], n_bin, 1)
    assert_fobs(got, want, "beside every other block")
    alone = fobs_call(f, leaf, B0, cuda, coef, mz, w=w, rg=rg, sets=SETS, bins=bins, n_bin=n_bin, bin_base=1)
    for key in ("fobs", "fcov"):
        assert_bits(alone[key].cpu().numpy(), got[key].cpu().numpy(), ("without the other blocks", key))


# ---- 4. chunks ------------------------------------------------------------------------------------------------------------------------------ #
def test_chunks_groups_poisoned_samples_repeats_and_shards(libfdg, cuda):
    """FDG_ROOT_SCRATCH_MB = 1 with 19 roots (root 7 does not exist): eleven chunks of 6 848 samples; M = 8: all 152 value columns;
    four weight groups; inf and nan weights and leaves on samples whose bin is out of range reach no sum; a second run gives the same
    bits; prefilled arrays grow by the same amounts; two shards add up to the whole."""
    import torch
    rng = np.random.default_rng(5)
    t = random_table(rng)
    R, B, n_bin, missing, M = t.n_root, 70_003, 3, 7, 8
    freq = (0, 2, -1, -7, 11)
    exists = np.arange(R) != missing
    rg = [k % 4 for k in range(R)]
    sets = [(0, 1), (1, 2, 3), (0, 4), (2, 5)]
    f = fd.compile_table(t, specialize="isa", options={"FDG_ROOT_SCRATCH_MB": "1"})
    h_leaf = oracle.philox_uniform(B, t.n_leaf, 17) + 0.25
    h_bins = make_bins(rng, B, n_bin, base=0)
    h_w = rng.uniform(0.1, 2.0, size=(4, B))
    h_T = rng.uniform(0.0, BETA, size=(B, 5))
    pairs = [(1, 2), (3, 5), (4, 4)]
    tin, tout = [pairs[k % 3][0] for k in range(R)], [pairs[k % 3][1] for k in range(R)]
    out_of_range = np.flatnonzero((h_bins < 0) | (h_bins >= n_bin))
    assert out_of_range.size > 500
    h_leaf[out_of_range[0::3], 0], h_leaf[out_of_range[1::3], 1] = np.inf, np.nan
    h_w[1, out_of_range[2::3]], h_w[2, out_of_range[0::2]] = np.nan, np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        roots = oracle.eval_static(t, h_leaf)
    coef = random_coef(rng, M, R, zero_row=5)
    leaf, w, bins, d_T = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins).to(cuda), torch.from_numpy(h_T).to(cuda)
    tables = {p: phase_table(h_T[:, p[1] - 1] - h_T[:, p[0] - 1], BETA, freq, True) for p in pairs}
    with np.errstate(invalid="ignore", over="ignore"):
        want = capi.freq_observables_reference(roots, h_T, tin, tout, freq, BETA, True, coef, h_w, rg, h_bins, n_bin, 0, exists, phases=tables)
    live = [p for p in range(2 * M) if p % M != 5]
    assert np.isnan(want[0][:, :, [5, M + 5]]).all() and np.isfinite(want[0][:, :, live]).all()
    args = dict(w=w, rg=rg, sets=sets, bins=bins, n_bin=n_bin)
    mz = (d_T, freq, True, tin, tout)
    got = fobs_call(f, leaf, B, cuda, coef, mz, fill=SENTINEL, **args)
    assert np.isfinite(got["fobs"].cpu().numpy()).all() and np.isfinite(got["fcov"].cpu().numpy()).all()
    assert_fobs(got, want, "19 roots, 4 groups, 11 chunks", fill=SENTINEL)
    again = fobs_call(f, leaf, B, cuda, coef, mz, fill=SENTINEL, **args)
    for key in ("fobs", "fcov"):
        assert_bits(again[key].cpu().numpy(), got[key].cpu().numpy(), ("the same arguments, the same bits", key))
    # prefilled arrays grow by the same amounts: from 0 and from the sentinel the increments agree within the rounding of one addition
    zero = fobs_call(f, leaf, B, cuda, coef, mz, **args)
    for key, i in (("fobs", 2), ("fcov", 3)):
        g0, g1 = zero[key].cpu().numpy(), got[key].cpu().numpy()
        dead = np.isnan(want[i - 2])
        assert (g0[dead] == 0.0).all()
        grow = np.abs((g1[~dead] - SENTINEL) - g0[~dead])
        assert (grow <= 4.0 * np.finfo(float).eps * (np.abs(g0[~dead]) + abs(SENTINEL))).all(), key
    assert_fobs(zero, want, "from zero")
    # two shards added together (the cut on a chunk boundary of neither)
    cut = 64 * 517
    o = fobs_call(f, leaf, cut, cuda, coef, mz, fill=SENTINEL, **args)
    fobs_call(f, leaves(cuda, h_leaf[cut:], "tiled"), B - cut, cuda, coef, (d_T[cut:], freq, True, tin, tout), w=w[:, cut:], rg=rg, sets=sets,
              bins=bins[cut:], n_bin=n_bin, out=o)
    assert_fobs(o, want, "two shards", fill=SENTINEL)


def test_column_slices_and_the_largest_histogram(libfdg, cuda):
    """The shapes at which the plan takes its other paths.  3 000 bins x 5 frequencies with M = 8: one frequency per slice and the 152
    columns in slices of two, and the partial slab no longer holds the binned call's segment count.  16 384 bins, one frequency, M = 1:
    one column per slice, the histogram of FDG_BIN_MAX rows beside two stash rows (the largest LDS request)."""
    import torch
    t, h_leaf, roots, h_T, h_w, _, tin, tout = batch(NAME)
    f = fd.compile_table(t, specialize="isa")
    rng = np.random.default_rng(33)
    leaf, d_T, w = leaves(cuda, h_leaf, "tiled"), torch.from_numpy(h_T).to(cuda), torch.from_numpy(h_w).to(cuda)
    for n_bin, freq, M in ((3_000, (0, 2, -1, -7, 11), 8), (capi.FDG_BIN_MAX, (3,), 1)):
        h_bins = make_bins(rng, B0, n_bin, base=0)
        coef = random_coef(rng, M, t.n_root, None if M == 1 else 2)
        want = capi.freq_observables_reference(roots, h_T, tin, tout, freq, BETA, True, coef, h_w, None, h_bins, n_bin, 0)
        got = fobs_call(f, leaf, B0, cuda, coef, (d_T, freq, True, tin, tout), w=w, bins=torch.from_numpy(h_bins).to(cuda), n_bin=n_bin,
                        fill=SENTINEL)
        assert_fobs(got, want, (n_bin, len(freq), M), fill=SENTINEL)


# ---- 5. the Monte-Carlo routes ------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("route", ["split", "fused", None])
def test_mc_routes(libfdg, cuda, fdgopt, route):
    """fdg_mc_accumulate_device_freq_observables on every route, T component-major and sample-major (the descriptor's d_T NULL: the
    call's own T), against the same handle's mc_eval_device roots pushed through the reference."""
    import torch
    z = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    R, B, dim, n_loop, n_tau = t.n_root, B0, 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam, n_bin, freq, M = 1.919, BETA, 1.2, 5, (0, -1, 3), 3
    rng = np.random.default_rng(13)
    h_K, h_T = rng.uniform(-2.0, 2.0, size=(B, n_loop * dim)), rng.uniform(0.0, beta, size=(B, n_tau))
    tin, tout = [1] * R, [1 + k % n_tau for k in range(R)]
    st = torch.cuda.current_stream().cuda_stream
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    if route:
        fdgopt.set("FDG_MC_ROUTE", route)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    h_w, h_bins = rng.uniform(0.0, 1.0, size=B), make_bins(rng, B, n_bin, base=1)
    w, bins = torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins).to(cuda)
    exists = np.array([int(t.root_slot[k]) != 0xFFFFFFFF for k in range(R)])
    coef = random_coef(rng, M, R)
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
            torch.cuda.synchronize()
            want = capi.freq_observables_reference(root.cpu().numpy(), h_T, tin, tout, freq, beta, True, coef, h_w, None, h_bins, n_bin, 1, exists)
        o = torch.zeros((n_bin, len(freq), 2 * M), dtype=torch.float64, device=cuda)
        c = torch.zeros((n_bin, len(freq), 2 * M, 2 * M), dtype=torch.float64, device=cuda)
        desc, _k = capi.make_matsubara(freq, True, tin, tout, beta, n_tau, 0, 0, 0, 0)
        fo, _k2 = capi.make_freq_observables(coef, o.data_ptr(), c.data_ptr())
        f.handle.mc_accumulate_device_freq_observables(dK.data_ptr(), ks, kc, dT.data_ptr(), ts, tc, kF, beta, lam, bins.data_ptr(), 1, n_bin,
                                                       w.data_ptr(), fo, desc, B=B, stream=st)
        torch.cuda.synchronize()
        assert_fobs((o.cpu().numpy(), c.cpu().numpy()), want, (route, major))


# ---- 6. known answers through the driver ------------------------------------------------------------------------------------------------ #
def test_two_propagators_known_answer(libfdg, cuda):
    """Two roots, each one fermionic order-0 propagator from T[1] = 0 to T[2] = tau with its own loop momentum fixed at k = 1.5 and
    0.5: root i integrates to 1 / (eps_i - i omega_n), eps_i = k_i^2 - kF^2.  The rows (1, 1), (1, -1) and (1, 0) are the sum, the
    difference and root 0 alone.  2 iterations of 2^18 samples: the sizing of tests/test_matsubara_accumulate.py's known answer."""
    a, b = fd.Graph([]), fd.Graph([])
    t, _, _ = lower([fd.Graph([a], subgraph_factors=[1.0]), fd.Graph([b], subgraph_factors=[1.0])])
    assert t.n_leaf == 2 and t.n_root == 2
    assert list(oracle.eval_static(t, np.array([[2.0, 3.0]]))[0]) == [2.0, 3.0]      # root i reads leaf i
    kF, beta, N = 1.0, BETA, 1 << 18
    i32 = lambda *v: np.array(v, np.int32)
    tab, _keep = capi.make_leaf_tables(i32(1, 1), i32(0, 0), i32(1, 1), i32(2, 2), i32(1, 2), np.eye(2), 3, 2)
    mz = vegas.MatsubaraProjection(freq=(0, 1, -3), fermionic=True, root_tau_in=(1, 1), root_tau_out=(2, 2))
    fo = vegas.FrequencyObservables(((1.0, 1.0), (1.0, -1.0), (1.0, 0.0)))
    ks = (1.5, 0.5)
    f = fd.compile_table(t, specialize="isa")
    res = vegas.vegas_integrate(f, tab, [0.0], [beta], [7], kF, beta, 0.0, n_iter=2, n_sample=N, n_grid=32, seed=2_025,
                                fixed=[ks[0], 0.0, 0.0, ks[1], 0.0, 0.0, 0.0, 0.0], device=cuda, matsubara=mz, freq_observables=fo)
    assert res.mean.shape == (3, 2) and res.fobs_mean.shape == res.fobs_stderr.shape == res.fobs_chi2_dof.shape == (3, 3)
    assert np.iscomplexobj(res.fobs_mean) and np.iscomplexobj(res.fobs_stderr) and res.fobs_cov.shape == (3, 6, 6)
    assert len(res.fobs_iterations) == 2 and res.fobs_iterations[0][0].shape == (3, 6) and res.fobs_iterations[0][1].shape == (3, 6, 6)
    for i, n in enumerate(mz.freq):
        g = [1.0 / (k * k - kF * kF - 1j * (2 * n + 1) * np.pi / beta) for k in ks]
        for m, exact in enumerate((g[0] + g[1], g[0] - g[1], g[0])):
            got, err = res.fobs_mean[i, m], res.fobs_stderr[i, m]
            print(f"n {n:+d} row {m}: {got:.6f} +- ({err.real:.2e}, {err.imag:.2e}); exact {exact:.6f}; "
                  f"off by ({abs(got.real - exact.real) / err.real:.2f}, {abs(got.imag - exact.imag) / err.imag:.2f}) sigma")
            assert err.real > 0 and err.imag > 0
            assert abs(got.real - exact.real) < 5.0 * err.real and abs(got.imag - exact.imag) < 5.0 * err.imag, (n, m, got, err, exact)
    # the row (1, 0) is root 0 of the per-root projection
    for part in (np.real, np.imag):
        assert np.allclose(part(res.fobs_mean[:, 2]), part(res.mean[:, 0]), rtol=1e-12, atol=0.0)
        assert np.allclose(part(res.fobs_stderr[:, 2]), part(res.stderr[:, 0]), rtol=1e-12, atol=0.0)
    assert np.array_equal(res.fobs_cov, res.fobs_cov.transpose(0, 2, 1))
    assert np.allclose(np.einsum("fpp->fp", res.fobs_cov), np.concatenate([res.fobs_stderr.real, res.fobs_stderr.imag], axis=1) ** 2, rtol=1e-12)
    # without the keyword the results are what they are today
    ref = vegas.vegas_integrate(f, tab, [0.0], [beta], [7], kF, beta, 0.0, n_iter=2, n_sample=N, n_grid=32, seed=2_025,
                                fixed=[ks[0], 0.0, 0.0, ks[1], 0.0, 0.0, 0.0, 0.0], device=cuda, matsubara=mz)
    assert ref.fobs_mean is None and ref.fobs_cov is None and ref.fobs_iterations == []
    assert_bits(ref.mean.real, res.mean.real, "mean beside the frequency observables")
    assert_bits(ref.mean.imag, res.mean.imag, "mean beside the frequency observables")
    assert_bits(ref.stderr.real, res.stderr.real, "stderr beside the frequency observables")
    assert_bits(ref.stderr.imag, res.stderr.imag, "stderr beside the frequency observables")


def test_sum_and_difference_of_equal_roots_known_answer(libfdg, cuda):
    """twin_roots(): the same root twice.  At every frequency the difference is exactly 0 with an error of exactly 0, and the error of
    the sum is twice the per-root error -- quadrature of the per-root errors would say sqrt(2) sigma for both."""
    L, lam, G, B, n_iter = 2.0, 0.05, 32, 50_000, 3
    t, tab, _keep = twin_roots()
    f = fd.compile_table(t, specialize="isa")
    mz = vegas.MatsubaraProjection(freq=(0, 2, -1), fermionic=True, root_tau_in=(1, 1), root_tau_out=(1, 1))
    res = vegas.vegas_integrate(f, tab, [-L] * 3, [L] * 3, [0, 1, 2], 0.0, 1.0, lam, n_iter=n_iter, n_sample=B, n_grid=G, seed=2025, device=cuda,
                                matsubara=mz, freq_observables=vegas.FrequencyObservables(((1.0, 1.0), (1.0, -1.0))))
    print("twin roots:", res.mean, res.stderr, "frequency observables:", res.fobs_mean, res.fobs_stderr)
    assert res.fobs_mean.shape == (3, 2) and res.fobs_cov.shape == (3, 4, 4) and len(res.fobs_iterations) == n_iter
    assert (res.stderr[:, 0].real > 0).all() and np.array_equal(res.stderr[:, 0], res.stderr[:, 1])
    assert (res.fobs_mean[:, 1] == 0.0).all() and (res.fobs_stderr[:, 1] == 0.0).all()
    for part in (np.real, np.imag):
        assert np.allclose(part(res.fobs_stderr[:, 0]), 2.0 * part(res.stderr[:, 0]), rtol=1e-12, atol=0.0)
        assert np.allclose(part(res.fobs_mean[:, 0]), 2.0 * part(res.mean[:, 0]), rtol=1e-12, atol=0.0)
    exact = 64.0 * math.pi * L ** 3 * (lam + L * L)                            # (the two times of a root coincide: the phase is 1)
    assert (np.abs(res.fobs_mean[:, 0].real - 2.0 * exact) < 5.0 * res.fobs_stderr[:, 0].real).all()
