"""The Markov chain with a discrete external variable and per-bin measurement on the device (include/fdg.h:
fdg_chain_propose_device_discrete, fdg_chain_step_device_binned, fdg_mc_chain_step_device_binned; feynmandiagram.jl_amd/vegas.py:
chain_integrate_binned).  With one value the step is tied bit for bit to the plain, the projected and the grouped step; the proposal
is tied bit for bit to the direct sampler (fdg_vegas_sample_device_discrete); every step is compared bit for bit with the numpy
mirror (capi.chain_binned_reference): x, fac, bin, root, a, sum, n_accept.  In the leaf form the mirror's roots are the CPU oracle's,
in the Monte-Carlo form fdg_mc_eval_device's on the mirror's own proposals, as in tests/test_chain_matsubara_accumulate.py.  The
statistical conditions of the leaf-form known answer are the ones the mirror alone meets in tests/test_chain_binned_host.py."""
import math

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from test_chain_accumulate import PAD, SENT, DeviceChain, assert_reduced
from test_chain_binned_host import (CDF3, ECOL3, EXT3, KNOWN_B, cdf_of, fresh_binned_state, known_b_graph, known_b_mirror, mirror_binned_step)
from test_chain_groups_accumulate import RHO3, DeviceChainGrp, poison_case
from test_chain_groups_host import GROUPS3
from test_chain_host import FAKE, INIT, MEASURE, failed, oracle_roots
from test_chain_matsubara_accumulate import DeviceChainMz, device_mc_roots, leaf_case, mc_cases  # noqa: F401 (mc_cases: a fixture)
from test_strat_accumulate import assert_bits
from test_vegas_discrete_accumulate import leaf_on_k1_plus_k2, refined_cdf, refined_grid

pytestmark = pytest.mark.gpu

STATE = ("x", "fac", "bin", "root", "a", "sum", "n_accept")


class DeviceChainBin(DeviceChain):
    """DeviceChain with the discrete variable: fac / facp [D + 1, B], bin / binp int32 [B], sum [n_bin (R or 2 F R) + 1, B]; bit D of a
    step's mask moves the discrete variable.  ``groups`` a dict of root_group and var_sets or None (a NULL cg), ``mz`` as DeviceChainMz's
    or None."""

    def __init__(self, handle, cuda, grid, col, fixed, B, cdf, ext=None, ext_col=(), groups=None, reweight=None, mz=None, coef=None,
                 shard_start=0):
        import torch
        super().__init__(handle, cuda, grid, col, fixed, B, coef, shard_start)
        D, R = self.D, self.R
        self.n_bin, self.ext_col = len(cdf) - 1, [int(e) for e in ext_col]
        self.d_cdf = torch.from_numpy(np.ascontiguousarray(cdf, dtype=np.float64)).to(cuda)
        self.d_ext = None if ext is None else torch.from_numpy(np.ascontiguousarray(ext, dtype=np.float64)).to(cuda)
        self.n_sum = self.n_bin * (R if mz is None else 2 * len(mz[0]) * R) + 1
        f64 = dict(dtype=torch.float64, device=cuda)
        self.fac, self.facp = torch.full(((D + 1) * B + PAD,), SENT, **f64), torch.full(((D + 1) * B + PAD,), SENT, **f64)
        self.total = torch.full((self.n_sum * B + PAD,), SENT, **f64)
        self.bins, self.binp = (torch.full((B + PAD,), int(SENT), dtype=torch.int32, device=cuda) for _ in range(2))
        self.fac[:(D + 1) * B], self.total[:self.n_sum * B], self.bins[:B] = 1.0, 0.0, 0
        self.desc = self.groups = None
        if mz is not None:
            self.desc, self._keep = capi.make_chain_matsubara(*mz)
        if groups is not None:
            self.groups, self._gkeep = capi.make_chain_groups(groups["root_group"], groups["var_sets"], reweight)

    def propose(self, mask, seed, off):
        D = self.D
        capi.chain_propose_device_discrete(self.d_grid.data_ptr(), D, self.G, self.col, self.C, mask & ((1 << D) - 1), seed, off, self.x.data_ptr(),
                                           self.xc, self.fac.data_ptr(), self.xp.data_ptr(), self.xc, self.facp.data_ptr(), bool((mask >> D) & 1),
                                           self.d_cdf.data_ptr(), self.n_bin, 0 if self.d_ext is None else self.d_ext.data_ptr(), self.ext_col,
                                           self.bins.data_ptr(), self.binp.data_ptr(), self.B, self.st)

    def select(self, gamma, seed, off, flags, mc=None):
        tail = (self.facp.data_ptr(), self.C, self.D, self.coef, gamma, seed, off, flags, self.x.data_ptr(), self.xc, self.fac.data_ptr(),
                self.root.data_ptr(), self.a.data_ptr(), self.total.data_ptr(), self.n_acc.data_ptr(), self.desc, self.groups, self.n_bin,
                self.binp.data_ptr(), self.bins.data_ptr(), self.B, self.st)
        if mc is None:
            self.h.chain_step_device_binned(self.xp.data_ptr(), self.xc, *tail)
        else:
            self.h.mc_chain_step_device_binned(self.xp.data_ptr(), self.xc, *mc, *tail)

    reduced = DeviceChainMz.reduced

    def state(self):
        """DeviceChain.state with the row D of fac, the bins and the larger sum"""
        import torch
        torch.cuda.synchronize()
        B, D, R = self.B, self.D, self.R
        x, xp = self.x.cpu().numpy(), self.xp.cpu().numpy()
        assert (x[:, B:] == SENT).all() and (xp[:, B:] == SENT).all(), "a lane past n_walker of x or xp was written"
        out = {"x": x[:, :B].copy(), "xp": xp[:, :B].copy()}
        for name, t, n in (("fac", self.fac, (D + 1) * B), ("facp", self.facp, (D + 1) * B), ("root", self.root, R * B), ("a", self.a, B),
                           ("sum", self.total, self.n_sum * B), ("n_accept", self.n_acc, B), ("bin", self.bins, B), ("binp", self.binp, B)):
            h = t.cpu().numpy()
            assert (h[n:] == (SENT if h.dtype == np.float64 else int(SENT))).all(), name + ": a word past the array was written"
            out[name] = h[:n].reshape(-1, B).copy() if name not in ("a", "n_accept", "bin", "binp") else h[:n].copy()
        return out


def assert_binned_state(got, want, what):
    for k in STATE:
        assert_bits(got[k], want[k], f"{what}: {k}")


def binned_steps(D, B, gamma):
    """INIT, two unmeasured and six measured steps: everything, the discrete variable alone, one continuous variable alone, a pair with
    the discrete one, nothing"""
    full, disc = (1 << (D + 1)) - 1, 1 << D
    moves = [(full, INIT), (full, 0), (disc, 0), (full, MEASURE), (disc, MEASURE), (1 << (D // 2), MEASURE), (disc | 1, MEASURE), (0, MEASURE),
             (full, MEASURE)]
    return [(mask, i * B + 17, 1.0 if flags == INIT else gamma, flags) for i, (mask, flags) in enumerate(moves)]


def mz_dict(mz):
    return None if mz is None else dict(freq=mz[0], fermionic=mz[1], weight_freq=mz[2], root_col_in=mz[3], root_col_out=mz[4], beta=mz[5])


def run_against_mirror(chain, m, grid, col, steps, seed, ev, cdf, ext, ext_col, groups, reweight, mz, coef, exists, what, mc=None, lo=0):
    for i, (mask, off, g, flags) in enumerate(steps):
        chain.step(mask, g, seed, off + lo, flags, mc)
        m = mirror_binned_step(m, grid, col, mask, seed, off + lo, g, flags, ev, cdf, ext, ext_col, groups, reweight, mz_dict(mz), coef, exists)
        got = chain.state()
        assert_bits(got["xp"], m["xp"], f"{what}, step {i}: xp")
        assert_bits(got["facp"], m["facp"], f"{what}, step {i}: facp")
        assert_bits(got["binp"], m["binp"], f"{what}, step {i}: binp")
        assert_binned_state(got, m, f"{what}, step {i}")
    return m


# ---- 1. the tie to the entries that exist -------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("entry", ["plain", "matsubara", "grouped"])
def test_one_value_ties_the_step_to_the_existing_entries(libfdg, cuda, entry):
    """n_bin = 1, cdf = {0, 1}, n_ext = 0: fd = 1.0 and jac * 1.0 keeps its bits.  Over INIT and three steps x, fac rows 0 .. n_dim - 1,
    root, a, sum and n_accept are bit for bit those of fdg_chain_step_device, of .._matsubara (3 frequencies) and of .._grouped
    (3 groups, rho), whether the discrete variable is redrawn or copied."""
    t, f, col, fixed, grid, coef, exists, cin, cout = leaf_case(cuda)
    B, D, seed, gamma = 1_229, len(col), 9, 0.37
    mz = ((2, -1, 0), True, 1, cin, cout, 1.7)
    one = np.array([0.0, 1.0])
    args = (f.handle, cuda, grid, col, fixed, B)
    for move in (0, 1):
        if entry == "plain":
            old, new = DeviceChain(*args, coef), DeviceChainBin(*args, one, coef=coef)
        elif entry == "matsubara":
            old, new = DeviceChainMz(*args, mz, coef), DeviceChainBin(*args, one, mz=mz, coef=coef)
        else:
            old = DeviceChainGrp(*args, GROUPS3["root_group"], GROUPS3["var_sets"], RHO3, None, coef)
            new = DeviceChainBin(*args, one, groups=GROUPS3, reweight=RHO3, coef=coef)
        full = (1 << D) - 1
        for i, (mask, flags) in enumerate([(full, INIT), (full, MEASURE), (0b010, MEASURE), (full, MEASURE)]):
            off, g = i * B + 17, 1.0 if flags == INIT else gamma
            old.step(mask, g, seed, off, flags)
            new.step(mask | (move << D), g, seed, off, flags)
            a, b = old.state(), new.state()
            for k in ("x", "root", "a", "sum", "n_accept"):
                assert_bits(b[k], a[k], f"move_discrete {move}, step {i}: {k}")
            assert_bits(b["fac"][:D], a["fac"], f"move_discrete {move}, step {i}: fac")
            assert (b["fac"][D] == 1.0).all() and (b["bin"] == 0).all()
        assert 0 < (a["n_accept"] < 4).sum() and np.abs(a["sum"][:-1]).max() > 0.0


# ---- 2. the tie to the direct sampler ------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("n_bin", [1, 2, 7, 64])
@pytest.mark.parametrize("D", [1, 5, 63])
def test_a_full_proposal_is_the_direct_samplers_draw(libfdg, cuda, D, n_bin):
    """Every variable and the discrete one redrawn: xp, the ext_col columns included, is fdg_vegas_sample_device_discrete's x and binp
    its d_bin (bin_base 0) for the same seed and offset, bit for bit.  A refined grid and a refined cdf; col and ext_col a permutation
    that leaves three columns unnamed, which the proposal copies from x."""
    import torch
    rng = np.random.default_rng(1_000 * D + n_bin)
    B, G, seed, off, n_ext = 1_229, 6, 0x1234_5678_9ABC, 3_000_000_011, 4
    C = D + n_ext + 3
    grid, cdf = refined_grid(rng, D, G), refined_cdf(rng, n_bin)
    perm = rng.permutation(C)
    col, ext_col = [int(c) for c in perm[:D]], [int(c) for c in perm[D:D + n_ext]]
    ext = rng.uniform(-5.0, 5.0, size=(n_bin, n_ext))
    st = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=cuda)
    d_grid, d_cdf, d_ext = (torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for v in (grid, cdf, ext))
    x = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(C, B))).to(cuda)
    fac, facp, xp = torch.ones((D + 1, B), **f64), torch.zeros((D + 1, B), **f64), torch.full((C, B), -77.0, **f64)
    bins, binp = torch.zeros(B, dtype=torch.int32, device=cuda), torch.full((B,), -5, dtype=torch.int32, device=cuda)
    capi.chain_propose_device_discrete(d_grid.data_ptr(), D, G, col, C, (1 << D) - 1, seed, off, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B,
                                       facp.data_ptr(), True, d_cdf.data_ptr(), n_bin, d_ext.data_ptr(), ext_col, bins.data_ptr(), binp.data_ptr(),
                                       B, st)
    sx, jac = torch.full((C, B), -77.0, **f64), torch.zeros(B, **f64)
    sb = torch.full((B,), -5, dtype=torch.int32, device=cuda)
    capi.vegas_sample_device_discrete(d_grid.data_ptr(), D, G, col, d_cdf.data_ptr(), n_bin, 0, d_ext.data_ptr(), ext_col, seed, off, sx.data_ptr(),
                                      1, B, jac.data_ptr(), sb.data_ptr(), 0, B, st)
    torch.cuda.synchronize()
    named = col + ext_col
    rest = [c for c in range(C) if c not in named]
    hxp, hsx, hb = xp.cpu().numpy(), sx.cpu().numpy(), binp.cpu().numpy()
    assert_bits(hxp[named], hsx[named], "xp")
    assert np.array_equal(hb, sb.cpu().numpy()) and hb.min() >= 0 and hb.max() < n_bin and (n_bin == 1 or len(set(hb)) > 1)
    assert_bits(hxp[ext_col], ext[hb].T, "the table's rows")
    assert len(rest) == 3 and np.array_equal(hxp[rest], x.cpu().numpy()[rest]) and (hsx[rest] == -77.0).all()
    p = cdf[hb + 1] - cdf[hb]
    hf = facp.cpu().numpy()
    assert_bits(hf[D], 1.0 / p, "facp[n_dim]")
    j = hf[0].copy()
    for d in range(1, D):
        j = j * hf[d]
    assert_bits(j / p, jac.cpu().numpy(), "the sampler's weight from the proposal's factors")


# ---- 3. bit for bit against the mirror ----------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n_bin", [2, 7])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_every_step_matches_the_mirror_bit_for_bit(libfdg, cuda, B, n_bin):
    """The random graph of tests/test_chain_accumulate.py (ten roots, one of which does not exist; three variables) in three groups:
    group 1 holds only the root that does not exist, variable 1 belongs to no group with a root, group 2 has an empty mask.  reweight
    and coef given and NULL, plain and with 3 frequencies, a NULL cg once; after INIT and after every step."""
    t, f, col, fixed, grid, coef, exists, cin, cout = leaf_case(cuda)
    D, R, seed, gamma = len(col), t.n_root, 11, 0.37
    rng = np.random.default_rng(n_bin)
    cdf, ext = refined_cdf(rng, n_bin), rng.uniform(-1.0, 1.0, size=(n_bin, 2))
    ev = oracle_roots(t)
    refused = 0
    cases = [(GROUPS3, rho, cf, mz) for mz in (None, ((2, -1, 0), True, 1, cin, cout, 1.7)) for rho in (None, RHO3) for cf in (None, coef)]
    for groups, rho, cf, mz in cases + [(None, None, coef, None)]:
        chain = DeviceChainBin(f.handle, cuda, grid, col, fixed, B, cdf, ext, ECOL3, groups, rho, mz, cf)
        m = fresh_binned_state(fixed, D, R, B, n_bin, 3 if mz else 0)
        m = run_against_mirror(chain, m, grid, col, binned_steps(D, B, gamma), seed, ev, cdf, ext, ECOL3, groups, rho, mz, cf, exists,
                               f"groups {groups is not None}, rho {rho is not None}, coef {cf is not None}, mz {mz is not None}")
        refused += int((m["n_accept"] < 9).sum())
        assert (m["sum"][-1] > 0.0).all()
        assert_reduced(chain.reduced(), m["sum"], "reduced sums")
    assert B < 63 or refused > 0                             # some proposals were refused


def test_walkers_over_several_chunks_and_from_two_shards(libfdg, cuda):
    """70 003 walkers with FDG_ROOT_SCRATCH_MB = 1 (chunks of 13 056 walkers, the last one of 4 723) against the mirror after every
    step; the same bits with the default scratch (one chunk), and from two shards; the projected step across the same three runs."""
    B, seed, gamma, n_bin = 70_003, 12, 0.37, 3
    t, f1, col, fixed, grid, coef, exists, cin, cout = leaf_case(cuda, options={"FDG_ROOT_SCRATCH_MB": "1"})
    f = fd.compile_table(t, specialize="isa")
    D, R = len(col), t.n_root
    rng = np.random.default_rng(n_bin)
    cdf, ext = refined_cdf(rng, n_bin), rng.uniform(-1.0, 1.0, size=(n_bin, 2))
    ev = oracle_roots(t)
    steps = binned_steps(D, B, gamma)
    for mz in (None, ((0, -2, 1), True, 2, cin, cout, 1.7)):
        def run(handle, n, lo, check):
            chain = DeviceChainBin(handle, cuda, grid, col, fixed, n, cdf, ext, ECOL3, GROUPS3, RHO3, mz, coef, lo)
            if check:
                run_against_mirror(chain, fresh_binned_state(fixed, D, R, n, n_bin), grid, col, steps, seed, ev, cdf, ext, ECOL3, GROUPS3, RHO3,
                                   mz, coef, exists, "chunks")
            else:
                for mask, off, g, flags in steps:
                    chain.step(mask, g, seed, off + lo, flags)
            return chain.state(), chain.reduced()
        small, small_red = run(f1.handle, B, 0, mz is None)
        whole, whole_red = run(f.handle, B, 0, False)
        assert_binned_state(whole, small, "FDG_ROOT_SCRATCH_MB changed")
        assert_bits(whole_red, small_red, "reduced sums, FDG_ROOT_SCRATCH_MB changed")
        assert 0 < (small["n_accept"] < 9).sum() and np.abs(small["sum"]).max() > 0.0 and set(small["bin"]) == set(range(n_bin))
        cut = 30_001
        for lo, n in ((0, cut), (cut, B - cut)):
            part, _ = run(f1.handle, n, lo, False)
            for k in STATE:
                assert_bits(part[k], small[k][..., lo:lo + n], f"shard at {lo}: {k}")


def test_monte_carlo_form_matches_the_mirror(mc_cases, cuda):
    """parquet_sigma2 in the Monte-Carlo form with its external momentum from the table (7 values), its two roots in two groups (root 0:
    the momenta only; root 1: everything), with factors and with a projection; the mirror's roots are fdg_mc_eval_device's"""
    c = mc_cases["parquet_sigma2"]
    t, h, col, grid, fixed = c["t"], c["f"].handle, c["col"], c["grid"], c["fixed"]
    B, D, R, seed, n_bin = 1_229, len(col), t.n_root, 21, 7
    kF, beta, lam, nk = c["phys"]
    n_mom = sum(1 for v in col if v < nk)
    groups = dict(root_group=[0, 1], var_sets=[tuple(range(n_mom)), tuple(range(D))])
    rng = np.random.default_rng(3)
    cdf, ext = refined_cdf(rng, n_bin), rng.uniform(-kF, kF, size=(n_bin, 3))
    ev = device_mc_roots(h, cuda, c["phys"], R)
    for mz, rho in ((None, (2.5, 0.4)), (((0, -1, 2), True, 2, c["cin"], c["cout"], beta), None)):
        chain = DeviceChainBin(h, cuda, grid, col, fixed, B, cdf, ext, [0, 1, 2], groups, rho, mz)
        m, gamma = fresh_binned_state(fixed, D, R, B, n_bin, 3 if mz else 0), None
        for i, (mask, off, g, flags) in enumerate(binned_steps(D, B, 1.0)):
            if flags != INIT:
                g = gamma
            chain.step(mask, g, seed, off, flags, mc=(kF, beta, lam))
            m = mirror_binned_step(m, grid, col, mask, seed, off, g, flags, ev, cdf, ext, [0, 1, 2], groups, rho, mz_dict(mz), None, None)
            assert_binned_state(chain.state(), m, f"step {i}")
            if flags == INIT:
                gamma = float(m["a"].mean())
                assert gamma > 0.0
        assert 0 < (m["n_accept"] < 9).sum() and np.abs(m["sum"][:-1]).max() > 0.0 and set(m["bin"]) == set(range(n_bin))


@pytest.fixture(scope="module")
def ver4(libfdg):
    """parquet_ver4_4 and its compiled function: built once, shared, never written to"""
    t = workloads.get("parquet_ver4_4")
    return t, fd.compile_table(t, specialize="isa")


@pytest.mark.parametrize("n_freq", [0, 4])
def test_180_roots_63_variables_8_groups_and_64_bins(ver4, cuda, n_freq):
    """parquet_ver4_4 in the leaf form with 63 of its leaves as variables and two more written from the table of 64 values, 8 groups
    with nested masks and the roots spread over them, with factors; 65 walkers, INIT and 3 steps, plain and with 4 frequencies."""
    t, f = ver4
    B, D, G, seed, beta, n_bin = 65, capi.FDG_VEGAS_DIM_MAX - 1, 3, 9, 1.0, capi.FDG_CHAIN_BIN_MAX
    NG = capi.FDG_WEIGHT_GROUP_MAX
    assert t.n_root == 180 and t.n_leaf >= D + 2
    rng = np.random.default_rng(6)
    perm = [int(c) for c in rng.permutation(t.n_leaf)]
    col, ext_col = perm[:D], perm[D:D + 2]
    fixed = rng.uniform(0.2, 1.0, size=t.n_leaf)
    grid = capi.vegas_refine(vegas.uniform_grid([0.2] * D, [1.0] * D, G), rng.random((D, G)) + 0.5, 1.0)
    cdf, ext = refined_cdf(rng, n_bin), rng.uniform(0.2, 1.0, size=(n_bin, 2))
    coef = rng.uniform(-1.0, 1.0, size=t.n_root)
    groups = dict(root_group=[k % NG for k in range(t.n_root)], var_sets=[tuple(range(min(8 * g + 8, D))) for g in range(NG)])
    rho = tuple(rng.uniform(0.5, 2.0, size=NG))
    tin, tout = workloads.root_times("parquet_ver4_4")
    mz = ((0, 1, -3, 7), True, 3, [int(i) - 1 for i in tin], [int(i) - 1 for i in tout], beta) if n_freq else None
    ev = oracle_roots(t)
    full = (1 << (D + 1)) - 1
    fresh = lambda: fresh_binned_state(fixed, D, t.n_root, B, n_bin, n_freq)      # noqa: E731
    m = mirror_binned_step(fresh(), grid, col, full, seed, 1 << 32, 1.0, INIT, ev, cdf, ext, ext_col, groups, rho, mz_dict(mz), coef, None)
    gamma = float(m["a"].mean())
    assert gamma > 0.0
    steps = [(full, (1 << 32) + i * B, 1.0 if i == 0 else gamma, flags) for i, flags in enumerate([INIT, MEASURE, MEASURE, MEASURE])]
    steps[2] = ((1 << D) | (1 << (D - 1)) | 1,) + steps[2][1:]
    chain = DeviceChainBin(f.handle, cuda, grid, col, fixed, B, cdf, ext, ext_col, groups, rho, mz, coef)
    m = run_against_mirror(chain, fresh(), grid, col, steps, seed, ev, cdf, ext, ext_col, groups, rho, mz, coef, None, "largest")
    assert 0 < (m["n_accept"] < 4).sum() < B and np.abs(m["sum"][:-1]).max() > 0.0 and len(set(m["bin"])) > 8


# ---- 4. poison ----------------------------------------------------------------------------------------------------------------------------- #
TINY = 1e-300
POISON = [
    # (what, grid of x, cdf, coef, reweight, projected): tests/test_chain_groups_accumulate.py's graph, r_0 = (2e154 x)^2 in group 0 with x only,
    # r_1 and r_2 in group 1 with y only
    ("a root is not finite", [0.0, 0.25, 0.5, 0.75, 1.0], (0.5, 0.25, 0.25), (1.0, 1.0, 1.0), None, False),           # r_0 = inf where x > 0.67
    ("jac_g s_g overflows", [0.0, 0.1, 0.2, 0.3, 1.0], (0.5, 0.25, 0.25), (1.0, 1.0, 1.0), (4.0, 1.0), False),         # fac_0 = 2.8 where x > 0.3, fd up to 4
    ("fd * jac overflows", [0.0, 0.25, 0.5, 0.75, 1.0], (TINY, 0.5, 0.5 - TINY), (1.0, 1.0, 1.0), None, False),        # fd = 1e300 in bin 0: r_0 > 1.8e8 overflows
    # projected: a term above 1.3e154 squares to inf, so the factors keep the terms of x < 0.18 below that where fd is 2
    ("fd * jac overflows, projected", [0.0, 0.25, 0.5, 0.75, 1.0], (TINY, 0.5, 0.5 - TINY), (1e-153, 1e-153, 1.0), (1.0, 1.0), True),
]


@pytest.mark.parametrize("what,gx,p,cf,rho,projected", POISON)
def test_poisoned_proposals_count_as_zero(libfdg, cuda, what, gx, p, cf, rho, projected):
    """A root that is not finite, an overflowing jac_g s_g and an overflowing fd * jac (a value with p = 1e-300, which half of the
    walkers are placed on: no uniform ever draws it) zero the whole proposal.  a stays finite, nothing that is not finite reaches the
    state or a sum, the columns of the root that does not exist are never written in any bin, a step changes no column of a bin
    other than the walker's own, and the mirror agrees bit for bit."""
    t, col = poison_case()
    f = fd.compile_table(t, specialize="isa")
    B, seed, gamma, R, D, n_bin = 300, 4, 0.5, 4, 2, 3
    grid = np.array([gx, [0.0, 0.25, 0.5, 0.75, 1.0]])
    cdf = np.array([0.0, p[0], p[0] + p[1], 1.0])
    coef = np.array(cf + (1.0,))
    groups = dict(root_group=[0, 1, 1, 5], var_sets=[(0,), (1,)])
    mz = ((0, -2), True, 1, [0, 1, 0, 9], [1, 0, 0, 9], 0.8) if projected else None
    F = 2 if projected else 0
    exists = [True, True, True, False]
    ev = oracle_roots(t)
    chain = DeviceChainBin(f.handle, cuda, grid, col, np.zeros(2), B, cdf, None, [], groups, rho, mz, coef)
    m = fresh_binned_state(np.zeros(2), D, R, B, n_bin, F)
    n_one = R if mz is None else 2 * F * R
    gone = [j * n_one + (3 if mz is None else 2 * (fr * R + 3) + q) for j in range(n_bin) for fr in range(max(F, 1)) for q in ((0, 1) if F else (0,))]
    chain.root[3 * B:4 * B] = 3.5
    m["root"][3] = 3.5
    for c in gone:
        chain.total[c * B:(c + 1) * B] = -9.75
        m["sum"][c] = -9.75
    # the placement keeps the discrete variable: every other walker sits on value 0 (p = cdf[1]), the rest on value 1
    import torch
    b0 = (np.arange(B) % 2 == 0)
    m["bin"] = np.where(b0, 0, 1).astype(np.int32)
    m["fac"][D] = 1.0 / np.where(b0, cdf[1] - cdf[0], cdf[2] - cdf[1])
    chain.bins[:B] = torch.from_numpy(m["bin"]).to(cuda)
    chain.fac[D * B:(D + 1) * B] = torch.from_numpy(m["fac"][D]).to(cuda)
    n_bad = n_overflow = 0
    prev = chain.state()["sum"]
    for i, (mask, flags) in enumerate([(3, INIT)] + [(mask, MEASURE) for mask in (3, 1, 2, 7, 0, 3, 4, 7)]):
        off = i * B
        chain.step(mask, gamma, seed, off, flags)
        got = chain.state()
        m = mirror_binned_step(m, grid, col, mask, seed, off, gamma, flags, ev, cdf, None, [], groups, rho, mz_dict(mz), coef, exists)
        rp = ev(m["xp"])[:3]
        bad = ~np.isfinite(rp).all(axis=0)
        zeroed = m["accept"] & (m["root"][:3] == 0.0).all(axis=0) & (m["a"] == 0.0)
        n_bad += int(bad.sum())
        n_overflow += int((zeroed & ~bad & (rp[2] != 0.0)).sum())        # every root finite, and the proposal counts as zero all the same
        assert zeroed[bad & m["accept"]].all()
        assert_binned_state(got, m, f"step {i}")
        assert all(np.isfinite(got[k]).all() for k in ("x", "fac", "root", "a", "sum"))
        assert (got["root"][3] == 3.5).all() and (got["sum"][gone] == -9.75).all()
        changed = (got["sum"][:-1] != prev[:-1]).reshape(n_bin, n_one, B).any(axis=1)                # [n_bin, B]: which bins a walker wrote
        assert not changed[np.arange(n_bin)[:, None] != got["bin"][None, :]].any(), f"step {i}: a column of another bin was written"
        prev = got["sum"]
    assert n_bad > 0 and n_overflow > 0 and 0 < (m["a"] == 0.0).sum() < B, (what, n_bad, n_overflow)
    assert len(set(m["bin"])) > 1


# ---- 5. argument errors, before any device work ---------------------------------------------------------------------------------------------- #
def _propose(n_dim=3, n_grid=8, col=None, n_col=7, mask=0b101, d_grid=FAKE[0], d_x=FAKE[1], xc=100, d_fac=FAKE[2], d_xp=FAKE[3], xpc=100,
             d_facp=FAKE[4], move=1, d_cdf=FAKE[5], n_bin=4, d_ext=FAKE[6], ext_col=(5, 6), d_bin=FAKE[7], d_binp=FAKE[7] + 0x10000, B=100):
    c = None if col is None else np.ascontiguousarray(col, dtype=np.uint32)
    ec = None if ext_col is None else np.ascontiguousarray(ext_col, dtype=np.uint32)
    return capi.lib().fdg_chain_propose_device_discrete(d_grid, n_dim, n_grid, None if c is None else c.ctypes.data, n_col, mask, 1, 0, d_x, xc,
                                                        d_fac, d_xp, xpc, d_facp, move, d_cdf, n_bin, d_ext, 0 if ec is None else len(ec),
                                                        None if ec is None or not len(ec) else ec.ctypes.data, d_bin, d_binp, B, None)


def test_propose_argument_checks(libfdg):
    for kw in (dict(d_grid=None), dict(d_x=None), dict(d_fac=None), dict(d_xp=None), dict(d_facp=None), dict(B=-1), dict(n_dim=0, mask=0),
               dict(n_grid=0), dict(d_xp=FAKE[1]), dict(d_facp=FAKE[2]), dict(mask=0b1000), dict(mask=1 << 63), dict(col=[0, 1, 7]),
               dict(n_col=2), dict(xc=99), dict(xpc=99),                                               # what fdg_chain_propose_device refuses
               dict(d_cdf=None), dict(d_bin=None), dict(d_binp=None), dict(d_binp=FAKE[7]), dict(n_bin=0), dict(d_ext=None),
               dict(ext_col=(5, 5)), dict(ext_col=(5, 2)), dict(ext_col=(5, 7)), dict(col=[0, 1, 5])):
        assert failed(_propose(**kw), capi.FDG_E_INVALID), kw
    assert failed(capi.lib().fdg_chain_propose_device_discrete(FAKE[0], 3, 8, None, 7, 5, 1, 0, FAKE[1], 100, FAKE[2], FAKE[3], 100, FAKE[4], 1, FAKE[5], 4,
                                                      FAKE[6], 2, None, FAKE[7], FAKE[7] + 0x10000, 100, None), capi.FDG_E_INVALID)   # no ext_col
    for kw in (dict(n_grid=capi.FDG_VEGAS_GRID_MAX + 1), dict(n_dim=capi.FDG_VEGAS_DIM_MAX + 1, n_col=100),
               dict(n_dim=capi.FDG_VEGAS_DIM_MAX, n_col=100, mask=0, ext_col=(70, 71)), dict(n_bin=capi.FDG_CHAIN_BIN_MAX + 1),
               dict(ext_col=tuple(range(10, 10 + capi.FDG_VEGAS_EXT_MAX + 1)), n_col=100)):
        assert failed(_propose(**kw), capi.FDG_E_UNSUPPORTED), kw
    assert _propose(B=0) == capi.FDG_OK and _propose(B=0, move=0, mask=0) == capi.FDG_OK
    assert _propose(B=0, ext_col=(), d_ext=None) == capi.FDG_OK and _propose(B=0, n_bin=capi.FDG_CHAIN_BIN_MAX) == capi.FDG_OK
    assert _propose(B=0, n_dim=capi.FDG_VEGAS_DIM_MAX - 1, n_col=100, mask=0, ext_col=(70,)) == capi.FDG_OK


def _step(h, mc=False, d_xp=FAKE[0], xpc=100, d_facp=FAKE[1], n_col=None, n_dim=3, coef=None, gamma=0.5, flags=MEASURE, d_x=FAKE[2], xc=100,
          d_fac=FAKE[3], d_root=FAKE[4], d_a=FAKE[5], d_sum=FAKE[6], d_n_accept=FAKE[7], mz=None, cg=None, n_bin=4, d_binp=FAKE[7] + 0x10000,
          d_bin=FAKE[7] + 0x20000, B=100):
    import ctypes as C
    if n_col is None:
        n_col = h.table.n_leaf if h is not None and not mc else 5
    c = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    tail = (d_facp, n_col, n_dim, None if c is None else c.ctypes.data, gamma, 1, 0, flags, d_x, xc, d_fac, d_root, d_a, d_sum, d_n_accept,
            None if mz is None else C.addressof(mz), None if cg is None else C.addressof(cg), n_bin, d_binp, d_bin, B, None)
    if mc:
        return capi.lib().fdg_mc_chain_step_device_binned(h._h if h else None, d_xp, xpc, 1.0, 2.0, 0.5, *tail)
    return capi.lib().fdg_chain_step_device_binned(h._h if h else None, d_xp, xpc, *tail)


def test_step_argument_checks(libfdg):
    t = workloads.get("sigma2")
    h = capi.GraphHandle(t)
    R = t.n_root
    arrays = ("d_xp", "d_facp", "d_x", "d_fac", "d_root", "d_a", "d_sum")
    for mc in (False, True):
        for name in arrays + ("d_bin", "d_binp"):
            assert failed(_step(h, mc, **{name: None}), capi.FDG_E_INVALID), name
        for i, a in enumerate(arrays):                      # any two of the state, proposal and sum arrays the same buffer
            for b in arrays[:i]:
                assert failed(_step(h, mc, **{a: FAKE[arrays.index(b)]}), capi.FDG_E_INVALID), (a, b)
            for name in ("d_bin", "d_binp"):                # ... and the bins no other array's
                assert failed(_step(h, mc, **{name: FAKE[i]}), capi.FDG_E_INVALID), (a, name)
        assert failed(_step(h, mc, d_n_accept=FAKE[6]), capi.FDG_E_INVALID) and failed(_step(h, mc, d_bin=FAKE[7]), capi.FDG_E_INVALID)
        assert failed(_step(h, mc, d_bin=FAKE[7] + 0x10000), capi.FDG_E_INVALID)                      # d_bin == d_binp
        for g in (0.0, -1.0, math.inf, math.nan):
            assert failed(_step(h, mc, gamma=g), capi.FDG_E_INVALID), g
        for kw in (dict(B=-1), dict(n_dim=0), dict(flags=4), dict(xc=99), dict(xpc=99), dict(coef=[math.nan] * R), dict(n_bin=0)):
            assert failed(_step(h, mc, **kw), capi.FDG_E_INVALID), kw
        assert failed(_step(None, mc), capi.FDG_E_INVALID)
        assert failed(_step(h, mc, n_dim=capi.FDG_VEGAS_DIM_MAX + 1), capi.FDG_E_UNSUPPORTED)
        assert failed(_step(h, mc, n_bin=capi.FDG_CHAIN_BIN_MAX + 1), capi.FDG_E_UNSUPPORTED)
        # a descriptor that is given is checked as the projected and the grouped step check it
        leaf = 0 if mc else t.n_leaf
        mz, _k1 = capi.make_chain_matsubara([0, 1], True, 2, [0] * R, [0] * R, 1.0)                  # weight_freq >= n_freq
        assert failed(_step(h, mc, mz=mz), capi.FDG_E_INVALID)
        mz, _k1 = capi.make_chain_matsubara([0, 1], True, 0, [0] * R, [max(leaf, 5)] * R, 1.0)        # a time column >= n_col
        assert failed(_step(h, mc, mz=mz), capi.FDG_E_INVALID)
        cg, _k2 = capi.make_chain_groups([1] * R, [(0,)])                                            # root_group >= n_group
        assert failed(_step(h, mc, cg=cg), capi.FDG_E_INVALID)
        cg, _k2 = capi.make_chain_groups([0] * R, [(0, 3)])                                          # a variable >= n_dim
        assert failed(_step(h, mc, cg=cg), capi.FDG_E_INVALID)
        cg, _k2 = capi.make_chain_groups([0] * R, [(0,)], [-1.0])
        assert failed(_step(h, mc, cg=cg), capi.FDG_E_INVALID)
    assert failed(_step(h, n_col=t.n_leaf + 1), capi.FDG_E_INVALID)                 # the leaf form: n_col is the number of leaves
    ok_mz, _k1 = capi.make_chain_matsubara([0, 1], True, 1, [0] * R, [1] * R, 1.0)
    ok_cg, _k2 = capi.make_chain_groups([0] * R, [(0, 2)], [2.0])
    assert _step(h, B=0) == capi.FDG_OK and _step(h, B=0, d_n_accept=None) == capi.FDG_OK and _step(h, B=0, mz=ok_mz, cg=ok_cg) == capi.FDG_OK
    assert _step(h, B=0, flags=INIT, d_sum=None) == capi.FDG_OK and _step(h, B=0, n_bin=capi.FDG_CHAIN_BIN_MAX) == capi.FDG_OK
    assert failed(_step(h, True, B=0), capi.FDG_E_INVALID)                           # fdg_graph_specialize_fused has not been called


# ---- 6. the known answers through the driver --------------------------------------------------------------------------------------------------- #
def test_leaf_form_known_answer_through_the_driver(libfdg, cuda):
    """The known answer of tests/test_chain_binned_host.py at seed 0: every (bin, root) within 5 reported sigma of 0.05 e_j and
    0.25 e_j^2, and the mirror's means.  The driver takes gamma from a torch sum over the 4096 walkers, the mirror from numpy's:
    either is within 4096 * 2^-53 = 5e-13 of the exact sum, and the means depend smoothly on it, so they agree to 1e-10 and not to the
    bit."""
    t, col, ecol, fixed = known_b_graph()
    k = KNOWN_B
    dm = vegas.DiscreteMap(cdf_of(k["p"]), np.array(k["ext"])[:, None], [ecol], device=cuda)
    res = vegas.chain_integrate_binned(fd.compile_table(t, specialize="isa"), None, [0, 0], [1, 1], col, dm, n_walker=k["n_walker"],
                                       n_step=k["n_step"], n_therm=k["n_therm"], moves=list(k["moves"]), gamma_rel=k["gamma_rel"], n_warm=0,
                                       n_grid=k["n_grid"], seed=0, fixed=fixed, device=cuda)
    mirror = known_b_mirror(0)
    print("device: mean", res.mean, "stderr", res.stderr, "acceptance", res.acceptance, "gamma", res.gamma)
    print("mirror: mean", mirror["mean"], "stderr", mirror["stderr"], "acceptance", mirror["acceptance"], "gamma", mirror["gamma"])
    assert res.mean.shape == res.stderr.shape == (4, 2) and res.S.shape == (9,)
    assert (np.abs(res.mean - k["exact"]) <= 5.0 * res.stderr).all()
    assert np.allclose(res.mean, mirror["mean"], rtol=1e-10, atol=0) and np.allclose(res.stderr, mirror["stderr"], rtol=1e-8, atol=0)
    assert math.isclose(res.gamma, mirror["gamma"], rel_tol=1e-12) and res.acceptance == mirror["acceptance"]
    assert np.array_equal(dm.cdf, cdf_of(k["p"]))                                  # no warm-up: the map is used as given


def test_monte_carlo_form_known_answer_with_a_warm_up(libfdg, cuda):
    """tests/test_vegas_discrete_accumulate.py's helper: one bosonic leaf on K_1 + K_2 with K_1 = q_j from the table, K_2 over
    [-L, L]^3; bin j holds 64 pi L^3 (lambda + L^2 + |q_j|^2).  4096 walkers, 40 steps with 8 discarded, a warm-up of 2 iterations
    of vegas_integrate_binned, which trains the map and the discrete variable's probabilities; every bin within 5 reported errors."""
    t, tab, _keep = leaf_on_k1_plus_k2(0)
    f = fd.compile_table(t, specialize="isa")
    L, lam, n_bin = 2.0, 0.05, 8
    q = np.array([[0.3 * j, -0.2 * j, 0.1 * j * j] for j in range(n_bin)])
    dm = vegas.DiscreteMap(vegas.uniform_cdf(n_bin), ext=q, ext_col=[0, 1, 2], device=cuda)
    res = vegas.chain_integrate_binned(f, tab, [-L] * 3, [L] * 3, [3, 4, 5], dm, 0.0, 1.0, lam, n_walker=4096, n_step=40, n_therm=8, n_warm=2,
                                       n_grid=16, seed=0, device=cuda)
    exact = 64.0 * math.pi * L ** 3 * (lam + L * L + (q * q).sum(axis=1))
    print("mean", res.mean[:, 0], "stderr", res.stderr[:, 0], "exact", exact, "pull", (res.mean[:, 0] - exact) / res.stderr[:, 0],
          "acceptance", res.acceptance, "gamma", res.gamma, "p", dm.prob)
    assert res.mean.shape == res.stderr.shape == (n_bin, 1)
    assert (res.stderr[:, 0] > 0).all() and (np.abs(res.mean[:, 0] - exact) <= 5.0 * res.stderr[:, 0]).all()
    assert dm.cdf[0] == 0.0 and dm.cdf[n_bin] == 1.0 and (np.diff(dm.cdf) > 0).all() and not np.array_equal(dm.cdf, vegas.uniform_cdf(n_bin))
    assert np.array_equal(dm.d_cdf.cpu().numpy(), dm.cdf)
    g = res.map.grid
    assert (np.diff(g, axis=1) > 0).all() and not np.array_equal(g, vegas.uniform_grid([-L] * 3, [L] * 3, 16))
