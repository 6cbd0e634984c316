"""The Markov chain with weight groups and reweighting between orders on the device (include/fdg.h: fdg_chain_step_device_grouped,
fdg_mc_chain_step_device_grouped; feynmandiagram.jl_amd/vegas.py: chain_integrate_grouped).  Every step is compared bit for bit with
the numpy mirror (capi.chain_grouped_reference): x, fac, root, a, sum, n_accept.  In the leaf form the mirror's roots are the CPU
oracle's; in the Monte-Carlo form they are fdg_mc_eval_device's on the mirror's own proposals, as in
tests/test_chain_matsubara_accumulate.py.  With one group, a full mask and no factors the step is tied bit for bit to the plain and to
the projected step.  The statistical conditions of known answer A are the ones the mirror alone meets in
tests/test_chain_groups_host.py."""
import math

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT
from test_chain_accumulate import PAD, SENT, STATE, DeviceChain, assert_reduced, assert_state
from test_chain_groups_host import GROUPS3, KNOWN_A, known_a_graph, known_a_grid, known_a_mirror
from test_chain_host import INIT, MEASURE, fresh_state, oracle_roots, step_uniforms
from test_chain_matsubara_accumulate import DeviceChainMz, device_mc_roots, leaf_case, mc_cases, step_list  # noqa: F401 (mc_cases: a fixture)
from test_matsubara_accumulate import phase_table
from test_strat_accumulate import assert_bits
from test_weight_groups_accumulate import two_orders

pytestmark = pytest.mark.gpu


class DeviceChainGrp(DeviceChain):
    """DeviceChain whose step is the grouped one; ``mz = (freq, fermionic, weight_freq, cin, cout, beta)`` or None"""

    def __init__(self, handle, cuda, grid, col, fixed, B, root_group, var_sets, reweight=None, mz=None, coef=None, shard_start=0):
        import torch
        super().__init__(handle, cuda, grid, col, fixed, B, coef, shard_start)
        self.mz = mz
        self.n_sum = self.R + 1 if mz is None else 2 * len(mz[0]) * self.R + 1
        self.total = torch.full((self.n_sum * B + PAD,), SENT, dtype=torch.float64, device=cuda)
        self.total[:self.n_sum * B] = 0.0
        self.desc = None
        if mz is not None:
            self.desc, self._keep = capi.make_chain_matsubara(*mz)
        self.groups, self._gkeep = capi.make_chain_groups(root_group, var_sets, reweight)

    def select(self, gamma, seed, off, flags, mc=None):
        tail = (self.facp.data_ptr(), self.C, self.D, self.coef, gamma, seed, off, flags, self.x.data_ptr(), self.xc, self.fac.data_ptr(),
                self.root.data_ptr(), self.a.data_ptr(), self.total.data_ptr(), self.n_acc.data_ptr(), self.desc, self.groups, self.B, self.st)
        if mc is None:
            self.h.chain_step_device_grouped(self.xp.data_ptr(), self.xc, *tail)
        else:
            self.h.mc_chain_step_device_grouped(self.xp.data_ptr(), self.xc, *mc, *tail)

    reduced = DeviceChainMz.reduced
    state = DeviceChainMz.state


def mz_dict(mz):
    return None if mz is None else dict(freq=mz[0], fermionic=mz[1], weight_freq=mz[2], root_col_in=mz[3], root_col_out=mz[4], beta=mz[5])


def mirror_state(fixed, D, R, B, mz):
    m = fresh_state(fixed, D, R, B)
    if mz is not None:
        m["sum"] = np.zeros((2 * len(mz[0]) * R + 1, B))
    return m


def mirror_step(m, grid, col, mask, seed, off, gamma, flags, ev, root_group, var_sets, reweight, mz, coef, exists):
    u, ua = step_uniforms(m["x"].shape[1], grid.shape[0], mask, seed, off)
    return capi.chain_grouped_reference(grid, col, m, mask, u, ua, gamma, flags, ev, root_group, var_sets, reweight, coef, exists, mz_dict(mz),
                                        phase_table)


RHO3 = (0.7, 1.9, 3.3)


def run_against_mirror(chain, m, grid, col, steps, seed, ev, groups, reweight, mz, coef, exists, what, mc=None, lo=0):
    for i, (mask, off, g, flags) in enumerate(steps):
        chain.step(mask, g, seed, off + lo, flags, mc)
        m = mirror_step(m, grid, col, mask, seed, off + lo, g, flags, ev, groups["root_group"], groups["var_sets"], reweight, mz, coef, exists)
        got = chain.state()
        assert_bits(got["xp"], m["xp"], f"{what}, step {i}: xp")
        assert_state(got, m, f"{what}, step {i}")
    return m


# ---- bit for bit against the mirror ------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("projected", [False, True])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_every_step_matches_the_mirror_bit_for_bit(libfdg, cuda, B, projected):
    """The random graph of tests/test_chain_accumulate.py (ten roots, one of which does not exist; three variables) in three groups:
    group 1 holds only the root that does not exist, variable 1 belongs to no group with a root, group 2 has an empty mask.  reweight
    given and NULL, coef given and NULL, mz NULL and a 3-frequency fermionic projection; after INIT and after every step."""
    t, f, col, fixed, grid, coef, exists, cin, cout = leaf_case(cuda)
    D, R, seed, gamma = len(col), t.n_root, 11, 0.37
    mz = ((2, -1, 0), True, 1, cin, cout, 1.7) if projected else None
    ev = oracle_roots(t)
    refused = 0
    for rho in (None, RHO3):
        for cf in (None, coef):
            chain = DeviceChainGrp(f.handle, cuda, grid, col, fixed, B, GROUPS3["root_group"], GROUPS3["var_sets"], rho, mz, cf)
            m = run_against_mirror(chain, mirror_state(fixed, D, R, B, mz), grid, col, step_list(D, B, gamma), seed, ev, GROUPS3, rho, mz, cf,
                                   exists, f"rho {rho is not None}, coef {cf is not None}")
            refused += int((m["n_accept"] < 8).sum())
            assert (m["sum"][-1] > 0.0).all()
            assert_reduced(chain.reduced(), m["sum"], "reduced sums")
    assert B < 63 or refused > 0                             # some proposals were refused


def test_walkers_over_several_chunks_and_from_two_shards(libfdg, cuda):
    """70 003 walkers with FDG_ROOT_SCRATCH_MB = 1 (chunks of 13 056 walkers, the last one of 4 723) against the mirror after every
    step, plain and projected; the same bits with the default scratch (one chunk), and from two shards."""
    B, seed, gamma = 70_003, 12, 0.37
    t, f1, col, fixed, grid, coef, exists, cin, cout = leaf_case(cuda, options={"FDG_ROOT_SCRATCH_MB": "1"})
    f = fd.compile_table(t, specialize="isa")
    D, R = len(col), t.n_root
    ev = oracle_roots(t)
    steps = step_list(D, B, gamma)
    for mz in (None, ((0, -2, 1), True, 2, cin, cout, 1.7)):
        def run(handle, n, lo, check):
            chain = DeviceChainGrp(handle, cuda, grid, col, fixed, n, GROUPS3["root_group"], GROUPS3["var_sets"], RHO3, mz, coef, lo)
            if check:
                run_against_mirror(chain, mirror_state(fixed, D, R, n, mz), grid, col, steps, seed, ev, GROUPS3, RHO3, mz, coef, exists, "chunks")
            else:
                for mask, off, g, flags in steps:
                    chain.step(mask, g, seed, off + lo, flags)
            return chain.state(), chain.reduced()
        small, small_red = run(f1.handle, B, 0, True)
        whole, whole_red = run(f.handle, B, 0, False)
        assert_state(whole, small, "FDG_ROOT_SCRATCH_MB changed")
        assert_bits(whole_red, small_red, "reduced sums, FDG_ROOT_SCRATCH_MB changed")
        assert 0 < (small["n_accept"] < 8).sum() and np.abs(small["sum"]).max() > 0.0
        cut = 30_001
        for lo, n in ((0, cut), (cut, B - cut)):
            part, _ = run(f1.handle, n, lo, False)
            for k in STATE:
                assert_bits(part[k], small[k][..., lo:lo + n], f"shard at {lo}: {k}")


def test_monte_carlo_form_with_groups_matches_the_mirror(mc_cases, cuda):
    """parquet_sigma2 in the Monte-Carlo form, its two roots in two groups (root 0: the momenta only; root 1: everything), with
    factors and a projection; the mirror's roots are fdg_mc_eval_device's"""
    c = mc_cases["parquet_sigma2"]
    t, h, col, grid, fixed = c["t"], c["f"].handle, c["col"], c["grid"], c["fixed"]
    B, D, R, seed = 1_229, len(col), t.n_root, 21
    kF, beta, lam, nk = c["phys"]
    n_mom = sum(1 for v in col if v < nk)
    groups = dict(root_group=[0, 1], var_sets=[tuple(range(n_mom)), tuple(range(D))])
    ev = device_mc_roots(h, cuda, c["phys"], R)
    for mz, rho in ((None, (2.5, 0.4)), (((0, -1, 2), True, 2, c["cin"], c["cout"], beta), None)):
        chain = DeviceChainGrp(h, cuda, grid, col, fixed, B, groups["root_group"], groups["var_sets"], rho, mz)
        m, gamma = mirror_state(fixed, D, R, B, mz), None
        for i, (mask, off, g, flags) in enumerate(step_list(D, B, 1.0)):
            if flags != INIT:
                g = gamma
            chain.step(mask, g, seed, off, flags, mc=(kF, beta, lam))
            m = mirror_step(m, grid, col, mask, seed, off, g, flags, ev, groups["root_group"], groups["var_sets"], rho, mz, None, None)
            assert_state(chain.state(), m, f"step {i}")
            if flags == INIT:
                gamma = float(m["a"].mean())
                assert gamma > 0.0
        assert 0 < (m["n_accept"] < 8).sum() and np.abs(m["sum"][:-1]).max() > 0.0


# ---- ties on the device ------------------------------------------------------------------------------------------------------------------ #
def tie(old, new, steps, mc=None, seed=9):
    for i, (mask, off, g, flags) in enumerate(steps):
        old.step(mask, g, seed, off, flags, mc)
        new.step(mask, g, seed, off, flags, mc)
        a, b = old.state(), new.state()
        for k in STATE:
            assert_bits(b[k], a[k], f"step {i}: {k}")
    assert 0 < (a["n_accept"] < len(steps)).sum() and np.abs(a["sum"][:-1]).max() > 0.0


def test_one_full_group_ties_the_step_to_the_existing_steps(mc_cases, cuda):
    """One group, a full mask and NULL reweight: the state and the sums of fdg_chain_step_device and of
    fdg_chain_step_device_matsubara in the leaf form, and of both mc_ forms on parquet_sigma2, bit for bit after every step."""
    t, f, col, fixed, grid, coef, exists, cin, cout = leaf_case(cuda)
    B, D, R = 1_229, len(col), t.n_root
    one = ([0] * R, [tuple(range(D))])
    mz = ((2, -1, 0), True, 1, cin, cout, 1.7)
    tie(DeviceChain(f.handle, cuda, grid, col, fixed, B, coef), DeviceChainGrp(f.handle, cuda, grid, col, fixed, B, *one, None, None, coef),
        step_list(D, B, 0.37))
    tie(DeviceChainMz(f.handle, cuda, grid, col, fixed, B, mz, coef), DeviceChainGrp(f.handle, cuda, grid, col, fixed, B, *one, None, mz, coef),
        step_list(D, B, 0.37))
    c = mc_cases["parquet_sigma2"]
    h, R, D = c["f"].handle, c["t"].n_root, len(c["col"])
    kF, beta, lam, _ = c["phys"]
    one = ([0] * R, [tuple(range(D))])
    mz = ((0, -1, 2), True, 2, c["cin"], c["cout"], beta)
    probe = DeviceChain(h, cuda, c["grid"], c["col"], c["fixed"], B)
    probe.step((1 << D) - 1, 1.0, 9, 17, INIT, (kF, beta, lam))
    gamma = float(probe.state()["a"].mean())
    args = (h, cuda, c["grid"], c["col"], c["fixed"], B)
    tie(DeviceChain(*args), DeviceChainGrp(*args, *one), step_list(D, B, gamma), (kF, beta, lam))
    tie(DeviceChainMz(*args, mz), DeviceChainGrp(*args, *one, None, mz), step_list(D, B, gamma), (kF, beta, lam))


# ---- the largest shape ------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def ver4(libfdg):
    """parquet_ver4_4 and its compiled function: built once, shared, never written to"""
    t = workloads.get("parquet_ver4_4")
    return t, fd.compile_table(t, specialize="isa")


@pytest.mark.parametrize("n_freq", [0, 4])
def test_180_roots_64_variables_and_8_groups(ver4, cuda, n_freq):
    """The graph of tests/test_chain_accumulate.py::test_180_roots_and_64_variables: parquet_ver4_4 in the leaf form with 64 of its
    leaves as variables, 8 groups with nested masks (group g holds the variables 0 .. 8 g + 7) and the roots spread over them (root k
    in group k mod 8), with factors.  Once plain and once with 4 frequencies; 256 walkers, INIT and 3 steps."""
    t, f = ver4
    B, D, G, seed, beta = 256, capi.FDG_VEGAS_DIM_MAX, 3, 9, 1.0
    NG = capi.FDG_WEIGHT_GROUP_MAX
    rng = np.random.default_rng(6)
    col = [int(c) for c in rng.permutation(t.n_leaf)[:D]]
    fixed = rng.uniform(0.2, 1.0, size=t.n_leaf)
    grid = capi.vegas_refine(vegas.uniform_grid([0.2] * D, [1.0] * D, G), rng.random((D, G)) + 0.5, 1.0)
    coef = rng.uniform(-1.0, 1.0, size=t.n_root)
    groups = dict(root_group=[k % NG for k in range(t.n_root)], var_sets=[tuple(range(8 * g + 8)) for g in range(NG)])
    rho = tuple(rng.uniform(0.5, 2.0, size=NG))
    tin, tout = workloads.root_times("parquet_ver4_4")
    mz = ((0, 1, -3, 7), True, 3, [int(i) - 1 for i in tin], [int(i) - 1 for i in tout], beta) if n_freq else None
    ev = oracle_roots(t)
    chain = DeviceChainGrp(f.handle, cuda, grid, col, fixed, B, groups["root_group"], groups["var_sets"], rho, mz, coef)
    full = (1 << D) - 1
    # gamma: the mean of a on the first placement (the driver's gamma_rel = 1), from the mirror
    m = mirror_step(mirror_state(fixed, D, t.n_root, B, mz), grid, col, full, seed, 1 << 32, 1.0, INIT, ev, groups["root_group"],
                    groups["var_sets"], rho, mz, coef, None)
    gamma = float(m["a"].mean())
    assert gamma > 0.0
    steps = [(full, (1 << 32) + i * B, 1.0 if i == 0 else gamma, flags)
             for i, flags in enumerate([INIT, MEASURE, MEASURE, MEASURE])]
    steps[2] = (0x8000000000000001,) + steps[2][1:]
    m = run_against_mirror(chain, mirror_state(fixed, D, t.n_root, B, mz), grid, col, steps, seed, ev, groups, rho, mz, coef, None, "largest")
    assert 0 < (m["n_accept"] < 4).sum() < B and np.abs(m["sum"][-2]).max() > 0.0


# ---- poison ------------------------------------------------------------------------------------------------------------------------------ #
def poison_case():
    """tests/test_chain_accumulate.py's poison_graph with a fourth root that does not exist: r_0 = (2e154 x)^2 is inf for x > 0.67,
    r_1 = r_0 - (2e154 y)^2 nan where both overflow, r_2 = x y finite everywhere, over [0, 1]^2"""
    x, y = fd.Graph([]), fd.Graph([])
    bx = fd.Graph([fd.Graph([x], subgraph_factors=[2e154], operator=fd.Sum())], operator=fd.Power(2))
    by = fd.Graph([fd.Graph([y], subgraph_factors=[2e154], operator=fd.Sum())], operator=fd.Power(2))
    r1 = fd.Graph([bx, by], subgraph_factors=[1.0, -1.0], operator=fd.Sum())
    r2 = fd.Graph([x, y], operator=fd.Prod())
    t, leafmap, _ = lower([bx, r1, r2], root=[bx.id, r1.id, r2.id, 424_242])
    at = {g.id: i - 1 for i, g in leafmap.items()}
    assert t.n_leaf == 2 and t.n_root == 4 and int(t.root_slot[3]) == FDG_NO_ROOT
    return t, [at[x.id], at[y.id]]


POISON = [
    # (what, grid of x, coef, reweight, projected): r_0 in group 0 with x only, r_1 and r_2 in group 1 with y only, whose map is
    # uniform: jac_1 = 1, so whatever of r_1 is finite stays finite in the measurement
    ("jac_g s_g overflows", [0.0, 0.1, 0.2, 0.3, 1.0], (1.0, 1.0, 1.0), None, False),          # fac_0 = 2.8 where x > 0.3: 0.4 < x < 0.67
    ("rho_g a_g overflows", [0.0, 0.25, 0.5, 0.75, 1.0], (1.0, 1.0, 1.0), (4.0, 1.0), False),  # 4 r_0 = inf where 0.34 < x < 0.67
    ("q_g overflows", [0.0, 0.25, 0.5, 0.75, 1.0], (1e-153, 1e-153, 1.0), (1.0, 1.0), True),  # a term above 1.3e154 squares to inf: x > 0.18
]


@pytest.mark.parametrize("what,gx,coef,rho,projected", POISON)
def test_poisoned_proposals_count_as_zero(libfdg, cuda, what, gx, coef, rho, projected):
    """A root that is not finite in one group zeroes the whole proposal, the other group's root too; so does a finite root whose
    jac_g s_g (or rho_g a_g, or q_g) overflows.  a never becomes inf or nan, nothing that is not finite reaches the state or a sum,
    the columns of the root that does not exist stay untouched, and the mirror agrees bit for bit."""
    t, col = poison_case()
    f = fd.compile_table(t, specialize="isa")
    B, seed, gamma, R = 300, 4, 0.5, 4
    grid = np.array([gx, [0.0, 0.25, 0.5, 0.75, 1.0]])
    coef = np.array(coef + (1.0,))
    groups = dict(root_group=[0, 1, 1, 5], var_sets=[(0,), (1,)])
    mz = ((0, -2), True, 1, [0, 1, 0, 9], [1, 0, 0, 9], 0.8) if projected else None
    exists = [True, True, True, False]
    ev = oracle_roots(t)
    chain = DeviceChainGrp(f.handle, cuda, grid, col, np.zeros(2), B, groups["root_group"], groups["var_sets"], rho, mz, coef)
    m = mirror_state(np.zeros(2), 2, R, B, mz)
    gone = [3] if mz is None else [2 * (fr * R + 3) + p for fr in range(2) for p in (0, 1)]
    chain.root[3 * B:4 * B] = 3.5
    m["root"][3] = 3.5
    for c in gone:
        chain.total[c * B:(c + 1) * B] = -9.75
        m["sum"][c] = -9.75
    n_bad = n_overflow = 0
    for i, (mask, flags) in enumerate([(3, INIT)] + [(mask, MEASURE) for mask in (3, 1, 2, 3, 0, 3, 1)]):
        off = i * B
        chain.step(mask, gamma, seed, off, flags)
        got = chain.state()
        m = mirror_step(m, grid, col, mask, seed, off, gamma, flags, ev, groups["root_group"], groups["var_sets"], rho, mz, coef, exists)
        rp = ev(m["xp"])[:3]
        bad = ~np.isfinite(rp).all(axis=0)
        zeroed = m["accept"] & (m["root"][:3] == 0.0).all(axis=0) & (m["a"] == 0.0)
        n_bad += int(bad.sum())
        n_overflow += int((zeroed & ~bad & (rp[2] != 0.0)).sum())        # every root finite, and the proposal counts as zero all the same
        assert zeroed[bad & m["accept"]].all()
        assert_state(got, m, f"step {i}")
        assert all(np.isfinite(got[k]).all() for k in ("x", "fac", "root", "a", "sum"))
        assert (got["root"][3] == 3.5).all() and (got["sum"][gone] == -9.75).all()
    assert n_bad > B and n_overflow > 0 and 0 < (m["a"] == 0.0).sum() < B, (what, n_bad, n_overflow)


# ---- the known answers -------------------------------------------------------------------------------------------------------------------- #
def test_known_answer_a_through_the_driver(libfdg, cuda):
    """Known answer A of tests/test_chain_groups_host.py at seed 0: within 5 reported sigma of 1.4, 0.35 and 1.0, and the mirror's
    means.  The driver takes rho and gamma from torch sums over the 4096 walkers, the mirror from numpy's: either is within
    4096 * 2^-53 = 5e-13 of the exact sum, and the means depend smoothly on both, so they agree to 1e-10 and not to the bit."""
    t, col, fixed = known_a_graph()
    k = KNOWN_A
    f = fd.compile_table(t, specialize="isa")
    res = vegas.chain_integrate_grouped(f, None, k["lo"], k["hi"], col, vegas.WeightGroups(k["root_group"], k["var_sets"]), n_walker=k["n_walker"],
                                        n_step=k["n_step"], n_therm=k["n_therm"], moves=list(k["moves"]), gamma_rel=k["gamma_rel"], n_warm=0,
                                        seed=0, fixed=fixed, coef=list(k["coef"]), vmap=vegas.VegasMap(known_a_grid(), cuda), device=cuda)
    mirror = known_a_mirror(0)
    print("device: mean", res.mean, "stderr", res.stderr, "acceptance", res.acceptance, "rho", res.reweight, "gamma", res.gamma)
    print("mirror: mean", mirror["mean"], "stderr", mirror["stderr"], "acceptance", mirror["acceptance"], "rho", mirror["reweight"])
    assert (np.abs(res.mean - k["exact"]) <= 5.0 * res.stderr).all()
    assert np.allclose(res.mean, mirror["mean"], rtol=1e-10, atol=0) and np.allclose(res.stderr, mirror["stderr"], rtol=1e-8, atol=0)
    assert np.allclose(res.reweight, mirror["reweight"], rtol=1e-12, atol=0) and math.isclose(res.gamma, mirror["gamma"], rel_tol=1e-12)
    assert res.acceptance == mirror["acceptance"]


def test_known_answer_b_two_orders_through_the_driver(libfdg, cuda):
    """tests/test_weight_groups_accumulate.py's two orders in one run, Monte-Carlo form: I = int over [-L, L]^3 of 8 pi (|K|^2 + lambda)
    = 64 pi L^3 (lambda + L^2); root 0 integrates K_1 only, root 1 both, so the exact values are I and I^2.  Both means within 5
    sigma, and the factors come back.  The run with all factors 1 is printed beside it; no improvement is asserted (with
    gamma_rel = 1 the gamma q term carries half the density)."""
    L, lam = 2.0, 0.05
    exact = 64.0 * math.pi * L ** 3 * (lam + L * L)
    want = np.array([exact, exact ** 2])
    t, tab, _keep = two_orders()
    f = fd.compile_table(t, specialize="isa")
    groups = vegas.groups_from_dof([[1], [2]], [[[0, 1, 2], [3, 4, 5]]])
    kw = dict(n_walker=4096, n_step=40, n_therm=8, n_warm=0, seed=0, device=cuda)
    res = vegas.chain_integrate_grouped(f, tab, [-L] * 6, [L] * 6, list(range(6)), groups, 0.0, 1.0, lam, **kw)
    flat = vegas.chain_integrate_grouped(f, tab, [-L] * 6, [L] * 6, list(range(6)), groups, 0.0, 1.0, lam, reweight=[1.0, 1.0], **kw)
    for name, r in (("reweighted", res), ("all factors 1", flat)):
        print(name, "mean", r.mean, "stderr", r.stderr, "relative error", r.mean / want - 1.0, "pull", (r.mean - want) / r.stderr,
              "acceptance", r.acceptance, "rho", r.reweight, "gamma", r.gamma)
    assert (np.abs(res.mean - want) <= 5.0 * res.stderr).all()
    assert res.reweight is not None and res.reweight.shape == (2,) and (res.reweight > 0.0).all()
    assert np.array_equal(flat.reweight, [1.0, 1.0])


def test_the_warm_up_trains_the_map_with_the_grouped_sampler(libfdg, cuda):
    """Both forms with n_warm = 2: the leaf form trains through vegas_integrate_stratified(groups=...), the Monte-Carlo form through
    vegas_integrate(groups=...); the map that comes back is trained and valid, and the known answers hold within 5 sigma on it."""
    t, col, fixed = known_a_graph()
    k = KNOWN_A
    res = vegas.chain_integrate_grouped(fd.compile_table(t, specialize="isa"), None, k["lo"], k["hi"], col,
                                        vegas.WeightGroups(k["root_group"], k["var_sets"]), n_walker=k["n_walker"], n_step=k["n_step"],
                                        n_therm=k["n_therm"], moves=list(k["moves"]), n_warm=2, n_grid=k["n_grid"], seed=0, fixed=fixed,
                                        coef=list(k["coef"]), device=cuda)
    print("leaf form: mean", res.mean, "stderr", res.stderr, "acceptance", res.acceptance, "rho", res.reweight)
    g = res.map.grid
    assert (np.diff(g, axis=1) > 0).all() and not np.array_equal(g, vegas.uniform_grid(k["lo"], k["hi"], k["n_grid"]))
    assert (np.abs(res.mean - k["exact"]) <= 5.0 * res.stderr).all() and (res.reweight > 0.0).all()
    L, lam = 2.0, 0.05
    exact = 64.0 * math.pi * L ** 3 * (lam + L * L)
    t, tab, _keep = two_orders()
    res = vegas.chain_integrate_grouped(fd.compile_table(t, specialize="isa"), tab, [-L] * 6, [L] * 6, list(range(6)),
                                        vegas.groups_from_dof([[1], [2]], [[[0, 1, 2], [3, 4, 5]]]), 0.0, 1.0, lam, n_walker=4096, n_step=40,
                                        n_therm=8, n_warm=2, n_grid=16, seed=0, device=cuda)
    print("Monte-Carlo form: mean", res.mean, "stderr", res.stderr, "acceptance", res.acceptance, "rho", res.reweight)
    g = res.map.grid
    assert (np.diff(g, axis=1) > 0).all() and not np.array_equal(g[3:], vegas.uniform_grid([-L] * 3, [L] * 3, 16))
    assert (np.abs(res.mean - [exact, exact ** 2]) <= 5.0 * res.stderr).all()
