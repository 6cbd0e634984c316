"""The Markov chain's proposal with spherical momentum variables on the device (include/fdg.h: fdg_chain_propose_device_polar;
feynmandiagram.jl_amd/vegas.py: chain_integrate_polar).  Without groups the entry is tied bit for bit to fdg_chain_propose_device and
fdg_chain_propose_device_discrete; a full proposal is tied bit for bit to the direct sampler (fdg_vegas_sample_device_polar); partial
masks and whole runs -- INIT and four steps through the plain, the projected, the grouped and the binned step -- are compared bit for
bit with the numpy mirror (capi.chain_propose_polar_reference, then the step mirrors as they are): x, fac, bin, root, a, sum, n_accept.
The statistical conditions of the known answers are the ones the mirror alone meets in tests/test_chain_polar_host.py."""
import math

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas
from test_chain_accumulate import PAD, SENT, DeviceChain, assert_reduced
from test_chain_groups_accumulate import RHO3
from test_chain_groups_host import GROUPS3
from test_chain_host import INIT, MEASURE, fresh_state, oracle_roots, philox_columns
from test_chain_binned_host import fresh_binned_state
from test_chain_matsubara_accumulate import device_mc_roots, leaf_case, mc_cases  # noqa: F401 (mc_cases: a fixture)
from test_chain_polar_host import (FULL_CONFIGS, KNOWN_M, KNOWN_W, ball_volume, full_case, jac_bound, known_m_mirror, known_w_qtab,
                                   measure_graph, mirror_polar_step)
from test_strat_accumulate import assert_bits
from test_vegas_discrete_accumulate import refined_cdf
from test_vegas_polar_accumulate import ball_integral, leaf_on_k1_plus_k2
from test_vegas_polar_host import mirror_sincos

pytestmark = pytest.mark.gpu


class DeviceChainPolar(DeviceChain):
    """DeviceChain whose proposal is fdg_chain_propose_device_polar and whose step is the plain one, the projected one (``mz``), the
    grouped one (``groups``: a dict of root_group and var_sets) or, with ``cdf``, the binned one: fac / facp [D + 1, B], bin / binp
    int32 [B]; bit D of a step's mask moves the discrete variable."""

    def __init__(self, handle, cuda, grid, col, polar, fixed, B, cdf=None, ext=None, ext_col=(), groups=None, reweight=None, mz=None, coef=None,
                 shard_start=0):
        import torch
        super().__init__(handle, cuda, grid, col, fixed, B, coef, shard_start)
        D, R = self.D, self.R
        self.polar, self.ext_col = polar, [int(e) for e in ext_col]
        self.n_bin = 0 if cdf is None else len(cdf) - 1
        self.DV = D + (cdf is not None)
        self.d_cdf = None if cdf is None else torch.from_numpy(np.ascontiguousarray(cdf, dtype=np.float64)).to(cuda)
        self.d_ext = None if ext is None else torch.from_numpy(np.ascontiguousarray(ext, dtype=np.float64)).to(cuda)
        self.n_sum = max(self.n_bin, 1) * (R if mz is None else 2 * len(mz[0]) * R) + 1
        f64 = dict(dtype=torch.float64, device=cuda)
        self.fac, self.facp = torch.full((self.DV * B + PAD,), SENT, **f64), torch.full((self.DV * B + PAD,), SENT, **f64)
        self.total = torch.full((self.n_sum * B + PAD,), SENT, **f64)
        self.bins, self.binp = (torch.full((B + PAD,), int(SENT), dtype=torch.int32, device=cuda) for _ in range(2))
        self.fac[:self.DV * B], self.total[:self.n_sum * B], self.bins[:B] = 1.0, 0.0, 0
        self.desc = self.groups = None
        if mz is not None:
            self.desc, self._keep = capi.make_chain_matsubara(*mz)
        if groups is not None:
            self.groups, self._gkeep = capi.make_chain_groups(groups["root_group"], groups["var_sets"], reweight)

    def propose(self, mask, seed, off):
        D, disc = self.D, self.d_cdf is not None
        capi.chain_propose_device_polar(self.d_grid.data_ptr(), D, self.G, self.col, self.C, mask & ((1 << D) - 1), seed, off, self.x.data_ptr(),
                                        self.xc, self.fac.data_ptr(), self.xp.data_ptr(), self.xc, self.facp.data_ptr(), bool((mask >> D) & 1),
                                        self.d_cdf.data_ptr() if disc else 0, self.n_bin, 0 if self.d_ext is None else self.d_ext.data_ptr(),
                                        self.ext_col, self.bins.data_ptr() if disc else 0, self.binp.data_ptr() if disc else 0, self.polar,
                                        self.B, self.st)

    def select(self, gamma, seed, off, flags, mc=None):
        head = (self.xp.data_ptr(), self.xc) + (() if mc is None else tuple(mc))
        tail = (self.facp.data_ptr(), self.C, self.D, self.coef, gamma, seed, off, flags, self.x.data_ptr(), self.xc, self.fac.data_ptr(),
                self.root.data_ptr(), self.a.data_ptr(), self.total.data_ptr(), self.n_acc.data_ptr())
        pre = "chain_step_device" if mc is None else "mc_chain_step_device"
        if self.d_cdf is not None:
            getattr(self.h, pre + "_binned")(*head, *tail, self.desc, self.groups, self.n_bin, self.binp.data_ptr(), self.bins.data_ptr(), self.B,
                                             self.st)
        elif self.groups is not None:
            getattr(self.h, pre + "_grouped")(*head, *tail, self.desc, self.groups, self.B, self.st)
        elif self.desc is not None:
            getattr(self.h, pre + "_matsubara")(*head, *tail, self.desc, self.B, self.st)
        else:
            getattr(self.h, pre)(*head, *tail, self.B, self.st)

    def reduced(self):
        import torch
        out = torch.zeros(3 * (self.n_sum - 1) + 2, dtype=torch.float64, device=self.cuda)
        capi.chain_reduce_device(self.total.data_ptr(), self.n_sum - 1, self.B, out.data_ptr(), self.st)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def state(self):
        """DeviceChain.state with the rows of fac, the larger sum and, with a discrete variable, the bins"""
        import torch
        torch.cuda.synchronize()
        B, DV, R = self.B, self.DV, self.R
        x, xp = self.x.cpu().numpy(), self.xp.cpu().numpy()
        assert (x[:, B:] == SENT).all() and (xp[:, B:] == SENT).all(), "a lane past n_walker of x or xp was written"
        out = {"x": x[:, :B].copy(), "xp": xp[:, :B].copy()}
        arrays = [("fac", self.fac, DV * B), ("facp", self.facp, DV * B), ("root", self.root, R * B), ("a", self.a, B),
                  ("sum", self.total, self.n_sum * B), ("n_accept", self.n_acc, B), ("bin", self.bins, B), ("binp", self.binp, B)]
        for name, t, n in arrays:
            h = t.cpu().numpy()
            assert (h[n:] == (SENT if h.dtype == np.float64 else int(SENT))).all(), name + ": a word past the array was written"
            out[name] = h[:n].reshape(-1, B).copy() if name not in ("a", "n_accept", "bin", "binp") else h[:n].copy()
        if self.d_cdf is None:
            assert (out["bin"] == 0).all() and (out["binp"] == int(SENT)).all()      # no discrete variable: never touched
        return out


def state_keys(disc):
    return ("x", "fac", "root", "a", "sum", "n_accept") + (("bin",) if disc else ())


def run_against_mirror(chain, m, grid, col, polar, steps, seed, ev, cdf, ext, ext_col, groups, reweight, mz, coef, exists, what, mc=None, lo=0):
    mzd = None if mz is None else dict(freq=mz[0], fermionic=mz[1], weight_freq=mz[2], root_col_in=mz[3], root_col_out=mz[4], beta=mz[5])
    for i, (mask, off, g, flags) in enumerate(steps):
        chain.step(mask, g, seed, off + lo, flags, mc)
        m = mirror_polar_step(m, grid, col, polar, mask, seed, off + lo, g, flags, ev, cdf, ext, ext_col, groups, reweight, mzd, coef, exists)
        got = chain.state()
        for k in ("xp", "facp") + (("binp",) if cdf is not None else ()) + state_keys(cdf is not None):
            assert_bits(got[k], m[k], f"{what}, step {i}: {k}")
    return m


# ---- 1. without groups the entry is the proposals that exist ---------------------------------------------------------------------------------- #
@pytest.mark.parametrize("D", [1, 5, 63, 64])
def test_no_groups_ties_the_entry_to_the_existing_proposals(libfdg, cuda, D):
    """n_polar = 0: xp and facp are fdg_chain_propose_device's bit for bit (d_cdf NULL; 64 variables allowed), and xp, facp and binp
    fdg_chain_propose_device_discrete's, whether the discrete variable moves or not; full, empty and random masks; 1, 65 and 1229
    walkers; a refined grid and cdf; three columns that nobody names."""
    import torch
    rng = np.random.default_rng(D)
    G, n_bin, n_ext, seed, off = 6, 7, 2, 0x1234_5678_9ABC, 3_000_000_011
    C = D + n_ext + 3
    grid = capi.vegas_refine(vegas.uniform_grid([-1.0] * D, [2.0] * D, G), rng.random((D, G)) + 0.5, 1.0)
    cdf, ext = refined_cdf(rng, n_bin), rng.uniform(-5.0, 5.0, size=(n_bin, n_ext))
    perm = rng.permutation(C)
    col, ext_col = [int(c) for c in perm[:D]], [int(c) for c in perm[D:D + n_ext]]
    st = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=cuda)
    d_grid, d_cdf, d_ext = (torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for v in (grid, cdf, ext))
    full = (1 << D) - 1
    for B in (1, 65, 1_229):
        x = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(C, B))).to(cuda)
        bins = torch.from_numpy(rng.integers(0, n_bin, size=B).astype(np.int32)).to(cuda)
        for mask in (full, 0, int(rng.integers(0, 1 << 62)) & full):
            for discrete, move in ((False, False), (True, False), (True, True)):
                if discrete and D == 64:
                    continue
                DV = D + discrete
                fac = torch.from_numpy(rng.uniform(0.5, 2.0, size=(DV, B))).to(cuda)
                out = []
                for polar in (False, True):
                    xp, facp = torch.full((C, B), -77.0, **f64), torch.full((DV, B), -77.0, **f64)
                    binp = torch.full((B,), -5, dtype=torch.int32, device=cuda)
                    head = (d_grid.data_ptr(), D, G, col, C, mask, seed, off, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B, facp.data_ptr())
                    disc = (move, d_cdf.data_ptr(), n_bin, d_ext.data_ptr(), ext_col, bins.data_ptr(), binp.data_ptr())
                    if polar:
                        capi.chain_propose_device_polar(*head, *(disc if discrete else (move, 0, 0, 0, None, 0, 0)), [], B, st)
                    elif discrete:
                        capi.chain_propose_device_discrete(*head, *disc, B, st)
                    else:
                        capi.chain_propose_device(*head, B, st)
                    torch.cuda.synchronize()
                    out.append((xp.cpu().numpy(), facp.cpu().numpy(), binp.cpu().numpy()))
                what = f"B {B}, mask {mask:#x}, discrete {discrete}, move {move}"
                assert_bits(out[1][0], out[0][0], what + ": xp")
                assert_bits(out[1][1], out[0][1], what + ": facp")
                assert np.array_equal(out[1][2], out[0][2]) and (discrete or (out[1][2] == -5).all()), what
                assert not (out[1][0] == -77.0).any() and not (out[1][1] == -77.0).any()


# ---- 2. a full proposal is the direct sampler's draw --------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("G", [1, 64])
@pytest.mark.parametrize("config", list(FULL_CONFIGS))
def test_a_full_proposal_is_the_direct_samplers_draw(libfdg, cuda, config, G):
    """Every variable (and the discrete one) redrawn: xp, the groups' columns and ext_col included, is fdg_vegas_sample_device_polar's
    x and binp its d_bin (bin_base 0) for the same seed and offset, bit for bit; the unnamed columns are copied from x.  The product
    of the rows of facp agrees with the sampler's jac to 2 (D + 3 n_polar) 2^-53 relative: both are folds of the same factors in
    different orders, at most D + 3 n_polar rounded products each."""
    import torch
    grid, col, polar, cdf, ext, ext_col, C = full_case(config, G)
    D, seed, off = grid.shape[0], 0x1234_5678_9ABC, 3_000_000_011
    disc = cdf is not None
    n_bin = len(cdf) - 1 if disc else 0
    st = torch.cuda.current_stream().cuda_stream
    f64 = dict(dtype=torch.float64, device=cuda)
    d_grid = torch.from_numpy(np.ascontiguousarray(grid)).to(cuda)
    d_cdf, d_ext = (torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for v in (cdf, ext)) if disc else (None, None)
    rng = np.random.default_rng(5)
    for B in (1, 63, 64, 65, 257):
        x = torch.from_numpy(rng.uniform(-1.0, 1.0, size=(C, B))).to(cuda)
        fac, facp, xp = torch.ones((D + disc, B), **f64), torch.full((D + disc, B), -77.0, **f64), torch.full((C, B), -77.0, **f64)
        bins, binp = torch.zeros(B, dtype=torch.int32, device=cuda), torch.full((B,), -5, dtype=torch.int32, device=cuda)
        capi.chain_propose_device_polar(d_grid.data_ptr(), D, G, col, C, (1 << D) - 1, seed, off, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B,
                                        facp.data_ptr(), True, d_cdf.data_ptr() if disc else 0, n_bin, d_ext.data_ptr() if disc else 0, ext_col,
                                        bins.data_ptr() if disc else 0, binp.data_ptr() if disc else 0, polar, B, st)
        sx, jac = torch.full((C, B), -77.0, **f64), torch.zeros(B, **f64)
        sb = torch.full((B,), -5, dtype=torch.int32, device=cuda)
        capi.vegas_sample_device_polar(d_grid.data_ptr(), D, G, col, d_cdf.data_ptr() if disc else 0, n_bin, 0, d_ext.data_ptr() if disc else 0,
                                       ext_col, polar, seed, off, sx.data_ptr(), 1, B, jac.data_ptr(), sb.data_ptr() if disc else 0, 0, B, st)
        torch.cuda.synchronize()
        named = [c for c in col if c is not None] + [c for _, cols in polar for c in cols] + list(ext_col)
        rest = [c for c in range(C) if c not in named]
        hxp, hsx, hb, hf, hj = xp.cpu().numpy(), sx.cpu().numpy(), binp.cpu().numpy(), facp.cpu().numpy(), jac.cpu().numpy()
        assert_bits(hxp[named], hsx[named], f"B {B}: xp")
        assert len(rest) == 3 and np.array_equal(hxp[rest], x.cpu().numpy()[rest]) and (hsx[rest] == -77.0).all()
        assert np.array_equal(hb, sb.cpu().numpy()) and (hb.min() >= 0 and hb.max() < n_bin if disc else (hb == -5).all())
        j = hf[0].copy()
        for d in range(1, D + disc):
            j = j * hf[d]
        assert (hf >= 0.0).all() and (hj > 0.0).all()
        assert (np.abs(j - hj) <= jac_bound(D, len(polar)) * hj).all(), (B, (np.abs(j - hj) / hj).max() / 2.0 ** -53)


# ---- 3. partial masks ------------------------------------------------------------------------------------------------------------------------ #
def test_every_unit_alone_matches_the_mirror_and_leaves_the_rest(libfdg, cuda):
    """17 variables in four groups (listed out of variable order) and six variables of no group, and the discrete variable: every
    group alone, every lone variable alone and the discrete variable alone, xp, facp and binp bit for bit against the mirror;
    whatever the move does not name -- columns, rows of fac, the bin -- is the state's."""
    import torch
    grid, col, polar, cdf, ext, ext_col, C = full_case("mixed_discrete", 64)
    D, B, seed, off = grid.shape[0], 257, 77, 1 << 33
    n_bin = len(cdf) - 1
    rng = np.random.default_rng(9)
    state = dict(x=rng.uniform(-1.0, 1.0, size=(C, B)), fac=rng.uniform(0.5, 2.0, size=(D + 1, B)), bin=rng.integers(0, n_bin, size=B).astype(np.int32))
    st = torch.cuda.current_stream().cuda_stream
    d_grid, d_cdf, d_ext, x, fac, bins = (torch.from_numpy(np.ascontiguousarray(v)).to(cuda)
                                          for v in (grid, cdf, ext, state["x"], state["fac"], state["bin"]))
    units = vegas.chain_moves_polar(D + 1, polar)[1:]
    assert len(units) == 4 + 6 + 1 and sum(units) == (1 << (D + 1)) - 1
    cols_of = {}                                              # the columns and the rows of fac of every unit, by its mask
    for var, cols in polar:
        cols_of[((1 << len(cols)) - 1) << var] = (list(cols), list(range(var, var + len(cols))))
    for d in range(D):
        if col[d] is not None:
            cols_of[1 << d] = ([col[d]], [d])
    cols_of[1 << D] = (list(ext_col), [D])
    for mask in units + [units[0] | units[3] | units[-1], 0]:
        xp, facp = torch.full((C, B), -77.0, dtype=torch.float64, device=cuda), torch.full((D + 1, B), -77.0, dtype=torch.float64, device=cuda)
        binp = torch.full((B,), -5, dtype=torch.int32, device=cuda)
        capi.chain_propose_device_polar(d_grid.data_ptr(), D, 64, col, C, mask & ((1 << D) - 1), seed, off, x.data_ptr(), B, fac.data_ptr(),
                                        xp.data_ptr(), B, facp.data_ptr(), bool((mask >> D) & 1), d_cdf.data_ptr(), n_bin, d_ext.data_ptr(), ext_col,
                                        bins.data_ptr(), binp.data_ptr(), polar, B, st)
        torch.cuda.synchronize()
        u = np.zeros((B, D))
        ds = [d for d in range(D) if (mask >> d) & 1]
        if ds:
            u[:, ds] = philox_columns(B, ds, seed, off)
        ud = philox_columns(B, [D], seed, off)[:, 0]
        wx, wf, wb = capi.chain_propose_polar_reference(grid, col, polar, state, mask & ((1 << D) - 1), u, cdf, ext, ext_col, bool((mask >> D) & 1), ud,
                                                        mirror_sincos)
        hx, hf, hb = xp.cpu().numpy(), facp.cpu().numpy(), binp.cpu().numpy()
        assert_bits(hx, wx, f"mask {mask:#x}: xp")
        assert_bits(hf, wf, f"mask {mask:#x}: facp")
        assert np.array_equal(hb, wb), mask
        moved_c = sorted(c for m, (cs, _) in cols_of.items() if m & mask for c in cs)
        moved_r = sorted(r for m, (_, rs) in cols_of.items() if m & mask for r in rs)
        keep_c, keep_r = [c for c in range(C) if c not in moved_c], [r for r in range(D + 1) if r not in moved_r]
        assert np.array_equal(hx[keep_c], state["x"][keep_c]) and np.array_equal(hf[keep_r], state["fac"][keep_r]), mask
        assert ((mask >> D) & 1) or np.array_equal(hb, state["bin"])
        if mask:
            assert (hx[moved_c] != state["x"][moved_c]).any(axis=1).all() and (hf[moved_r] != state["fac"][moved_r]).any(axis=1).all()


# ---- 4. INIT and four steps against the mirror -------------------------------------------------------------------------------------------------- #
LEAF_POLAR = dict(col=[None, None, None, 2, None, None], polar=[(4, (4, 6)), (0, (5, 0, 3))], ext_col=[1],
                  lo=[0.2, 0.0, 0.0, -1.0, 0.1, 0.0], hi=[1.0, math.pi, 2.0 * math.pi, 1.0, 0.9, 2.0 * math.pi])
GROUPS_P = dict(root_group=GROUPS3["root_group"], var_sets=[(0, 1, 2), (0, 1, 2, 3, 4, 5), ()])     # a polar group in a weight group whole


def leaf_polar_grid():
    rng = np.random.default_rng(31)
    g = capi.vegas_refine(vegas.uniform_grid(LEAF_POLAR["lo"], LEAF_POLAR["hi"], 6), rng.random((6, 6)) + 0.5, 1.0)
    assert np.array_equal(g[:, 0], LEAF_POLAR["lo"]) and np.array_equal(g[:, -1], LEAF_POLAR["hi"])
    return g


def polar_steps(B, gamma, disc):
    """INIT and four measured steps: everything, the 3D group, the 2D group (with the discrete variable), the lone variable"""
    d = (1 << 6) if disc else 0
    moves = [(0b111111 | d, INIT), (0b111111 | d, MEASURE), (0b000111, MEASURE), (0b110000 | d, MEASURE), (0b001000, MEASURE)]
    return [(mask, i * B + 17, 1.0 if flags == INIT else gamma, flags) for i, (mask, flags) in enumerate(moves)]


ENTRIES = ["plain", "matsubara", "grouped", "binned2", "binned7"]


def entry_args(entry, cin, cout, rng):
    """(cdf, ext, ext_col, groups, reweight, mz) of one of the step entries"""
    mz = ((2, -1, 0), True, 1, cin, cout, 1.7)
    if entry == "plain":
        return None, None, (), None, None, None
    if entry == "matsubara":
        return None, None, (), None, None, mz
    if entry == "grouped":
        return None, None, (), GROUPS_P, RHO3, None
    n_bin = int(entry[6:])
    return refined_cdf(rng, n_bin), rng.uniform(-1.0, 1.0, size=(n_bin, 1)), LEAF_POLAR["ext_col"], GROUPS_P, RHO3, (mz if n_bin == 7 else None)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("B", [1, 65])
def test_init_and_four_steps_match_the_mirror_bit_for_bit(libfdg, cuda, B, entry):
    """The random graph of tests/test_chain_accumulate.py (ten roots, one of which does not exist; seven leaves) with six variables: a
    3D group and a 2D group, listed out of variable order, and one variable of no group; through the plain step, the projected one
    (3 frequencies), the grouped one (three groups with rho) and the binned one (2 values; 7 values with groups and a projection)."""
    t, f, _, fixed, _, coef, exists, cin, cout = leaf_case(cuda)
    grid, col, polar = leaf_polar_grid(), LEAF_POLAR["col"], LEAF_POLAR["polar"]
    D, R, seed, gamma = 6, t.n_root, 11, 0.37
    cdf, ext, ext_col, groups, rho, mz = entry_args(entry, cin, cout, np.random.default_rng(3))
    n_bin = 0 if cdf is None else len(cdf) - 1
    chain = DeviceChainPolar(f.handle, cuda, grid, col, polar, fixed, B, cdf, ext, ext_col, groups, rho, mz, coef)
    m = fresh_state(fixed, D, R, B) if cdf is None else fresh_binned_state(fixed, D, R, B, n_bin, 3 if mz else 0)
    if cdf is None and mz is not None:
        m["sum"] = np.zeros((2 * 3 * R + 1, B))
    m = run_against_mirror(chain, m, grid, col, polar, polar_steps(B, gamma, cdf is not None), seed, oracle_roots(t), cdf, ext, ext_col, groups, rho,
                           mz, coef, exists, entry)
    assert (m["sum"][-1] > 0.0).all() and np.abs(m["sum"][:-1]).max() > 0.0
    assert B == 1 or 0 < (m["n_accept"] < 5).sum()
    assert_reduced(chain.reduced(), m["sum"], "reduced sums")


def test_walkers_over_several_chunks_and_from_two_shards(libfdg, cuda):
    """70 003 walkers with FDG_ROOT_SCRATCH_MB = 1 (several chunks, a short last one) against the mirror after every step, through the
    binned step with groups and rho; the same bits with the default scratch (one chunk), and from two shards."""
    B, seed, gamma, n_bin = 70_003, 12, 0.37, 3
    t, f1, _, fixed, _, coef, exists, cin, cout = leaf_case(cuda, options={"FDG_ROOT_SCRATCH_MB": "1"})
    f = fd.compile_table(t, specialize="isa")
    grid, col, polar, ext_col = leaf_polar_grid(), LEAF_POLAR["col"], LEAF_POLAR["polar"], LEAF_POLAR["ext_col"]
    D, R = 6, t.n_root
    rng = np.random.default_rng(n_bin)
    cdf, ext = refined_cdf(rng, n_bin), rng.uniform(-1.0, 1.0, size=(n_bin, 1))
    ev = oracle_roots(t)
    steps = polar_steps(B, gamma, True)

    def run(handle, n, lo, check):
        chain = DeviceChainPolar(handle, cuda, grid, col, polar, fixed, n, cdf, ext, ext_col, GROUPS_P, RHO3, None, coef, lo)
        if check:
            run_against_mirror(chain, fresh_binned_state(fixed, D, R, n, n_bin), grid, col, polar, steps, seed, ev, cdf, ext, ext_col, GROUPS_P, RHO3,
                               None, coef, exists, "chunks")
        else:
            for mask, off, g, flags in steps:
                chain.step(mask, g, seed, off + lo, flags)
        return chain.state(), chain.reduced()
    small, small_red = run(f1.handle, B, 0, True)
    whole, whole_red = run(f.handle, B, 0, False)
    for k in state_keys(True):
        assert_bits(whole[k], small[k], f"FDG_ROOT_SCRATCH_MB changed: {k}")
    assert_bits(whole_red, small_red, "reduced sums, FDG_ROOT_SCRATCH_MB changed")
    assert 0 < (small["n_accept"] < 5).sum() and np.abs(small["sum"]).max() > 0.0 and set(small["bin"]) == set(range(n_bin))
    cut = 30_001
    for lo, n in ((0, cut), (cut, B - cut)):
        part, _ = run(f1.handle, n, lo, False)
        for k in state_keys(True):
            assert_bits(part[k], small[k][..., lo:lo + n], f"shard at {lo}: {k}")


def test_monte_carlo_form_matches_the_mirror(mc_cases, cuda):
    """parquet_sigma2 in the Monte-Carlo form with its two loop momenta 3D groups over a ball: the plain step, and the binned step with
    the external momentum from a table of 7 values, the two roots in two groups (root 0: the momenta only; root 1: everything) and a
    projection; the mirror's roots are fdg_mc_eval_device's."""
    c = mc_cases["parquet_sigma2"]
    t, h, fixed = c["t"], c["f"].handle, c["fixed"]
    kF, beta, lam, nk = c["phys"]
    assert nk == 9 and c["col"] == [3, 4, 5, 6, 7, 8, 10]
    B, D, R, seed, n_bin = 1_229, 7, t.n_root, 21, 7
    col, polar = [None] * 6 + [10], [(3, (6, 7, 8)), (0, (3, 4, 5))]
    lo, hi = vegas.ball(2.0, 3)
    grid = capi.vegas_refine(vegas.uniform_grid(lo + lo + [0.0], hi + hi + [beta], 12), np.random.default_rng(2).random((D, 12)) + 0.05, 1.0)
    groups = dict(root_group=[0, 1], var_sets=[tuple(range(6)), tuple(range(7))])
    rng = np.random.default_rng(3)
    cdf, ext = refined_cdf(rng, n_bin), rng.uniform(-kF, kF, size=(n_bin, 3))
    ev = device_mc_roots(h, cuda, c["phys"], R)
    for what, args in (("plain", (None, None, (), None, None, None)),
                       ("binned", (cdf, ext, [0, 1, 2], groups, (2.5, 0.4), ((0, -1, 2), True, 2, c["cin"], c["cout"], beta)))):
        disc, mz = args[0] is not None, args[5]
        chain = DeviceChainPolar(h, cuda, grid, col, polar, fixed, B, *args)
        m = fresh_state(fixed, D, R, B) if not disc else fresh_binned_state(fixed, D, R, B, n_bin, 3)
        full = (1 << (D + disc)) - 1
        moves = [(full, INIT), (full, MEASURE), (0b0000111, MEASURE), (0b1111000 | ((1 << D) if disc else 0), MEASURE), (full, MEASURE)]
        gamma = 1.0
        for i, (mask, flags) in enumerate(moves):
            m = run_against_mirror(chain, m, grid, col, polar, [(mask, i * B + 17, gamma, flags)], seed, ev, *args[:5], mz, None, None,
                                   f"{what}, move {i}", mc=(kF, beta, lam))
            if flags == INIT:
                gamma = float(m["a"].mean())
                assert gamma > 0.0
        assert 0 < (m["n_accept"] < 5).sum() and np.abs(m["sum"][:-1]).max() > 0.0
        assert not disc or set(m["bin"]) == set(range(n_bin))


# ---- 5. the known answers through the driver ------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("dim", [2, 3])
def test_the_measure_through_the_driver(libfdg, cuda, dim):
    """tests/test_chain_polar_host.py's known answer at seed 0: r = 1 over a flat map on ball(2.5, dim) is the ball's volume, within 5
    reported sigma, and the mirror's mean.  The driver takes gamma from a torch sum over the 4096 walkers, the mirror from numpy's:
    either is within 4096 * 2^-53 = 5e-13 of the exact sum and the means depend smoothly on it, so they agree to 1e-10 and not to the
    bit.  The mirror alone: pulls -0.48 (2D) and -0.80 (3D) at seed 0, chi^2 over 32 seeds 27.2 and 27.6."""
    t, _, kcols, fixed = measure_graph(dim)
    k = KNOWN_M
    lo, hi = vegas.ball(k["k_max"], dim)
    res = vegas.chain_integrate_polar(fd.compile_table(t, specialize="isa"), None, lo, hi, [None] * dim, [vegas.PolarVar(0, kcols)],
                                      n_walker=k["n_walker"], n_step=k["n_step"], n_therm=k["n_therm"], gamma_rel=k["gamma_rel"], n_warm=0,
                                      n_grid=k["n_grid"], seed=0, fixed=fixed, device=cuda)
    mirror, exact = known_m_mirror(0, dim), ball_volume(k["k_max"], dim)
    print("device: mean", res.mean, "stderr", res.stderr, "acceptance", res.acceptance, "gamma", res.gamma)
    print("mirror: mean", mirror["mean"], "stderr", mirror["stderr"], "acceptance", mirror["acceptance"], "gamma", mirror["gamma"])
    assert res.mean.shape == res.stderr.shape == (1,)
    assert abs(res.mean[0] - exact) <= 5.0 * res.stderr[0]
    assert np.allclose(res.mean, mirror["mean"], rtol=1e-10, atol=0) and np.allclose(res.stderr, mirror["stderr"], rtol=1e-8, atol=0)
    assert math.isclose(res.gamma, mirror["gamma"], rel_tol=1e-12) and res.acceptance == mirror["acceptance"]
    assert np.array_equal(res.map.grid, vegas.uniform_grid(lo, hi, k["n_grid"]))       # no warm-up: the map is used as given


@pytest.mark.parametrize("qx", [0.0, 1.5])
def test_the_diagram_like_weight_through_the_driver(libfdg, cuda, qx):
    """8 pi lam^2 / (|K + q|^2 + lam) over |K| < 3, lam = 0.05, q = (qx, 0, 0), in the Monte-Carlo form: 2.104512 and 1.898826.  4096
    walkers, 40 steps with 8 discarded, a warm-up of 2 iterations of vegas_integrate(polar=...), which trains the map.  The mirror
    alone (a numpy formula for the leaf, the warm-up in numpy) lands -0.27 and -0.24 reported errors from the exact values."""
    k = KNOWN_W
    t, tab, _keep = leaf_on_k1_plus_k2(2)
    lo, hi = vegas.ball(k["k_max"], 3)
    res = vegas.chain_integrate_polar(fd.compile_table(t, specialize="isa"), tab, lo, hi, [None] * 3, [vegas.PolarVar(0, (3, 4, 5))], 0.0, 1.0,
                                      k["lam"], n_walker=k["n_walker"], n_step=k["n_step"], n_therm=k["n_therm"], n_warm=k["n_warm"],
                                      n_grid=k["n_grid"], seed=0, fixed=[qx, 0, 0, 0, 0, 0, 0], device=cuda)
    exact = ball_integral(qx, k["k_max"], k["lam"])
    print("mean", res.mean, "stderr", res.stderr, "exact", exact, "pull", (res.mean[0] - exact) / res.stderr[0], "acceptance", res.acceptance,
          "gamma", res.gamma)
    assert res.mean.shape == res.stderr.shape == (1,)
    assert res.stderr[0] > 0 and abs(res.mean[0] - exact) <= 5.0 * res.stderr[0]
    g = res.map.grid
    assert (np.diff(g, axis=1) > 0).all() and not np.array_equal(g, vegas.uniform_grid(lo, hi, k["n_grid"]))   # the warm-up changed the map
    assert np.array_equal(g[:, 0], lo) and np.array_equal(g[:, -1], hi)


def test_the_diagram_like_weight_per_bin_through_the_driver(libfdg, cuda):
    """... with K_1 = q_j = (0.4 j, 0, 0), j < 8, from the discrete variable's table: every bin within 5 reported errors of its closed
    form (j = 0) or quadrature value; the warm-up is vegas_integrate_binned(polar=...), which trains the map and the probabilities.
    The mirror alone lands within 1.42 reported errors in every bin."""
    k = KNOWN_W
    t, tab, _keep = leaf_on_k1_plus_k2(2)
    q = known_w_qtab()
    dm = vegas.DiscreteMap(vegas.uniform_cdf(k["n_bin"]), ext=q, ext_col=[0, 1, 2], device=cuda)
    lo, hi = vegas.ball(k["k_max"], 3)
    res = vegas.chain_integrate_polar(fd.compile_table(t, specialize="isa"), tab, lo, hi, [None] * 3, [vegas.PolarVar(0, (3, 4, 5))], 0.0, 1.0,
                                      k["lam"], n_walker=k["n_walker"], n_step=k["n_step"], n_therm=k["n_therm"], n_warm=k["n_warm"],
                                      n_grid=k["n_grid"], seed=0, dmap=dm, device=cuda)
    exact = np.array([ball_integral(float(v), k["k_max"], k["lam"]) for v in q[:, 0]])
    print("mean", res.mean[:, 0], "stderr", res.stderr[:, 0], "exact", exact, "pull", (res.mean[:, 0] - exact) / res.stderr[:, 0],
          "acceptance", res.acceptance, "gamma", res.gamma, "p", dm.prob)
    assert res.mean.shape == res.stderr.shape == (k["n_bin"], 1)
    assert (res.stderr[:, 0] > 0).all() and (np.abs(res.mean[:, 0] - exact) <= 5.0 * res.stderr[:, 0]).all()
    assert not np.array_equal(res.map.grid, vegas.uniform_grid(lo, hi, k["n_grid"])) and not np.array_equal(dm.cdf, vegas.uniform_cdf(k["n_bin"]))
