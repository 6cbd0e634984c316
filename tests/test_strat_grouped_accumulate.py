"""Stratified sampling for spherical momenta and weight groups on the device (include/fdg.h: fdg_vegas_sample_device_strat_grouped,
fdg_accumulate_device_strat_grouped, fdg_mc_accumulate_device_strat_grouped; feynmandiagram.jl_amd/vegas.py:
vegas_integrate_stratified).  The identities of the header hold bit for bit; the sampler is compared bit for bit with
capi.strat_grouped_reference; the per-hypercube moments with exact sums (math.fsum) of the oracle's roots, |d| <= 1e-12 sum |term| per
(hypercube, column); the driver against the exact integral of a peak inside the unit disc, with the conditions the CPU mirror of
tests/test_strat_grouped_host.py meets."""
import math
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas, workloads
from feynmandiagram_jl_amd.lowering import lower
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT
from test_strat_accumulate import (GOLD, SAMPLER_COUNTS, assert_bits, assert_close, host_cube_sums, host_strat_hist, prefix, random_program,
                                   run_strat, sums_case, to_tiles)
from test_strat_grouped_host import (CALIB_POLAR, DISC_HI, DISC_LO, KNOWN_GROUPS, KNOWN_POLAR, PEAK, groups_case, mirror_known, peak,
                                     polar_case)

pytestmark = pytest.mark.gpu

PI = math.pi


# ---- helpers -------------------------------------------------------------------------------------------------------------------------- #
# six variables: (k, theta, phi) of a ball -> columns 5, 1, 3;  (k, phi) of a disc -> columns 0, 6;  one free variable -> column 2
POLAR6 = [(0, (5, 1, 3)), (3, (0, 6))]
COL6 = [None, None, None, None, None, 2]
NCOL6 = 8                                               # columns 4 and 7 belong to nobody
SETS6 = ((0, 1, 2, 3, 4, 5), (0, 1, 2), (3, 4, 5))      # all; the dim-3 group only; the dim-2 group and the free variable


def polar_grid(rng, G):
    """a refined map over POLAR6's variables: the end edges stay at the box, so the angles stay in their domains"""
    lo = [0.25, 0.0, 0.0, 0.0, 0.0, -1.0]
    hi = [2.0, PI, 2.0 * PI, 1.5, 2.0 * PI, 2.0]
    g = capi.vegas_refine(vegas.uniform_grid(lo, hi, G), rng.random((6, G)) ** 3 + 1e-3, 1.0)
    assert g[1, -1] <= PI and g[2, -1] <= 2.0 * PI and g[4, -1] <= 2.0 * PI and (g[:, 0] == lo).all()
    return g


class Sampled:
    def __init__(self, cuda, n_col, n_jac, D, B):
        import torch
        self.x = torch.full((n_col, B), -77.0, dtype=torch.float64, device=cuda)
        self.jac = torch.full((n_jac, B), -5.0, dtype=torch.float64, device=cuda)
        self.cube = torch.full((B,), -1, dtype=torch.int32, device=cuda)
        self.cell = torch.full((D, B), -1, dtype=torch.int32, device=cuda)

    def host(self):
        return self.x.cpu().numpy(), self.jac.cpu().numpy(), self.cube.cpu().numpy(), self.cell.cpu().numpy()


def sample_sg(cuda, d_grid, D, G, col, polar, sets, strat, d_start, seed, off, B, n_col, into=None, at=0, total=None):
    """fdg_vegas_sample_device_strat_grouped into fresh arrays (or at sample `at` of given ones of `total` samples)"""
    import torch
    total = B if total is None else total
    s = into if into is not None else Sampled(cuda, n_col, 1 if sets is None else len(sets), D, total)
    capi.vegas_sample_device_strat_grouped(d_grid.data_ptr(), D, G, col, polar, sets, total, strat, d_start.data_ptr(), seed, off,
                                           s.x.data_ptr() + 8 * at, 1, total, s.jac.data_ptr() + 8 * at, s.cube.data_ptr() + 4 * at,
                                           s.cell.data_ptr() + 4 * at if total == B else 0, B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return s


def run_sg(f, cuda, leaf, strides, w, coef, seed, off, D, G, strat, cube, H, B, root_group, sets, into=None, poison=()):
    """fdg_accumulate_device_strat_grouped on fresh (or given) output arrays: (acc, acc2, hist, cube_sum, cube_sum2) as device tensors;
    w [n_group, stride]; the columns `poison` of fresh per-hypercube arrays start at -77"""
    import torch
    R, NG = f.handle.table.n_root, len(sets)
    if into is None:
        into = (torch.zeros(R, dtype=torch.float64, device=cuda), torch.zeros(R, dtype=torch.float64, device=cuda),
                torch.zeros((D, G), dtype=torch.float64, device=cuda), torch.zeros((H, R + NG), dtype=torch.float64, device=cuda),
                torch.zeros((H, R + NG), dtype=torch.float64, device=cuda))
        for c in poison:
            into[3][:, c], into[4][:, c] = -77.0, -77.0
    acc, acc2, hist, cs, cs2 = into
    wg, _keep = capi.make_weight_groups(root_group, sets, w.stride(0))
    f.handle.accumulate_device_strat_grouped(leaf.data_ptr(), *strides, w.data_ptr(), coef, seed, off, D, G, acc.data_ptr(), acc2.data_ptr(),
                                             hist.data_ptr(), strat, cube.data_ptr(), cs.data_ptr(), cs2.data_ptr(), wg, B,
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return acc, acc2, hist, cs, cs2


def host_grouped(roots, cube, H, strat, w, coef, live, root_group, sets, seed, off, G):
    """(sum, sum2, sum |t|) [H, R + NG] and the training histogram [D, G] of the grouped stratified call, from the ungrouped helpers
    group by group: the columns of a group's roots and its combination under its own weight, a variable's histogram over its owners"""
    R, NG, D = roots.shape[1], len(sets), len(strat)
    s1, s2, sa = np.zeros((H, R + NG)), np.zeros((H, R + NG)), np.zeros((H, R + NG))
    hist = np.zeros((D, G))
    for g in range(NG):
        mine = [k for k in live if root_group[k] == g]
        if not mine:
            continue
        a1, a2, aa = host_cube_sums(roots, cube, H, w[g], coef, mine)
        for k in mine:
            s1[:, k], s2[:, k], sa[:, k] = a1[:, k], a2[:, k], aa[:, k]
        s1[:, R + g], s2[:, R + g], sa[:, R + g] = a1[:, R], a2[:, R], aa[:, R]
        hg = host_strat_hist(roots, cube, H, strat, w[g], coef, mine, seed, off, G)
        for d in sets[g]:
            hist[d] += hg[d]
    return s1, s2, sa, hist


def check_grouped(got, roots, cube, H, strat, w, coef, live, root_group, sets, seed, off, G, untouched, what):
    s1, s2, sa, want = host_grouped(roots, cube.astype(np.int64), H, strat, w, coef, live, root_group, sets, seed, off, G)
    cs, cs2, hist = got[3].cpu().numpy(), got[4].cpu().numpy(), got[2].cpu().numpy()
    keep = [c for c in range(cs.shape[1]) if c not in untouched]
    assert np.isfinite(cs).all() and np.isfinite(cs2).all() and np.isfinite(hist).all(), what
    assert_close(cs[:, keep], s1[:, keep], sa[:, keep], (what, "cube_sum"))
    assert_close(cs2[:, keep], s2[:, keep], s2[:, keep], (what, "cube_sum2"))
    for c in untouched:                                                     # a missing root, a group without a root: the poison stays
        assert (cs[:, c] == -77.0).all() and (cs2[:, c] == -77.0).all(), (what, c)
    assert_close(hist, want, want, (what, "hist"))


# ---- 1. the sampler's identities ------------------------------------------------------------------------------------------------------ #
def test_sampler_identities(libfdg, cuda):
    import torch
    B, D, G, seed, off = 1000, 6, 8, 21, 300
    rng = np.random.default_rng(31)
    d_grid = torch.from_numpy(polar_grid(rng, G)).to(cuda)
    st = torch.cuda.current_stream().cuda_stream
    # no polar group and no weight group: the stratified sampler
    strat = (2, 1, 3, 1, 2, 1)
    start = prefix([40, 130, 2, 400, 3, 129, 64, 1, 200, 31, 250, 50])
    assert start[-1] == off + B
    d_start = torch.from_numpy(start).to(cuda)
    col = [3, 0, 5, 1, 4, 2]
    got = sample_sg(cuda, d_grid, D, G, col, (), None, strat, d_start, seed, off, B, 6)
    ref = Sampled(cuda, 6, 1, D, B)
    capi.vegas_sample_device_strat(d_grid.data_ptr(), D, G, col, strat, d_start.data_ptr(), seed, off, ref.x.data_ptr(), 1, B,
                                   ref.jac.data_ptr(), ref.cube.data_ptr(), ref.cell.data_ptr(), B, st)
    torch.cuda.synchronize()
    for a, b, what in zip(got.host(), ref.host(), ("x", "jac", "cube", "cell")):
        assert_bits(a, b, "no polar, no groups: " + what)
    assert len(set(got.host()[2].tolist())) == 9                            # (the batch starts behind hypercube 0)
    # one stratum per variable: the grouped sampler and the polar sampler without a discrete variable
    ones, whole = (1,) * D, torch.from_numpy(prefix([off + B])).to(cuda)
    got = sample_sg(cuda, d_grid, D, G, COL6, POLAR6, SETS6, ones, whole, seed, off, B, NCOL6)
    ref = Sampled(cuda, NCOL6, 3, D, B)
    capi.vegas_sample_device_grouped(d_grid.data_ptr(), D, G, COL6, 0, 1, 0, 0, None, POLAR6, SETS6, B, seed, off, ref.x.data_ptr(), 1, B,
                                     ref.jac.data_ptr(), 0, ref.cell.data_ptr(), B, st)
    torch.cuda.synchronize()
    for a, b, what in zip(got.host(), ref.host(), ("x", "jac", None, "cell")):
        if what:
            assert_bits(a, b, "one stratum, groups: " + what)
    assert (got.host()[2] == 0).all()
    got = sample_sg(cuda, d_grid, D, G, COL6, POLAR6, None, ones, whole, seed, off, B, NCOL6)
    ref = Sampled(cuda, NCOL6, 1, D, B)
    capi.vegas_sample_device_polar(d_grid.data_ptr(), D, G, COL6, 0, 1, 0, 0, None, POLAR6, seed, off, ref.x.data_ptr(), 1, B,
                                   ref.jac.data_ptr(), 0, ref.cell.data_ptr(), B, st)
    torch.cuda.synchronize()
    for a, b, what in zip(got.host(), ref.host(), ("x", "jac", None, "cell")):
        if what:
            assert_bits(a, b, "one stratum, polar: " + what)


# ---- 2. the sampler against the numpy restatement --------------------------------------------------------------------------------------- #
def test_sampler_matches_the_numpy_restatement_bit_for_bit(libfdg, cuda):
    import torch
    D, G, strat, seed = 6, 37, (2, 1, 3, 1, 2, 1), 0xFEDCBA
    rng = np.random.default_rng(32)
    grid = polar_grid(rng, G)
    counts = SAMPLER_COUNTS * 2
    assert SAMPLER_COUNTS == [1, 70, 2, 300, 3, 129] and len(counts) == int(np.prod(strat))
    start = prefix(counts)
    B = int(start[-1])
    want = capi.strat_grouped_reference(grid, strat, start, oracle.philox_uniform(B, D, seed, 0), COL6, POLAR6, SETS6, NCOL6, fill=-77.0)
    assert np.array_equal(np.bincount(want["cube"]), counts)
    d_grid, d_start = torch.from_numpy(grid).to(cuda), torch.from_numpy(start).to(cuda)
    got = sample_sg(cuda, d_grid, D, G, COL6, POLAR6, SETS6, strat, d_start, seed, 0, B, NCOL6)
    hx, hj, hc, hcell = got.host()
    assert_bits(hx.T, want["x"], "x")                                       # (the columns of nobody keep their fill)
    assert_bits(hj, want["jac"], "jac")
    assert np.array_equal(hc, want["cube"]) and np.array_equal(hcell.T, want["cell"])
    # without groups: one jacobian, the full fold
    one = sample_sg(cuda, d_grid, D, G, COL6, POLAR6, None, strat, d_start, seed, 0, B, NCOL6)
    w1 = capi.strat_grouped_reference(grid, strat, start, oracle.philox_uniform(B, D, seed, 0), COL6, POLAR6, None, NCOL6, fill=-77.0)
    assert_bits(one.host()[0].T, want["x"], "x without groups")
    assert_bits(one.host()[1][0], w1["jac"], "jac without groups")
    assert_bits(w1["jac"], want["jac"][0], "the full mask is the ungrouped fold")
    # every Cartesian point lies inside the image of its stratum: the polar coordinates recovered from the columns
    x = want["x"]
    (v3, c3), (v2, c2) = POLAR6
    k3 = np.sqrt(x[:, c3[0]] ** 2 + x[:, c3[1]] ** 2 + x[:, c3[2]] ** 2)
    back = {0: k3, 1: np.arccos(np.clip(x[:, c3[2]] / k3, -1.0, 1.0)), 2: np.mod(np.arctan2(x[:, c3[1]], x[:, c3[0]]), 2.0 * PI),
            3: np.hypot(x[:, c2[0]], x[:, c2[1]]), 4: np.mod(np.arctan2(x[:, c2[1]], x[:, c2[0]]), 2.0 * PI), 5: x[:, COL6[5]]}

    def image(d, v):
        y = v * G
        c = np.minimum(y.astype(np.int64), G - 1)
        return grid[d, c] + (y - c) * (grid[d, c + 1] - grid[d, c])
    rem = want["cube"].astype(np.int64)
    for d in range(D):
        s_d, rem = rem % strat[d], rem // strat[d]
        lo, hi = image(d, s_d / strat[d]), image(d, (s_d + 1.0) / strat[d])
        slack = 1e-9                                                        # the way back through acos / atan2 near the poles
        if d in (2, 4):                                                     # (an angle at 2 pi comes back as 0)
            ok = ((back[d] >= lo - slack) & (back[d] <= hi + slack)) | ((back[d] + 2.0 * PI >= lo - slack) & (back[d] + 2.0 * PI <= hi + slack))
        else:
            ok = (back[d] >= lo - slack) & (back[d] <= hi + slack)
        assert ok.all(), (d, np.argwhere(~ok)[:4])
    # the weights integrate the constant 1 under every group: the volume of the group's own variables' domain
    vol = {0: 4.0 / 3.0 * PI * (2.0 ** 3 - 0.25 ** 3), 1: PI * 1.5 ** 2 * 3.0}
    assert abs(want["jac"][1].sum() / B / vol[0] - 1.0) < 0.25 and abs(want["jac"][2].sum() / B / vol[1] - 1.0) < 0.25
    # two shards with offsets are one call
    h = B // 2
    two = Sampled(cuda, NCOL6, 3, D, B)
    for off, n in ((0, h), (h, B - h)):
        sample_sg(cuda, d_grid, D, G, COL6, POLAR6, SETS6, strat, d_start, seed, off, n, NCOL6, into=two, at=off, total=B)
    assert_bits(two.host()[0].T, want["x"], "shards x")
    assert_bits(two.host()[1], want["jac"], "shards jac")
    assert np.array_equal(two.host()[2], want["cube"])


# ---- 3. the accumulate call's identities ------------------------------------------------------------------------------------------------ #
def test_accumulate_identities(libfdg, cuda):
    import torch
    B, D, G, seed, off = 1000, 3, 8, 5, 0
    t = random_program(21)
    R = t.n_root
    assert R == 10
    f = fd.compile_table(t, specialize="isa")
    rng = np.random.default_rng(33)
    leaf = torch.from_numpy(oracle.philox_uniform(B, t.n_leaf, 34) + 0.25).to(cuda)
    coef = rng.uniform(-1.0, 1.0, size=R)
    strides = (t.n_leaf, 1, 0)
    # one group that owns every variable: the stratified call, all five outputs
    strat, counts = (2, 3, 1), [100, 2, 333, 64, 1, 500]
    cube = torch.from_numpy(np.repeat(np.arange(6), counts).astype(np.int32)).to(cuda)
    w = torch.from_numpy(rng.uniform(-1.0, 2.0, size=(1, B))).to(cuda)
    got = run_sg(f, cuda, leaf, strides, w, coef, seed, off, D, G, strat, cube, 6, B, [0] * R, ((0, 1, 2),))
    ref = run_strat(f, cuda, leaf, strides, w[0], coef, seed, off, D, G, strat, cube, 6, B)
    for a, b, what in zip(got, ref, ("acc", "acc2", "hist", "cube_sum", "cube_sum2")):
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), "one full group: " + what)
    assert got[3].shape == (6, R + 1) and float(got[4].abs().sum()) > 0.0
    # three groups, one stratum per variable, every sample in hypercube 0: hist, acc and acc2 of the grouped call
    rg, sets = [k % 3 for k in range(R)], ((0, 1, 2), (1,), (0, 2))
    w3 = torch.from_numpy(rng.uniform(-1.0, 2.0, size=(3, B))).to(cuda)
    zero = torch.zeros(B, dtype=torch.int32, device=cuda)
    got = run_sg(f, cuda, leaf, strides, w3, coef, seed, off, D, G, (1, 1, 1), zero, 1, B, rg, sets)
    m = torch.zeros((2, R), dtype=torch.float64, device=cuda)
    hist = torch.zeros((D, G), dtype=torch.float64, device=cuda)
    wg, _keep = capi.make_weight_groups(rg, sets, B)
    f.handle.accumulate_device_grouped(leaf.data_ptr(), *strides, 0, 0, 1, w3.data_ptr(), wg, None, coef, seed, off, D, G, m[0].data_ptr(),
                                       m[1].data_ptr(), hist.data_ptr(), 0, B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_bits(got[0].cpu().numpy(), m[0].cpu().numpy(), "three groups: acc")
    assert_bits(got[1].cpu().numpy(), m[1].cpu().numpy(), "three groups: acc2")
    assert_bits(got[2].cpu().numpy(), hist.cpu().numpy(), "three groups: hist")
    assert float(hist.abs().sum()) > 0.0


# ---- 4.-6. the per-hypercube sums with groups -------------------------------------------------------------------------------------------- #
def grouped_case(seed, counts, n_bad, D):
    """sums_case with three weight groups: the missing root 3 is the only root of group 2, the others alternate between groups 0 and 1;
    13 columns, so two column groups of the per-hypercube pass.  The weights of the rootless group are poison."""
    t, B, H, cube, h_leaf, roots, w, coef, live = sums_case(seed, counts, n_bad)
    rg = [2 if k == 3 else k % 2 for k in range(t.n_root)]
    sets = ((0, 1), (1, 2), (0, 2)) if D == 3 else ((0,), (0, 1), (1,))
    rng = np.random.default_rng(seed + 1000)
    w3 = np.stack([w, rng.uniform(-1.0, 2.0, size=B), np.full(B, np.nan)])
    return t, B, H, cube, h_leaf, roots, w3, coef, live, rg, sets


def test_sums_with_groups_match_numpy_per_hypercube(libfdg, cuda):
    import torch
    counts = [1, 2, 3, 70, 300, 1, 64, 63, 65, 1500, 2, 256, 700, 5, 1, 1, 128, 1300, 40, 2]     # 20 hypercubes: strat (5, 2, 2)
    strat, D, G, seed, off = (5, 2, 2), 3, 16, 11, 0
    t, B, H, cube, h_leaf, roots, w3, coef, live, rg, sets = grouped_case(7, counts, 40, D)
    R = t.n_root
    assert B % 64 != 0 and R + 3 == 13
    f = fd.compile_table(t, specialize="isa")
    leaf = torch.from_numpy(to_tiles(h_leaf, np.nan)).to(cuda)              # tile-major: nan in the lanes past n_sample
    d_w, d_cube = torch.from_numpy(w3).to(cuda), torch.from_numpy(cube).to(cuda)
    strides = (1, 64, 64 * t.n_leaf)
    got = run_sg(f, cuda, leaf, strides, d_w, coef, seed, off, D, G, strat, d_cube, H, B, rg, sets, poison=(3, R + 2))
    check_grouped(got, roots, cube, H, strat, w3, coef, live, rg, sets, seed, off, G, (3, R + 2), "one chunk")
    again = run_sg(f, cuda, leaf, strides, d_w, coef, seed, off, D, G, strat, d_cube, H, B, rg, sets, poison=(3, R + 2))
    for a, b in zip(got, again):
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), "twice")
    # the moments are the grouped call's, whatever the hypercubes
    m = torch.zeros((2, R), dtype=torch.float64, device=cuda)
    wg, _keep = capi.make_weight_groups(rg, sets, B)
    f.handle.accumulate_device_grouped(leaf.data_ptr(), *strides, 0, 0, 1, d_w.data_ptr(), wg, None, None, 0, 0, 0, 0, m[0].data_ptr(),
                                       m[1].data_ptr(), 0, 0, B, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_bits(got[0].cpu().numpy(), m[0].cpu().numpy(), "acc")
    assert_bits(got[1].cpu().numpy(), m[1].cpu().numpy(), "acc2")


def test_sums_with_groups_over_chunks_and_segments(libfdg, cuda, fdgopt):
    """FDG_ROOT_SCRATCH_MB=1 and ten roots: four chunks of 13056 samples, training segments of 17 tiles; hypercubes straddle both kinds
    of boundary, one covers two whole chunks, and the last chunk is short."""
    import torch
    fdgopt.set("FDG_ROOT_SCRATCH_MB", "1")
    counts = [500, 900, 3000, 2, 9000, 1, 27000, 64, 1300, 11, 700, 2]
    strat, D, G, seed, off = (3, 4), 2, 24, 12, 0
    t, B, H, cube, h_leaf, roots, w3, coef, live, rg, sets = grouped_case(8, counts, 100, D)
    R = t.n_root
    Bc, seg = ((1 << 20) // (8 * R)) & ~63, 17 * 64
    start = prefix(counts)
    inside = lambda edge: bool(((start[:-1] < edge) & (edge < start[1:])).any())
    assert (B + Bc - 1) // Bc == 4 and B % Bc != 0 and inside(Bc) and inside(seg) and inside(Bc + seg)
    assert ((start[1:] - start[:-1]) > 2 * Bc).any()
    f = fd.compile_table(t, specialize="isa")
    assert f.handle.get_option("FDG_ROOT_SCRATCH_MB") == "1"
    leaf = torch.from_numpy(to_tiles(h_leaf, np.inf)).to(cuda)
    d_w, d_cube = torch.from_numpy(w3).to(cuda), torch.from_numpy(cube).to(cuda)
    strides = (1, 64, 64 * t.n_leaf)
    got = run_sg(f, cuda, leaf, strides, d_w, coef, seed, off, D, G, strat, d_cube, H, B, rg, sets, poison=(3, R + 2))
    check_grouped(got, roots, cube, H, strat, w3, coef, live, rg, sets, seed, off, G, (3, R + 2), "chunks")
    again = run_sg(f, cuda, leaf, strides, d_w, coef, seed, off, D, G, strat, d_cube, H, B, rg, sets, poison=(3, R + 2))
    for a, b in zip(got, again):
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), "twice")


def test_two_shards_with_groups_add_up_to_the_batch(libfdg, cuda):
    import torch
    counts = [300, 2, 1700, 64, 900, 1100]
    strat, D, G, seed = (2, 3), 2, 16, 13
    t, B, H, cube, h_leaf, roots, w3, coef, live, rg, sets = grouped_case(9, counts, 0, D)
    f = fd.compile_table(t, specialize="isa")
    leaf, d_w, d_cube = torch.from_numpy(h_leaf).to(cuda), torch.from_numpy(w3).to(cuda), torch.from_numpy(cube).to(cuda)
    whole = run_sg(f, cuda, leaf, (t.n_leaf, 1, 0), d_w, coef, seed, 0, D, G, strat, d_cube, H, B, rg, sets)
    parts = None
    half = B // 2
    assert cube[half - 1] == cube[half]                                     # the cut falls inside a hypercube
    for s, n in ((0, half), (half, B - half)):
        parts = run_sg(f, cuda, leaf[s:], (t.n_leaf, 1, 0), d_w[:, s:], coef, seed, s, D, G, strat, d_cube[s:], H, n, rg, sets, into=parts)
    s1, s2, sa, want = host_grouped(roots, cube.astype(np.int64), H, strat, w3, coef, live, rg, sets, seed, 0, G)
    assert_close(parts[3].cpu().numpy(), whole[3].cpu().numpy(), sa, "shards cube_sum")
    assert_close(parts[4].cpu().numpy(), whole[4].cpu().numpy(), s2, "shards cube_sum2")
    assert_close(parts[2].cpu().numpy(), whole[2].cpu().numpy(), want, "shards hist")
    assert (whole[3].cpu().numpy()[:, [3, t.n_root + 2]] == 0.0).all()
    keep = [c for c in range(t.n_root + 3) if c not in (3, t.n_root + 2)]
    assert_close(whole[3].cpu().numpy()[:, keep], s1[:, keep], sa[:, keep], "whole cube_sum")
    assert_close(whole[2].cpu().numpy(), want, want, "whole hist")


# ---- 7. both forms of the call on the GV tables -------------------------------------------------------------------------------------------- #
def test_leaf_and_mc_forms_on_gv_sigma4(libfdg, cuda):
    import torch
    z = dict(np.load(os.path.join(GOLD, "gv_sigma4_leafstates.npz")))
    t = workloads.get("gv_sigma4")
    R, B, dim, n_loop, n_tau = t.n_root, 4096, 3, int(z["basis"].shape[1]), int(z["n_tau"])
    kF, beta, lam = 1.919, 3.0, 1.2
    nk, C = n_loop * dim, n_loop * dim + n_tau
    # the external momentum and T[1] stay fixed; the first loop momentum is (k, theta, phi) of a ball, the others Cartesian
    col = [None] * dim + list(range(2 * dim, nk)) + list(range(nk + 1, C))
    polar = [(0, tuple(range(dim, 2 * dim)))]
    D, G, seed = len(col), 12, 78
    strat = tuple([2, 3] + [1] * (D - 3) + [2])
    H = 12
    rng = np.random.default_rng(15)
    lo = np.array([0.0, 0.0, 0.0] + [-2.0] * (nk - 2 * dim) + [0.0] * (n_tau - 1))
    hi = np.array([3.0, PI, 2.0 * PI] + [2.0] * (nk - 2 * dim) + [beta] * (n_tau - 1))
    grid = capi.vegas_refine(vegas.uniform_grid(lo, hi, G), rng.random((D, G)) + 0.05, 1.0)
    start = capi.strat_allocate(rng.random((H, 1)) * 50, rng.random((H, 1)) * 5000 + 2500, 0, capi.strat_allocate(None, None, 0, None, H, B),
                                H, B, 1.0)
    assert len(set(np.diff(start).tolist())) > 4
    times = tuple(range(D - (n_tau - 1), D))
    sets = (tuple(range(D)), (0, 1, 2) + times)                             # group 1 leaves the Cartesian momenta out
    live = [k for k in range(R) if int(t.root_slot[k]) != FDG_NO_ROOT]
    rg = [k % 2 for k in range(R)]
    d_grid, d_start = torch.from_numpy(grid).to(cuda), torch.from_numpy(start).to(cuda)
    fixed = np.zeros(C)
    fixed[0] = kF
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(fixed).to(cuda)[:, None].repeat(1, B).contiguous()
    jac = torch.zeros((2, B), dtype=torch.float64, device=cuda)
    cube = torch.zeros(B, dtype=torch.int32, device=cuda)
    capi.vegas_sample_device_strat_grouped(d_grid.data_ptr(), D, G, col, polar, sets, B, strat, d_start.data_ptr(), seed, 0, x.data_ptr(), 1, B,
                                           jac.data_ptr(), cube.data_ptr(), 0, B, st)
    torch.cuda.synchronize()
    want = capi.strat_grouped_reference(grid, strat, start, oracle.philox_uniform(B, D, seed, 0), col, polar, sets, C)
    written = [c for c in range(C) if c not in (0, 1, 2, nk)]
    assert_bits(x.cpu().numpy()[written].T, want["x"][:, written], "x")
    assert_bits(jac.cpu().numpy(), want["jac"], "jac")
    h_cube, h_jac = cube.cpu().numpy(), jac.cpu().numpy()
    assert np.array_equal(h_cube, want["cube"])
    tab, _keep = capi.make_leaf_tables(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau)
    f = fd.compile_table(t, specialize="isa")
    f.handle.specialize_fused(tab)
    dK, dT = x.data_ptr(), x.data_ptr() + 8 * nk * B
    root = torch.zeros((B, R), dtype=torch.float64, device=cuda)
    f.handle.mc_eval_device(dK, 1, B, dT, 1, B, kF, beta, lam, root.data_ptr(), R, 1, B, st)
    coef = rng.uniform(-1.0, 1.0, size=R)
    wg, _wkeep = capi.make_weight_groups(rg, sets, B)
    m = torch.zeros((2, 2, R), dtype=torch.float64, device=cuda)
    hist = torch.zeros((2, D, G), dtype=torch.float64, device=cuda)
    cs = torch.zeros((2, H, R + 2), dtype=torch.float64, device=cuda)
    f.handle.mc_accumulate_device_strat_grouped(dK, 1, B, dT, 1, B, kF, beta, lam, jac.data_ptr(), coef, seed, 0, D, G, m[0, 0].data_ptr(),
                                                m[0, 1].data_ptr(), hist[0].data_ptr(), strat, cube.data_ptr(), cs[0].data_ptr(),
                                                cs[1].data_ptr(), wg, B, st)
    f.handle.mc_accumulate_device_grouped(dK, 1, B, dT, 1, B, kF, beta, lam, 0, 0, 1, jac.data_ptr(), wg, None, coef, seed, 0, D, G,
                                          m[1, 0].data_ptr(), m[1, 1].data_ptr(), hist[1].data_ptr(), 0, B, st)
    torch.cuda.synchronize()
    assert_bits(m[0].cpu().numpy(), m[1].cpu().numpy(), "moments of the mc form")
    h_root = root.cpu().numpy()
    s1, s2, sa, want_h = host_grouped(h_root, h_cube.astype(np.int64), H, strat, h_jac, coef, live, rg, sets, seed, 0, G)
    assert_close(cs[0].cpu().numpy(), s1, sa, "mc cube_sum")
    assert_close(cs[1].cpu().numpy(), s2, s2, "mc cube_sum2")
    assert_close(hist[0].cpu().numpy(), want_h, want_h, "mc hist")
    assert not np.array_equal(hist[0].cpu().numpy(), hist[1].cpu().numpy())           # the plain formula puts the samples in other cells
    # the leaf form over the leaves of the same samples
    leaf = torch.ones((B, t.n_leaf), dtype=torch.float64, device=cuda)
    capi.leaf_eval_device(z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, n_tau, kF, beta, lam,
                          dK, 1, B, dT, 1, B, leaf.data_ptr(), t.n_leaf, 1, B, st)
    got = run_sg(f, cuda, leaf, (t.n_leaf, 1, 0), jac, coef, seed, 0, D, G, strat, cube, H, B, rg, sets)
    l_root = oracle.eval_static(t, leaf.cpu().numpy())
    l1, l2, la, want_l = host_grouped(l_root, h_cube.astype(np.int64), H, strat, h_jac, coef, live, rg, sets, seed, 0, G)
    assert_close(got[3].cpu().numpy(), l1, la, "leaf cube_sum")
    assert_close(got[4].cpu().numpy(), l2, l2, "leaf cube_sum2")
    assert_close(got[2].cpu().numpy(), want_l, want_l, "leaf hist")
    # ... and the two forms agree with each other
    assert_close(got[3].cpu().numpy(), cs[0].cpu().numpy(), sa, "leaf form against mc form: cube_sum")
    assert_close(got[4].cpu().numpy(), cs[1].cpu().numpy(), s2, "leaf form against mc form: cube_sum2")
    assert_close(got[2].cpu().numpy(), hist[0].cpu().numpy(), want_h, "leaf form against mc form: hist")


# ---- 8.-10. the driver ------------------------------------------------------------------------------------------------------------------- #
def peak_graph(n_k, s, a):
    """f(K) = 1 / ((Kx - s)^2 + Ky^2 + a^2) for n_k momenta over the leaves (K1x, K1y, ..., s, a^2), built like
    test_strat_accumulate.ridge_graph.  Roots: f(K1), and with two momenta also f(K1) f(K2).  (compiled function, the columns of every
    K, the fixed leaf values)"""
    ks = [(fd.Graph([]), fd.Graph([])) for _ in range(n_k)]
    sh, c = fd.Graph([]), fd.Graph([])

    def f_of(x, y):
        d = fd.Graph([x, sh], subgraph_factors=[1.0, -1.0], operator=fd.Sum())
        q = fd.Graph([fd.Graph([d], operator=fd.Power(2)), fd.Graph([y], operator=fd.Power(2)), c], subgraph_factors=[1.0, 1.0, 1.0],
                     operator=fd.Sum())
        return fd.Graph([q], operator=fd.Power(-1))
    fs = [f_of(x, y) for x, y in ks]
    roots = [fs[0]] if n_k == 1 else [fs[0], fd.Graph([fs[0], fs[1]], operator=fd.Prod())]
    t, leafmap, _ = lower(roots)
    at = {g.id: i - 1 for i, g in leafmap.items()}
    assert t.n_leaf == 2 * n_k + 2 and t.n_root == len(roots)
    fixed = np.zeros(t.n_leaf)
    fixed[at[sh.id]], fixed[at[c.id]] = s, a * a
    return fd.compile_table(t, specialize="isa"), [(at[x.id], at[y.id]) for x, y in ks], fixed


def test_known_answer_in_a_disc(libfdg, cuda):
    """f(X, Y) = 1 / ((X - 0.6)^2 + Y^2 + 0.05^2) over the unit disc, (k, phi) stratified 16 x 16: the exact integral is
    pi [ln(2 sqrt(Q(u)) + 2 u + 2 (a^2 - s^2))] from 0 to 1 = 17.43976.  The numpy mirror on the CPU (tests/test_strat_grouped_host.py, the
    same samples bit for bit) gives, over 5 iterations of 2e5 samples at seed 2025, 17.43740 +- 0.00410."""
    k = KNOWN_POLAR
    f, (xy,), fixed = peak_graph(1, **PEAK)
    _, exact = peak(**PEAK)
    kw = dict(n_iter=k["n_iter"], n_sample=k["n_sample"], n_grid=k["n_grid"], alpha=0.5, seed=k["seed"], fixed=fixed, device=cuda)
    res = vegas.vegas_integrate_stratified(f, None, DISC_LO, DISC_HI, [None, None], vegas.Stratification(k["S"]),
                                           polar=[vegas.PolarVar(0, xy)], **kw)
    its, counts, _ = mirror_known(polar_case(), k, n_iter=1)
    print("stratified", res.mean, res.stderr, "exact", exact, "pull", (res.mean[0] - exact) / res.stderr[0])
    print("iterations", res.iterations, "mirror iteration 0", its[0])
    assert abs(res.mean[0] - exact) < 5.0 * res.stderr[0] and res.stderr[0] > 0.0
    assert abs(res.iterations[0][0][0] / its[0][0][0] - 1.0) <= 1e-9 and abs(res.iterations[0][1][0] / its[0][1][0] - 1.0) <= 1e-9
    assert len(res.cube_counts) == k["n_iter"] and all(c.sum() == k["n_sample"] and c.min() >= 2 for c in res.cube_counts)
    assert np.array_equal(res.cube_counts[0], counts[0])
    # not a condition: what the strata add to the polar map alone on a peak, which the separable map can follow
    one = vegas.vegas_integrate_stratified(f, None, DISC_LO, DISC_HI, [None, None], vegas.Stratification((1, 1)),
                                           polar=[vegas.PolarVar(0, xy)], **kw)
    print("one stratum per variable", one.mean, one.stderr, "variance ratio", (res.stderr[0] / one.stderr[0]) ** 2)


def test_known_answer_with_two_groups(libfdg, cuda):
    """root 0 = f(K1) in a group that owns K1's variables only, root 1 = f(K1) f(K2) in a group that owns all four, 6^4 hypercubes:
    I and I^2.  Root 0 is what a group with the wrong fac_h or the wrong jacobian would miss.  The mirror gives
    17.42356 +- 0.01331 and 303.980 +- 0.245 against 17.43976 and 304.145."""
    k = KNOWN_GROUPS
    f, (k1, k2), fixed = peak_graph(2, **PEAK)
    _, exact = peak(**PEAK)
    groups = vegas.WeightGroups((0, 1), ((0, 1), (0, 1, 2, 3)))
    res = vegas.vegas_integrate_stratified(f, None, DISC_LO * 2, DISC_HI * 2, [None] * 4, vegas.Stratification(k["S"]),
                                           polar=[vegas.PolarVar(0, k1), vegas.PolarVar(2, k2)], groups=groups, n_iter=k["n_iter"],
                                           n_sample=k["n_sample"], n_grid=k["n_grid"], alpha=0.5, seed=k["seed"], fixed=fixed, device=cuda)
    want = np.array([exact, exact * exact])
    print("stratified", res.mean, res.stderr, "exact", want, "pull", (res.mean - want) / res.stderr)
    print("iterations", res.iterations)
    assert (np.abs(res.mean - want) < 5.0 * res.stderr).all() and (res.stderr > 0.0).all()
    assert all(c.sum() == k["n_sample"] and c.min() >= 2 and c.shape == (6 ** 4,) for c in res.cube_counts)


def test_error_bars_are_calibrated_over_32_seeds(libfdg, cuda):
    """sum over 32 seeds of ((I - exact) / sigma)^2 at 2e4 samples, one iteration each: chi^2 with 32 degrees of freedom, whose 0.1 %
    two-sided range is about [12, 60].  The CPU mirror gives 25.71."""
    c = CALIB_POLAR
    f, (xy,), fixed = peak_graph(1, **PEAK)
    _, exact = peak(**PEAK)
    chi2 = 0.0
    for seed in range(c["n_seed"]):
        res = vegas.vegas_integrate_stratified(f, None, DISC_LO, DISC_HI, [None, None], vegas.Stratification(c["S"]),
                                               polar=[vegas.PolarVar(0, xy)], n_iter=1, n_sample=c["n_sample"], n_grid=c["n_grid"],
                                               seed=seed, fixed=fixed, device=cuda)
        chi2 += ((res.mean[0] - exact) / res.stderr[0]) ** 2
    print("calibration chi2 over", c["n_seed"], "seeds:", chi2)
    assert 12.0 <= chi2 <= 60.0


def test_without_polar_and_groups_it_is_the_keyword(libfdg, cuda):
    """vegas_integrate_stratified(polar=None, groups=None) and vegas_integrate(strat=...) make the same calls: the same bits"""
    from test_strat_accumulate import ridge_graph
    f, col, fixed = ridge_graph(0.02)
    kw = dict(n_iter=3, n_sample=20_000, n_grid=32, seed=4, fixed=fixed, device=cuda)
    s = vegas.Stratification((8, 8))
    a = vegas.vegas_integrate(f, None, [0, 0], [1, 1], col, strat=s, **kw)
    b = vegas.vegas_integrate_stratified(f, None, [0, 0], [1, 1], col, s, **kw)
    assert_bits(a.mean, b.mean, "mean")
    assert_bits(a.stderr, b.stderr, "stderr")
    for (m1, e1), (m2, e2), h1, h2, c1, c2 in zip(a.iterations, b.iterations, a.histograms, b.histograms, a.cube_counts, b.cube_counts):
        assert_bits(m1, m2, "iteration mean")
        assert_bits(e1, e2, "iteration stderr")
        assert_bits(h1, h2, "histogram")
        assert np.array_equal(c1, c2)
