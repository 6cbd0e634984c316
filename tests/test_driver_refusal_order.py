"""The ORDER of the drivers' refusals (feynmandiagram.jl_amd/vegas.py): every call below violates two conditions at once, and the
message that wins is pinned.  The three driver bodies share their set-up helpers; each helper is called where its checks always stood
in that driver, and this file holds them there.  Two differences between the drivers are pinned as they are: ``vegas_integrate`` and
``vegas_integrate_binned`` leave FDG_WEIGHT_GROUP_MAX to the library while the others check it, and the ``ext_col`` message ends
"that col does not" in the direct driver and "that col does not name" in the chain.  Nothing here touches a device."""
import math

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd  # noqa: F401
from feynmandiagram_jl_amd import capi, vegas, workloads

P, WG = vegas.PolarVar, vegas.WeightGroups
LO3, HI3 = vegas.ball(2.0, 3)
BAD_THETA = [2.0, math.pi + 1e-9, 2 * math.pi]              # theta beyond pi: a refusal of the polar groups
POLAR = [P(0, (0, 1, 2))]
NINE = WG((0, 0), ((0,),) * 9)                              # more than FDG_WEIGHT_GROUP_MAX groups, sound otherwise
DIRECT = dict(n_iter=1, n_sample=100, n_grid=8, device="cpu", specialize_fused=False)
CHAIN = dict(n_walker=64, n_step=4, n_therm=1, n_warm=0, device="cpu")


@pytest.fixture(scope="module")
def graph():
    """sigma2 (8 leaves, 2 roots) and leaf tables of 2 loops in 3 dimensions and 2 times: 8 columns in either form"""
    h = capi.GraphHandle(workloads.get("sigma2"))
    assert (h.table.n_leaf, h.table.n_root, capi.FDG_WEIGHT_GROUP_MAX, capi.FDG_CHAIN_BIN_MAX) == (8, 2, 8, 64)
    tab, keep = capi.make_leaf_tables([2] * 8, [0] * 8, [1] * 8, [2] * 8, [1] * 8, np.ones((1, 2)), 3, 2)
    return h, tab, keep


def dmap(ext_col, n_bin=3):
    return vegas.DiscreteMap(vegas.uniform_cdf(n_bin), np.zeros((n_bin, 1)), [ext_col], device="cpu")


def map3():
    return vegas.VegasMap(vegas.uniform_grid([0.0] * 3, [1.0] * 3, 8), "cpu")


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_vegas_integrate(graph):
    h, tab, _ = graph
    box = (h, tab, [0.0, 0.0], [1.0, 1.0])
    ball = (h, tab, LO3 + [0.0], BAD_THETA + [1.0], [None, None, None, 3])
    run = vegas.vegas_integrate
    refused("distinct columns", run, *box, [0, 0], fixed=[0.0], **DIRECT)                                   # col, fixed
    refused("freq_observables needs matsubara", run, *box, [0, 0], freq_observables=vegas.FrequencyObservables(((1.0, 1.0),)), **DIRECT)
    refused("one column per variable", run, *box[:2], None, None, [0, 1], vmap=map3(), fixed=[0.0], **DIRECT)     # the map, fixed
    refused("theta of a polar group", run, *ball, polar=POLAR, groups=WG((0,), ((0,),)), **DIRECT)          # polar, groups
    refused("without a column", run, h, tab, LO3 + [0.0], HI3 + [1.0], [None] * 4, polar=POLAR, groups=WG((0,), ((0,),)), **DIRECT)
    refused("var_sets names variables", run, *box, [0, 1], groups=WG((0, 0), ((2,),)), **dict(DIRECT, n_discard=1))
    refused("observables.coef", run, *box, [0, 1], observables=vegas.Observables(((1.0,),)), **dict(DIRECT, n_sample=0))
    refused("n_discard < n_iter", run, *box, [0, 1], fixed=[0.0], **dict(DIRECT, n_discard=1))              # the counts, fixed
    # this driver leaves the number of groups to the library: nine of them get as far as ``fixed``
    refused("fixed must hold 8", run, *box, [0, 1], groups=NINE, fixed=[0.0], **DIRECT)
    # with ``strat``: the stratified driver's order
    s = vegas.Stratification((2, 2))
    refused("cannot be combined", run, *box, [0, 0], strat=s, polar=POLAR, **DIRECT)
    refused("distinct columns", run, *box, [0, 0], strat=vegas.Stratification((2,)), **DIRECT)             # col, strat.strat
    refused("strat.strat holds one count", run, *box, [0, 1], strat=vegas.Stratification((2,)), fixed=[0.0], **DIRECT)


def test_vegas_integrate_binned(graph):
    h, tab, _ = graph
    box = (h, tab, [0.0, 0.0], [1.0, 1.0])
    run = vegas.vegas_integrate_binned
    refused("strat cannot be combined", run, *box, [0, 0], dmap(0), strat=vegas.Stratification((2, 2)), **DIRECT)
    refused("distinct columns", run, *box, [0, 0], dmap(0), **DIRECT)                                       # col, ext_col
    refused(r"\[0, 8\) that col does not$", run, *box[:2], None, None, [0, 1], dmap(1), vmap=map3(), **DIRECT)   # ext_col, the map
    refused(r"\[0, 8\) that col does not$", run, *box, [0, 1], dmap(8), fixed=[0.0], **DIRECT)              # (outside x), fixed
    refused("one column per variable", run, *box[:2], None, None, [0, 1], dmap(2), vmap=map3(), groups=WG((0,), ((0,),)), **DIRECT)
    refused("theta of a polar group", run, h, tab, LO3 + [0.0], BAD_THETA + [1.0], [None, None, None, 3], dmap(4), polar=POLAR,
            groups=WG((0,), ((0,),)), **DIRECT)
    refused("root_group names one group", run, *box, [0, 1], dmap(2), groups=WG((0,), ((0,),)), fixed=[0.0], **DIRECT)
    refused("fixed must hold 8", run, *box, [0, 1], dmap(2), groups=NINE, fixed=[0.0], **DIRECT)            # no limit on this side here either


def test_vegas_integrate_stratified(graph):
    h, _, _ = graph
    box = (h, None, [0.0, 0.0], [1.0, 1.0])
    s = vegas.Stratification((2, 2))
    run = vegas.vegas_integrate_stratified
    refused("needs a Stratification", run, *box, [0, 0], None, **DIRECT)
    refused("distinct columns", run, *box, [0, 0], s, fixed=[0.0], **DIRECT)
    refused("one column per variable", run, *box[:2], None, None, [0, 1], s, vmap=map3(), groups=WG((0,), ((0,),)), **DIRECT)
    refused("theta of a polar group", run, h, None, LO3 + [0.0], BAD_THETA + [1.0], [None, None, None, 3], vegas.Stratification((1,) * 4),
            polar=POLAR, groups=WG((0,), ((0,),)), **DIRECT)
    refused("root_group names one group", run, *box, [0, 1], s, groups=WG((0,), ((0,),) * 9), **DIRECT)
    refused("need 1 .. 8 weight groups", run, *box, [0, 1], vegas.Stratification((2,)), groups=NINE, **DIRECT)   # the limit, strat.strat
    refused("var_sets names variables", run, *box, [0, 1], vegas.Stratification((2,)), groups=WG((0, 0), ((2,),)), **DIRECT)
    refused("strat.strat holds one count", run, *box, [0, 1], vegas.Stratification((2,), beta=2.0), **DIRECT)
    refused("strat.beta", run, *box, [0, 1], vegas.Stratification((2, 2), beta=2.0), fixed=[0.0], **DIRECT)
    refused("alloc_cols names", run, *box, [0, 1], s, alloc_cols=[9], fixed=[0.0], **DIRECT)
    refused("belongs to a weight group whole", run, h, None, LO3 + [0.0], HI3 + [1.0], [None, None, None, 3], vegas.Stratification((1,) * 3),
            polar=POLAR, groups=WG((0, 0), ((0, 3),)), **DIRECT)


def test_chain_integrate(graph):
    h, tab, _ = graph
    box = (h, None, [0.0, 0.0], [1.0, 1.0])
    mz = vegas.MatsubaraProjection((0, 1), True, (1, 1), (2, 2))
    run = vegas.chain_integrate
    refused("groups cannot be combined", run, *box, [0, 0], groups=NINE, **CHAIN)
    refused("distinct columns", run, *box, [0, 0], fixed=[0.0], **CHAIN)
    refused("distinct columns", run, *box, [0, 0], matsubara=mz, weight_freq=2, **CHAIN)                    # col, the projection
    refused("weight_freq must be an index", run, *box, [0, 1], matsubara=mz, weight_freq=2, **dict(CHAIN, n_therm=4))
    refused("0 <= n_therm < n_step", run, *box, [0, 1], gamma=-1.0, **dict(CHAIN, n_therm=4))               # n_step, gamma
    refused("gamma must be finite", run, *box[:2], None, None, [0, 1], vmap=map3(), gamma=-1.0, **CHAIN)    # gamma, the map
    refused("gamma_rel must be finite", run, *box, [0, 1], gamma_rel=0.0, moves=[4], **CHAIN)
    refused("one column per variable", run, *box[:2], None, None, [0, 1], vmap=map3(), moves=[8], **CHAIN)  # the map, moves
    refused("moves holds masks over the variables of the map$", run, *box, [0, 1], moves=[4], fixed=[0.0], **CHAIN)
    refused("fixed must hold 8", run, h, tab, *box[2:], [0, 1], fixed=[0.0], coef=[1.0], **CHAIN)


def test_chain_integrate_grouped(graph):
    h, _, _ = graph
    box = (h, None, [0.0, 0.0], [1.0, 1.0])
    run = vegas.chain_integrate_grouped
    refused("groups must be a WeightGroups", run, *box, [0, 0], object(), **CHAIN)
    refused("distinct columns", run, *box, [0, 0], NINE, **CHAIN)
    refused("0 <= n_therm < n_step", run, *box, [0, 1], WG((0,), ((0,),)), **dict(CHAIN, n_therm=4))        # n_step, groups
    refused("fixed must hold 8", run, *box, [0, 1], NINE, fixed=[0.0], **CHAIN)                             # fixed stands before the groups here
    refused("need 1 .. 8 weight groups", run, *box, [0, 1], NINE, reweight=[-1.0], **CHAIN)                 # the limit, reweight
    refused("root_group names one group", run, *box, [0, 1], WG((0,), ((0,),) * 9), **CHAIN)
    refused("var_sets names variables", run, *box, [0, 1], WG((0, 0), ((2,),)), coef=[1.0], **CHAIN)
    refused("coef must hold n_root = 2", run, *box, [0, 1], WG((0, 0), ((0,),)), coef=[1.0], reweight=[-1.0], **CHAIN)
    refused("reweight must hold one finite factor", run, *box, [0, 1], WG((0, 0), ((0,),)), reweight=[-1.0], **CHAIN)


def test_chain_integrate_binned(graph):
    h, _, _ = graph
    box = (h, None, [0.0, 0.0], [1.0, 1.0])
    run = vegas.chain_integrate_binned
    refused("dmap must be a DiscreteMap", run, *box, [0, 0], object(), **CHAIN)
    refused("reweight goes with groups", run, *box, [0, 0], dmap(0), reweight=[1.0], **CHAIN)
    refused("distinct columns", run, *box, [0, 0], dmap(0), **CHAIN)
    refused("at most 64 values", run, *box, [0, 1], dmap(1, n_bin=65), **CHAIN)                             # n_bin, ext_col
    refused(r"\[0, 8\) that col does not name$", run, *box[:2], None, None, [0, 1], dmap(1), vmap=map3(), **CHAIN)   # ext_col, the map
    refused(r"\[0, 8\) that col does not name$", run, *box, [0, 1], dmap(8), **dict(CHAIN, n_warm=1))       # (outside x), the warm-up
    refused("no warm-up with a discrete variable", run, *box, [0, 1], dmap(2), **dict(CHAIN, n_warm=1, n_therm=4))
    refused("0 <= n_therm < n_step", run, *box[:2], None, None, [0, 1], dmap(2), vmap=map3(), **dict(CHAIN, n_therm=4))
    refused("masks over the variables of the map and the discrete variable$", run, *box, [0, 1], dmap(2), moves=[8], fixed=[0.0], **CHAIN)
    refused("need 1 .. 8 weight groups", run, *box, [0, 1], dmap(2), groups=NINE, reweight=[-1.0], **CHAIN)


def test_chain_integrate_polar(graph):
    h, _, _ = graph
    ball = (h, None, LO3 + [0.0], HI3 + [1.0], [None, None, None, 3])
    run = vegas.chain_integrate_polar
    refused("polar must be a sequence of PolarVar", run, *ball[:4], [0, 0, 0, 0], [(0, (0, 1, 2))], **CHAIN)
    refused("distinct columns", run, *ball[:4], [None, None, None, 2], POLAR, fixed=[0.0], **CHAIN)
    refused(r"that col does not name$", run, h, None, LO3 + [0.0], BAD_THETA + [1.0], ball[4], POLAR, dmap=dmap(1), **CHAIN)   # ext_col, polar
    refused("theta of a polar group", run, h, None, LO3 + [0.0], BAD_THETA + [1.0], ball[4], POLAR, groups=WG((0,), ((0,),)), **CHAIN)
    refused("without a column", run, *ball[:4], [None] * 4, POLAR, moves=[1], **CHAIN)
    refused("redraws a polar group whole or not at all", run, *ball, POLAR, moves=[1], fixed=[0.0], **CHAIN)
    refused("fixed must hold 8", run, *ball, POLAR, fixed=[0.0], groups=WG((0, 0), ((0, 3),)), **CHAIN)
    refused("belongs to a weight group whole", run, *ball, POLAR, groups=WG((0, 0), ((0, 3),)), reweight=[-1.0], **CHAIN)
    refused("need 1 .. 8 weight groups", run, *ball, POLAR, groups=WG((0, 0), ((0, 3),) * 9), **CHAIN)     # the limit, a split polar group


def test_chain_integrate_shift(graph):
    h, _, _ = graph
    box = (h, None, [0.0, 0.0], [1.0, 1.0], [0, 1])
    S = vegas.ChainShift
    run = vegas.chain_integrate_shift
    refused("shift must be a ChainShift", run, *box[:4], [0, 0], object(), **CHAIN)
    refused("distinct columns", run, *box[:4], [0, 0], S(width=0.7), **CHAIN)
    refused("shift.width holds one half width", run, *box, S(width=0.7, moves=[(1, 1)]), **CHAIN)           # the width, overlapping masks
    refused("shift.target must lie", run, *box, S(tune=True, target=1.0, moves=[(1, 1)]), **CHAIN)
    refused("its two masks overlap", run, *box, S(moves=[(1, 1)]), fixed=[0.0], **CHAIN)                    # the masks, fixed
    refused("pairs of masks over the variables", run, *box, S(moves=[(1, 5)]), **CHAIN)                     # outside the map, overlapping
    refused("the discrete variable can only be redrawn", run, *box, S(moves=[(0, 4)]), dmap=dmap(2), fixed=[0.0], **CHAIN)
    refused("0 <= n_therm < n_step", run, *box, S(moves=[(1, 1)]), **dict(CHAIN, n_therm=4))                # n_step, the masks
    refused("one column per variable", run, *box[:2], None, None, [0, 1], S(width=0.7), vmap=map3(), **CHAIN)     # the map, the width
    refused("can only be redrawn with its group", run, h, None, LO3 + [0.0], HI3 + [1.0], [None, None, None, 3], S(moves=[(0, 2)]),
            polar=POLAR, fixed=[0.0], **CHAIN)
    refused("need 1 .. 8 weight groups", run, *box, S(), groups=NINE, reweight=[-1.0], **CHAIN)
