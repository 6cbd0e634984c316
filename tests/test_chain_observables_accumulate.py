"""Observables of the Markov chain on the device (include/fdg.h: fdg_chain_reduce_device_observables; feynmandiagram.jl_amd/vegas.py:
chain_integrate_observables).  The entry is compared BIT FOR BIT with the numpy mirror (capi.chain_reduce_observables_reference, which
tests/test_chain_observables_host.py ties to the header's formulas) in all V outputs: random sums, walkers around the wave (63, 64,
65), the workgroup (255, 256, 257) and the point where the number of workgroups saturates (256 * 1024 - 1, .., 2 * 256 * 1024 + 5),
rows at both edges of every instance of the kernel (1, 4 | 5, 8 | 9, 16), with sentinels behind d_out and behind the stated size of
d_work.  The existing fdg_chain_reduce_device is the yardstick for unit rows (its order differs: within 1e-12 of the sum of
|term|).  The driver runs the known-answer graphs in leaf form beside the existing driver of the same arguments."""
import math

import numpy as np
import pytest
import torch

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, vegas
from test_chain_binned_host import cdf_of, known_b_graph
from test_chain_host import known_graph
from test_chain_matsubara_accumulate import leaf_case
from test_chain_observables_host import ROWS, formulas, idx, n_out
from test_strat_accumulate import assert_bits

pytestmark = pytest.mark.gpu

TOL = 1e-12
SENTINEL = -7.25
WALKERS = [1, 63, 64, 65, 255, 256, 257, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1, 2 * 256 * 1024 + 5]
ROWS_M = [1, 4, 5, 8, 9, 16]


def device_reduce(cuda, A, col_base, n_use, norm_col, coef, pre=None, d_A=None):
    """the entry on the sums ``A`` (host [n_columns, B], or ``d_A`` already on the device): the V outputs, from zeros or from ``pre``;
    the eight doubles behind d_out and the page behind the stated size of d_work are checked to be as they were"""
    M = np.asarray(coef).shape[0]
    V = n_out(M)
    d_A = torch.from_numpy(np.ascontiguousarray(A)).to(cuda) if d_A is None else d_A
    out = torch.full((V + 8,), SENTINEL, dtype=torch.float64, device=cuda)
    out[:V] = 0.0 if pre is None else torch.from_numpy(np.asarray(pre)).to(cuda)
    nb = capi.chain_reduce_observables_work_bytes(M, n_use)
    assert nb > 0
    work = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=cuda)
    capi.chain_reduce_observables_device(d_A.data_ptr(), d_A.shape[1], col_base, n_use, norm_col, coef, out.data_ptr(), work.data_ptr(),
                                         torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize(cuda)
    assert (out[V:] == SENTINEL).all().item(), "doubles behind d_out were written"
    assert (work[nb:] == 0xA5).all().item(), "bytes behind the stated size of d_work were written"
    return out[:V].cpu().numpy()


def random_rows(rng, M, n_use):
    """M rows over n_use columns: factors in [-2, 2], about a quarter of them zero, every row with a term"""
    c = rng.uniform(-2.0, 2.0, size=(M, n_use)) * (rng.random((M, n_use)) > 0.25)
    for m in range(M):
        if not c[m].any():
            c[m, rng.integers(n_use)] = 1.5
    return c


# ---- 1. the entry against the mirror, bit for bit -------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("B", WALKERS)
def test_the_entry_matches_the_mirror_bit_for_bit(libfdg, cuda, B):
    rng = np.random.default_rng(B)
    A9 = rng.normal(size=(9, B)) * rng.uniform(0.5, 3.0, size=(9, 1))
    d_A9 = torch.from_numpy(A9).to(cuda)
    for M in ROWS_M:
        # nine columns: the window 0 .. 7, the normalisation last; three columns: the window 0 .. 1 (beyond the workgroup only for the
        # smallest number of rows: the order of a sum does not depend on the columns, and the mirror's time does not shrink with them)
        for n_col in (9, 3) if (B <= 257 or M == 1) else (9,):
            n_use = n_col - 1
            coef = random_rows(rng, M, n_use)
            A, d_A = (A9, d_A9) if n_col == 9 else (A9[[4, 2, 7]].copy(), None)
            got = device_reduce(cuda, A, 0, n_use, n_use, coef, d_A=d_A)
            assert_bits(got, capi.chain_reduce_observables_reference(A, 0, n_use, n_use, coef), f"B {B}, M {M}, {n_col} columns")


# ---- 2. what the contract says beside the sums ------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("M", [3, 7, 12])
def test_prefilled_outputs_windows_and_zero_coefficients(libfdg, cuda, M):
    rng = np.random.default_rng(100 + M)
    B, n_col = 777, 12
    A = rng.normal(size=(n_col, B))
    A[n_col - 1] = rng.uniform(0.5, 2.0, size=B)
    pre = rng.normal(size=n_out(M))
    # a window in the middle of the columns, the normalisation last; a prefilled d_out is added to
    coef = random_rows(rng, M, 5)
    got = device_reduce(cuda, A, 3, 5, n_col - 1, coef, pre)
    assert_bits(got, capi.chain_reduce_observables_reference(A, 3, 5, n_col - 1, coef, out=pre), "window 3 .. 7 of 12, prefilled")
    assert not np.array_equal(got, pre)
    # ... and the normalisation may lie before the window as well
    got = device_reduce(cuda, A, 3, 5, 1, coef, pre)
    assert_bits(got, capi.chain_reduce_observables_reference(A, 3, 5, 1, coef, out=pre), "normalisation before the window")
    # a nan column with all-zero coefficients reaches no output; columns outside the window are not read either
    coef[:, 2] = 0.0
    clean = device_reduce(cuda, A, 3, 5, n_col - 1, coef)
    A2 = A.copy()
    A2[[0, 1, 2, 5, 8, 9, 10]] = math.nan
    got = device_reduce(cuda, A2, 3, 5, n_col - 1, coef)
    assert_bits(got, clean, "nan in a column of zero coefficients")
    assert np.isfinite(got).all()
    # a row without a term leaves its S entry and its row and column of P as they are
    gone = M // 2
    coef[gone] = 0.0
    got = device_reduce(cuda, A, 3, 5, n_col - 1, coef, pre)
    want = capi.chain_reduce_observables_reference(A, 3, 5, n_col - 1, coef, out=pre)
    kept = [gone] + [idx(min(gone, q), max(gone, q), M) for q in range(M + 1)]
    assert_bits(got, want, "a row without a term")
    assert_bits(got[kept], pre[kept], "the outputs of a row without a term")
    # no row has a term: only the normalisation's sum and square are added
    got = device_reduce(cuda, A, 3, 5, n_col - 1, np.zeros((M, 5)), pre)
    want = pre.copy()
    want[M] += capi.chain_reduce_observables_reference(A, 3, 5, n_col - 1, np.zeros((M, 5)))[M]
    want[-1] = capi.chain_reduce_observables_reference(A, 3, 5, n_col - 1, np.zeros((M, 5)), out=pre)[-1]
    assert_bits(got, want, "no row has a term")


def test_an_interleaved_window_of_real_and_imaginary_columns(libfdg, cuda):
    """the layout of a projected chain: 2 R interleaved columns per (bin, frequency); rows (Re o_0 .., Im o_0 ..) as the driver builds them"""
    rng = np.random.default_rng(7)
    R, F, B, Mf = 5, 3, 300, 2
    A = rng.normal(size=(2 * F * R + 1, B))
    A[-1] = rng.uniform(0.5, 2.0, size=B)
    fcoef = rng.uniform(-2.0, 2.0, size=(Mf, R))
    fcoef[1, 3] = 0.0
    _, rows = vegas._chain_observable_rows(None, vegas.FrequencyObservables(tuple(map(tuple, fcoef))), R)
    assert rows.shape == (2 * Mf, 2 * R)
    for f in range(F):
        got = device_reduce(cuda, A, 2 * f * R, 2 * R, 2 * F * R, rows)
        assert_bits(got, capi.chain_reduce_observables_reference(A, 2 * f * R, 2 * R, 2 * F * R, rows), f"frequency {f}")
        re, im = A[2 * f * R:2 * (f + 1) * R:2], A[2 * f * R + 1:2 * (f + 1) * R:2]
        want = np.concatenate([(fcoef @ re).sum(axis=1), (fcoef @ im).sum(axis=1)])
        assert np.allclose(got[:2 * Mf], want, rtol=1e-10, atol=1e-10)


# ---- 3. the existing reduction as the yardstick ---------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("R", [2, 8, 16])
def test_unit_rows_agree_with_the_existing_reduction(libfdg, cuda, R):
    rng = np.random.default_rng(R)
    B = 5000
    A = rng.normal(size=(R + 1, B)) * rng.uniform(0.5, 3.0, size=(R + 1, 1))
    d_A = torch.from_numpy(A).to(cuda)
    old = torch.zeros(3 * R + 2, dtype=torch.float64, device=cuda)
    capi.chain_reduce_device(d_A.data_ptr(), R, B, old.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
    got = device_reduce(cuda, A, 0, R, R, np.eye(R), d_A=d_A)
    old = old.cpu().numpy()
    S, Q, X = old[:R + 1], old[R + 1:2 * R + 2], old[2 * R + 2:]
    absum = np.array([math.fsum(np.abs(a)) for a in A])
    sq = np.array([math.fsum(a * a) for a in A])
    assert (np.abs(got[:R + 1] - S) <= TOL * absum).all()
    diag = np.array([got[idx(p, p, R)] for p in range(R + 1)])
    assert (np.abs(diag - Q) <= TOL * sq).all()
    cross = np.array([got[idx(k, R, R)] for k in range(R)])
    assert (np.abs(cross - X) <= TOL * np.array([math.fsum(np.abs(A[k] * A[R])) for k in range(R)])).all()


def test_two_shards_add_up(libfdg, cuda):
    rng = np.random.default_rng(65)
    M, n_col = 5, 7
    A = rng.normal(size=(n_col, 130))
    coef = random_rows(rng, M, n_col - 1)
    whole = device_reduce(cuda, A, 0, n_col - 1, n_col - 1, coef)
    half = device_reduce(cuda, A[:, :65].copy(), 0, n_col - 1, n_col - 1, coef)
    both = device_reduce(cuda, A[:, 65:].copy(), 0, n_col - 1, n_col - 1, coef, half)
    _, scale = formulas(A, 0, n_col - 1, n_col - 1, coef)
    assert (np.abs(both - whole) <= TOL * scale).all() and not np.array_equal(half, whole)


# ---- 4. the driver ------------------------------------------------------------------------------------------------------------------------ #
RUN = dict(n_walker=130, n_step=12, n_therm=3, n_warm=0, seed=5)


def driver_cases(cuda):
    """name -> (existing driver, its extra positional arguments, the new driver's keywords for them, common arguments, observables)"""
    cases = {}
    t, col, fixed = known_graph()
    f = fd.compile_table(t, specialize="isa")
    common = dict(RUN, n_grid=8, gamma=0.05, fixed=fixed, coef=[1.0, 1.0], device=cuda)
    ob = dict(observables=vegas.Observables(tuple(map(tuple, ROWS))))
    cases["plain"] = (vegas.chain_integrate, (f, None, [0, 0], [1, 1], col), (), {}, common, ob)
    sh = vegas.ChainShift(width=[0.1, 0.3])
    cases["shift"] = (vegas.chain_integrate_shift, (f, None, [0, 0], [1, 1], col), (sh,), dict(shift=sh), common, ob)
    # the random graph of tests/test_chain_matsubara_accumulate.py with the two weight groups of tests/test_chain_groups_accumulate.py
    # and a projection on two frequencies; the root that does not exist may name any time
    t, f, col, fixed, grid, coef, exists, cin, cout = leaf_case(cuda)
    R = t.n_root
    lab = lambda cols: tuple(c + 1 if e else 1 for c, e in zip(cols, exists))
    groups = vegas.WeightGroups(tuple([0, 1] * 5), ((0, 2), (0, 1, 2)))
    mz = vegas.MatsubaraProjection((2, -1), True, lab(cin), lab(cout))
    rng = np.random.default_rng(23)
    fcoef = rng.uniform(-2.0, 2.0, size=(2, R))
    fcoef[0, 4] = 0.0
    common = dict(RUN, gamma=0.37, reweight=[0.7, 1.9], fixed=fixed, coef=coef, vmap=vegas.VegasMap(grid, cuda), device=cuda, matsubara=mz,
                  weight_freq=1)
    cases["grouped, projected"] = (vegas.chain_integrate_grouped, (f, None, grid[:, 0], grid[:, -1], col), (groups, 0.0, 1.7),
                                   dict(groups=groups, beta=1.7), common, dict(freq_observables=vegas.FrequencyObservables(tuple(map(tuple, fcoef)))))
    t, col, ecol, fixed = known_b_graph()
    f = fd.compile_table(t, specialize="isa")
    dm = lambda: vegas.DiscreteMap(cdf_of((0.5, 0.125, 0.375)), np.array([[0.5], [1.0], [2.0]]), [ecol], device=cuda)
    common = dict(RUN, n_grid=8, gamma=0.05, fixed=fixed, device=cuda)
    cases["dmap"] = (vegas.chain_integrate_binned, (f, None, [0, 0], [1, 1], col), dm, "dmap", common, ob)
    return cases


def run_new(case, **kw):
    old_fn, args, extra, new_kw, common, ob = case
    if new_kw == "dmap":
        new_kw = dict(dmap=extra())
    return vegas.chain_integrate_observables(*args, **{**common, **new_kw, **ob, **kw})


def run_old(case):
    old_fn, args, extra, new_kw, common, ob = case
    return old_fn(*args, *((extra(),) if callable(extra) else extra), **common)


def blocks_of(res, case):
    """(rows, [(col_base, n_use)], norm_col, the raw sums per block, M) of a result of the new driver"""
    ob = case[5]
    R = case[1][0].handle.table.n_root
    n_sum = res.walker_sums.shape[0]
    if "observables" in ob:
        rows = np.array(ob["observables"].coef)
        sums = res.obs_sums.reshape(-1, res.obs_sums.shape[-1])
        return rows, [(j * R, R) for j in range((n_sum - 1) // R)], n_sum - 1, sums
    _, rows = vegas._chain_observable_rows(None, ob["freq_observables"], R)
    sums = res.fobs_sums.reshape(-1, res.fobs_sums.shape[-1])
    return rows, [(2 * jf * R, 2 * R) for jf in range((n_sum - 1) // (2 * R))], n_sum - 1, sums


@pytest.mark.parametrize("name", ["plain", "shift", "grouped, projected", "dmap"])
def test_the_driver_beside_the_existing_one(libfdg, cuda, name):
    case = driver_cases(cuda)[name]
    res, old = run_new(case, keep_sums=True), run_old(case)
    # 1. everything the existing driver reports, bit for bit
    for k in ("mean", "stderr", "S", "Q", "X"):
        assert_bits(getattr(res, k), getattr(old, k), f"{name}: {k}")
    assert res.acceptance == old.acceptance and res.gamma == old.gamma and 0.0 < res.acceptance < 1.0
    assert (res.shift_width is None and old.shift_width is None) or np.array_equal(res.shift_width, old.shift_width)
    assert (res.reweight is None and old.reweight is None) or np.array_equal(res.reweight, old.reweight)
    assert type(old) is vegas.ChainResult and type(res) is vegas.ChainObservablesResult and isinstance(res, vegas.ChainResult)
    # 2. the raw sums of every block, bit for bit the mirror's on the driver's own walkers' sums
    total = res.walker_sums.cpu().numpy()
    rows, blocks, norm_col, sums = blocks_of(res, case)
    M = rows.shape[0]
    assert len(blocks) == sums.shape[0] and sums.shape[1] == n_out(M) and total.shape[1] == RUN["n_walker"]
    for (base, n_use), got in zip(blocks, sums):
        assert_bits(got, capi.chain_reduce_observables_reference(total, base, n_use, norm_col, rows), f"{name}: block at column {base}")
    # 3. the means are the combinations of the roots' means; the shapes are the direct drivers'
    if res.obs_mean is not None:
        lead = res.mean.shape[:-1]
        assert res.obs_mean.shape == lead + (M,) and res.obs_cov.shape == lead + (M, M) and res.obs_stderr.shape == lead + (M,)
        assert res.fobs_mean is None and res.fobs_cov is None and res.fobs_sums is None
        want = res.mean @ rows.T
        bar = TOL * np.maximum(1.0, np.abs(res.mean) @ np.abs(rows).T)
        assert (np.abs(res.obs_mean - want) <= bar).all(), (name, np.abs(res.obs_mean - want).max())
        assert np.array_equal(res.obs_cov, np.swapaxes(res.obs_cov, -1, -2)) and (res.obs_stderr > 0.0).all()
        unit = res.obs_stderr[..., 2:]                                         # rows 2 and 3 are the roots themselves
        assert (np.abs(unit - res.stderr) <= 1e-9 * res.stderr).all()
    else:
        fcoef = np.array(case[5]["freq_observables"].coef)
        Mf, F = fcoef.shape[0], res.mean.shape[0]
        assert res.fobs_mean.shape == (F, Mf) and res.fobs_stderr.shape == (F, Mf) and res.fobs_cov.shape == (F, 2 * Mf, 2 * Mf)
        assert res.fobs_mean.dtype == np.complex128 and res.obs_mean is None and res.obs_sums is None
        want = res.mean @ fcoef.T
        bar = TOL * np.maximum(1.0, np.abs(res.mean) @ np.abs(fcoef).T)
        assert (np.abs(res.fobs_mean - want) <= bar).all(), (name, np.abs(res.fobs_mean - want).max())
        sd = np.sqrt(np.stack([np.diag(c) for c in res.fobs_cov]))
        assert np.array_equal(res.fobs_stderr.real, sd[:, :Mf]) and np.array_equal(res.fobs_stderr.imag, sd[:, Mf:]) and (sd > 0.0).all()
    # 4. one shard against two: the walkers' sums are the whole's bit for bit, the raw sums add up within the bar of a sum
    parts = [run_new(case, keep_sums=True, n_walker=65, n_total=130, shard_start=lo) for lo in (0, 65)]
    for lo, p in zip((0, 65), parts):
        assert_bits(p.walker_sums.cpu().numpy(), total[:, lo:lo + 65], f"{name}: the walkers' sums of the shard at {lo}")
    psums = [blocks_of(p, case)[3] for p in parts]
    for (base, n_use), whole, a, b in zip(blocks, sums, psums[0], psums[1]):
        _, scale = formulas(total, base, n_use, norm_col, rows)
        assert (np.abs(a + b - whole) <= TOL * scale).all(), (name, base)

    # ... and with reduce every shard reports the whole's figures
    def add_other(other):
        def reduce(v):
            if v.shape == other.shape:
                v += torch.from_numpy(other).to(v.device)
        return reduce
    key = "obs_sums" if res.obs_sums is not None else "fobs_sums"
    other = getattr(parts[1], key).reshape(sums.shape)
    red = run_new(case, n_walker=65, n_total=130, shard_start=0, reduce=add_other(other))
    assert_bits(getattr(red, key).reshape(sums.shape), psums[0] + psums[1], f"{name}: reduce on the raw sums")
