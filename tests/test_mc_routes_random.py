"""The leaf kernels and the split / fused routes of the Monte-Carlo step on random tables.

tests/test_random_graphs.py fuzzes the one-kernel route of the optimizing back end (FDG_MC_ROUTE=isa) only; the table-driven
leaf kernel (fdg_leaf_kernel), the kernel specialised to the tables (fdg_leaf_spec) and routes 1 (fused) and 2 (split) of
fdg_graph_specialize_fused otherwise see the two GV partitions: no leaf without a formula, three dimensions, a basis of
0 / +-1, one beta, component-major K and T, a fresh handle and one batch size per test.  Here:

 0. a census of the random inputs, on the CPU: what the device tests below rely on is really in seeds 0..15;
 1. both leaf kernels on random tables in every input and output layout, against the oracle's leaves at the project's
    tolerances (check_leaves), with everything they do not own left alone;
 2. routes 1 and 2 (and the library's own choice) on random graphs over random tables: the bits of the unfused sequence
    (leaf kernel into a buffer of ones, then the same kind of evaluator) and within 1e-12 max(1, root scale), plus the
    reference's own uncertainty where a graph cancels inside, of the oracle;
 3. one handle through many calls -- batch sizes that change the leaf stride of the chunk of leaves, a handle moved between
    the one-kernel and the split route (they share the buffer), and binned calls whose last chunk is shorter than the others:
    the columns of the leaves without a formula (value 1.0) have to be right in every one of them.
"""
import glob
import os

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT, OP_PROD, OP_SUM, from_program
from test_random_graphs import check_leaves, leaves_table, random_leaf_tables, random_table, same

SEEDS = list(range(16))               # the default MC_SEEDS of tests/test_random_graphs.py
KF, LAM = 1.3, 0.9
BETAS = [0.7, 3.0, 25.0]
PREFILL = 9.0                         # roots before a call: an absent root (FDG_NO_ROOT) keeps it
SENTINEL = -7.0                       # leaf buffers before a call: what the leaf kernels do not own keeps it
TOL = 1e-12


def case(seed, clip=False, min_type0=0, dim=None):
    """(graph, tables, dim, beta) of a seed; clip: interaction orders <= 3; min_type0: at least so many leaves without a formula"""
    t = random_table(seed)
    z = random_leaf_tables(seed, t.n_leaf, max_interaction_order=3 if clip else None)
    if min_type0:
        z = with_type0(z, min_type0)
    beta = float(np.random.default_rng(seed).choice(BETAS))     # (the draw of test_random_mc_step_on_device)
    return t, z, (2 + seed % 2) if dim is None else dim, beta


def with_type0(z, n):
    """the tables with the first leaves that have a formula turned into leaves without one, until there are n of those"""
    z = dict(z)
    ty = z["leaf_type"].copy()
    assert len(ty) >= n + 1                                     # (at least one leaf keeps its formula)
    for i in range(len(ty)):
        if (ty == 0).sum() >= n:
            break
        ty[i] = 0
    z["leaf_type"] = ty
    return z


def high_order(z):
    return bool(((z["leaf_type"] == 2) & (z["leaf_order"] > 3)).any())


def tab_args(z, dim):
    return (z["leaf_type"], z["leaf_order"], z["tau_in"], z["tau_out"], z["loop_index"], z["basis"], dim, z["n_tau"])


def host_inputs(z, dim, beta, B, key):
    rng = np.random.default_rng(key)
    return rng.uniform(-2, 2, (B, z["n_loop"], dim)), rng.uniform(0, beta, (B, z["n_tau"]))


S3_SEEDS = [1, 2, 4, 7]               # section 3: graphs with three leaves or more (two lose their formula, one keeps it)


# --------------------------------------------------------------------------- #
# 0. census
# --------------------------------------------------------------------------- #
def test_census_of_the_random_inputs():
    """What the device tests rely on is in the seeds they run (conditions, not measurements: a seed list that misses one is
    changed, not the threshold)."""
    n = dict(type0=0, tau0=0, ford=0, hi=0, lo=0)
    basis, dims, betas = set(), set(), set()
    for seed in SEEDS:
        t, z, dim, beta = case(seed)
        _, zc, _, _ = case(seed, clip=True)
        ty, od = z["leaf_type"], z["leaf_order"]
        n["type0"] += bool((ty == 0).any())
        n["tau0"] += bool(((ty == 1) & (z["tau_in"] == z["tau_out"])).any())
        n["ford"] += bool(((ty == 1) & (od >= 1) & (od <= 5)).any())
        n["hi"] += high_order(z)
        n["lo"] += (not high_order(zc)) and bool((zc["leaf_type"] == 2).any())
        assert all(np.array_equal(z[k], zc[k]) for k in z if k != "leaf_order")          # the clip changes the orders only
        assert np.array_equal(od[ty != 2], zc["leaf_order"][ty != 2])
        used = np.unique(z["loop_index"][ty != 0]) - 1
        basis |= set(z["basis"][used].ravel().tolist())
        dims.add(dim)
        betas.add(beta)
    assert all(v >= 4 for v in n.values()), n
    assert 0.5 in basis and -1.0 in basis
    assert dims == {2, 3}
    assert len(betas) >= 3
    # both dimensions reach the specialised kernel (clipped tables) and the pow_body branch of the generic one
    assert {case(s)[2] for s in SEEDS if high_order(case(s)[1])} == {2, 3}
    for seed in S3_SEEDS:
        assert random_table(seed).n_leaf >= 3
    assert {case(s)[2] for s in S3_SEEDS} == {2, 3}


# --------------------------------------------------------------------------- #
# 1. the leaf kernels
# --------------------------------------------------------------------------- #
LEAF_B = [1, 63, 64, 65, 193]         # lane tail, exact tile, one past a tile, several tiles
KT_LAYOUTS = ["component", "sample", "padded"]
OUT_LAYOUTS = ["leaf_major", "sample_major", "tiled"]


def kt_on_device(cuda, K, T, layout):
    """(dK, ks, kc, dT, ts, tc): component-major (1, B), sample-major (n, 1), or rows of n + 3 with NaN behind the row"""
    import torch
    B = K.shape[0]
    out = []
    for x in (K.reshape(B, -1), T):
        n = x.shape[1]
        if layout == "component":
            out += [torch.from_numpy(np.ascontiguousarray(x.T)).to(cuda), 1, B]
        elif layout == "sample":
            out += [torch.from_numpy(np.ascontiguousarray(x)).to(cuda), n, 1]
        else:
            pad = np.full((B, n + 3), np.nan)
            pad[:, :n] = x
            out += [torch.from_numpy(pad).to(cuda), n + 3, 1]
    return out


def leaves_on_device(cuda, z, dim, beta, kt, B, layout, st):
    """One call of the leaf entry point into a buffer of SENTINEL that is larger than the batch in every direction.  Returns the leaves
    [B, L] with the columns of the leaves without a formula set to 1.0 -- after the check that those columns, the rows behind the batch and
    the padding still hold the sentinel."""
    import torch
    from test_tile_major import from_tiles
    L = len(z["leaf_type"])
    dK, ks, kc, dT, ts, tc = kt
    own = (z["leaf_type"] != 0)
    if layout == "tiled":
        n_tile = (B + 63) // 64
        buf = torch.full((n_tile, L + 1, 64), SENTINEL, dtype=torch.float64, device=cuda)
        capi.leaf_eval_device_tiled(*tab_args(z, dim), KF, beta, LAM, dK.data_ptr(), ks, kc, dT.data_ptr(), ts, tc, buf.data_ptr(), 1, 64,
                                    (L + 1) * 64, B, st)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        mask = np.zeros(h.shape, dtype=bool)
        lane = (np.arange(n_tile)[:, None] * 64 + np.arange(64)[None, :]) < B
        mask[:, :L, :] = own[None, :, None] & lane[:, None, :]
        got = from_tiles(h, B, L).copy()
    else:
        shape, ss, ls = ((L + 1, B + 5), 1, B + 5) if layout == "leaf_major" else ((B + 2, L + 3), L + 3, 1)
        buf = torch.full(shape, SENTINEL, dtype=torch.float64, device=cuda)
        capi.leaf_eval_device(*tab_args(z, dim), KF, beta, LAM, dK.data_ptr(), ks, kc, dT.data_ptr(), ts, tc, buf.data_ptr(), ss, ls, B, st)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        mask = np.zeros(h.shape, dtype=bool)
        if layout == "leaf_major":
            mask[:L, :B] = own[:, None]
            got = h[:L, :B].T.copy()
        else:
            mask[:B, :L] = own[None, :]
            got = h[:B, :L].copy()
    assert (h[~mask] == SENTINEL).all(), (layout, B, "written outside the batch's own leaves", np.argwhere((h != SENTINEL) & ~mask)[:4])
    assert (got[:, ~own] == SENTINEL).all()
    got[:, ~own] = 1.0
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_leaf_kernels_on_random_tables(libfdg, cuda, fdgopt, tmp_path, seed):
    """fdg_leaf_eval_device / _tiled with FDG_LEAF_GENERIC set (table-driven kernel) and unset (the kernel specialised to the tables where
    every interaction order is <= 3), on the seed's tables as drawn and with the orders clipped: check_leaves' tolerances (1e-13 relative,
    1e-12 of the largest Leibniz term for derivative orders), every input and output layout the bits of the first one, nothing written
    that the kernel does not own, and the specialised kernel the bits of the table-driven one."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    os.chmod(tmp_path, 0o700)
    fdgopt.set("FDG_CACHE_DIR", str(tmp_path))
    variants = [case(seed)]
    if high_order(variants[0][1]):
        variants.append(case(seed, clip=True))
    for _, z, dim, beta in variants:
        spec_applies = not high_order(z) and bool((z["leaf_type"] != 0).any())
        for iB, B in enumerate(LEAF_B):
            K, T = host_inputs(z, dim, beta, B, 100 * seed + B)
            first = {}
            for generic in (True, False):
                if generic:
                    fdgopt.set("FDG_LEAF_GENERIC", "1")
                else:
                    fdgopt.unset("FDG_LEAF_GENERIC")
                for j, out in enumerate(OUT_LAYOUTS):
                    lay = KT_LAYOUTS[(iB + j + seed) % 3]                     # every (B, K/T layout) and every (B, output layout) pair occurs
                    got = leaves_on_device(cuda, z, dim, beta, kt_on_device(cuda, K, T, lay), B, out, st)
                    if generic not in first:
                        check_leaves(z, got, K, T, KF, beta, LAM)
                        first[generic] = got
                    else:
                        assert same(got, first[generic]), (seed, B, generic, lay, out)
            if spec_applies:
                assert same(first[False], first[True]), (seed, B, "specialised kernel differs from the table-driven one")
        if spec_applies:    # the specialised kernel was really built (a failed compilation falls back to the table-driven kernel)
            assert glob.glob(str(tmp_path / "fdg_leaf_*.hsaco")), seed


# --------------------------------------------------------------------------- #
# 2. routes 1 and 2 on random graphs over random tables
# --------------------------------------------------------------------------- #
def component_major(cuda, K, T):
    import torch
    B = K.shape[0]
    return torch.from_numpy(np.ascontiguousarray(K.reshape(B, -1).T)).to(cuda), torch.from_numpy(np.ascontiguousarray(T.T)).to(cuda)


def unfused_roots(f, z, dim, beta, dK, dT, B, st):
    """the sequence the routes replace, on the device: leaf kernel into a buffer of ones, then the handle's evaluator"""
    import torch
    L, R = len(z["leaf_type"]), f.handle.table.n_root
    leaf = torch.ones((L, B), dtype=torch.float64, device=dK.device).t()
    capi.leaf_eval_device(*tab_args(z, dim), KF, beta, LAM, dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, leaf.data_ptr(), leaf.stride(0),
                          leaf.stride(1), B, st)
    root = torch.full((B, R), PREFILL, dtype=torch.float64, device=dK.device)
    f(root, leaf)
    torch.cuda.synchronize()
    return root.cpu().numpy()


def mc_roots(h, dK, dT, beta, B, R, st):
    import torch
    root = torch.full((B, R), PREFILL, dtype=torch.float64, device=dK.device)
    h.mc_eval_device(dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, KF, beta, LAM, root.data_ptr(), R, 1, B, st)
    torch.cuda.synchronize()
    return root.cpu().numpy()


def leaf_tolerance(z, lv, K, T, beta):
    """check_leaves' own bars per entry: 1e-12 of the largest Leibniz term for derivative orders, 1e-13 relative otherwise, 0 for 1.0"""
    tol = 1e-13 * np.abs(lv)
    q2 = (np.einsum("bjd,nj->bnd", K, z["basis"]) ** 2).sum(axis=2)
    for i in range(len(z["leaf_type"])):
        if z["leaf_type"][i] == 0:
            tol[:, i] = 0.0
        elif z["leaf_type"][i] == 1 and z["leaf_order"][i] > 0:
            tau = T[:, z["tau_out"][i] - 1] - T[:, z["tau_in"][i] - 1]
            tol[:, i] = 1e-12 * oracle.green_derive_scale(tau, q2[:, z["loop_index"][i] - 1] - KF * KF, beta, int(z["leaf_order"][i]))
    return tol


def reference_uncertainty(t, lv, dl):
    """How far the roots of the oracle's graph can move when every leaf moves by up to dl and every operation rounds (twice: once on
    either side of a comparison): a running error bound (Higham, Accuracy and Stability of Numerical Algorithms, 3.3) carried through the
    nodes next to the values.  With a = |f v| and e the bound of a term f v: a sum of terms moves by at most sum e, a product by at
    most sum_j e_j prod_{i != j} (a_i + e_i), and each node adds 2 u (number of operations) (sum of |terms|, or |product|), u = 2^-53.
    Nothing in it comes from a kernel: the values are the oracle's, dl is check_leaves' bar."""
    from feynmandiagram_jl_amd.nodetable import OP_POWER
    u = 2.0 ** -53
    L = t.n_leaf
    val = [lv[:, i] for i in range(L)]
    err = [dl[:, i] for i in range(L)]
    off, idx, fac = t.child_off, t.child_idx, t.child_fac
    with np.errstate(all="ignore"):
        for n in range(t.op.shape[0]):
            a, b = int(off[n]), int(off[n + 1])
            ch = [(int(idx[e]), float(fac[e])) for e in range(a, b)]
            if int(t.op[n]) == OP_POWER:
                ch = [(ch[0][0], 1.0)] * (int(t.power[n]) - 1) + [ch[0]]               # x^n f as the product x ... x (x f)
            mag = [np.abs(f * val[c]) for c, f in ch]
            er = [abs(f) * err[c] for c, f in ch]
            if int(t.op[n]) == OP_SUM:
                v = sum(f * val[c] for c, f in ch)
                e = sum(er) + 2 * u * 2 * len(ch) * sum(mag)
            else:
                v = np.prod([f * val[c] for c, f in ch], axis=0)
                e = 2 * u * 2 * len(ch) * np.prod([m + x for m, x in zip(mag, er)], axis=0)
                for j in range(len(ch)):
                    e = e + er[j] * np.prod([m + x for i, (m, x) in enumerate(zip(mag, er)) if i != j] + [np.ones_like(er[j])], axis=0)
            val.append(v)
            err.append(e)
    out = np.zeros((lv.shape[0], t.n_root))
    for k, s in enumerate(t.root_slot):
        if s != FDG_NO_ROOT:
            out[:, k] = err[int(s)]
    return out


def check_against_oracle(t, z, K, T, beta, got, what):
    """Against the oracle's graph on the oracle's leaves (1.0 where a leaf has no formula): within 1e-12 max(1, root scale) plus the
    reference's own uncertainty there (reference_uncertainty of check_leaves' bars); absent roots untouched.

    Why the second term.  The root scale is the sum of |terms| of the root's own Sum node: it does not see cancellation inside the
    graph, and some of the random graphs cancel there.  Measured on the CPU against 60-digit mpmath (exact leaf formulas and exact graph
    on the same float64 K, T), the oracle's own float64 roots are off by up to 4.5e-9 of max(1, root scale) on seed 0 and by many
    orders of magnitude more than the scale on single samples of seed 7 at B = 1000 (large interior terms cancel);
    moving the oracle's leaves by one ulp moves seed 7's roots by 7e-3 of the scale.  No evaluation in float64 can meet
    1e-12 max(1, root scale) there, so the bar is that plus what the reference itself cannot pin down.  Where the graph does not cancel
    the second term is a few 1e-13 of the root's terms and the bar is the first one; both figures are printed."""
    lv = oracle.leaf_values(*tab_args(z, 0)[:6], K, T, KF, beta, LAM)
    lv[:, z["leaf_type"] == 0] = 1.0
    with np.errstate(all="ignore"):
        want = oracle.eval_static(t, lv, np.full(got.shape, PREFILL))
        scale = np.maximum(1.0, oracle.root_scale(t, lv))
        tol = TOL * scale + reference_uncertainty(t, lv, leaf_tolerance(z, lv, K, T, beta))
    live = t.root_slot != FDG_NO_ROOT
    assert (got[:, ~live] == PREFILL).all(), what
    ok = np.isfinite(want) & np.isfinite(tol) & live[None, :]
    assert np.isfinite(got[ok]).all(), what
    d = np.abs(got - want)[ok]
    print(what, "max |d| / max(1, root scale) =", float((d / scale[ok]).max()) if d.size else 0.0,
          "; max |d| / bar =", float((d / tol[ok]).max()) if d.size else 0.0)
    assert np.all(d <= tol[ok]), (what, float((d / tol[ok]).max()))


def check_mc_eval(f_ref, h, t, z, dim, beta, B, key, st, cuda, bitwise, what):
    """one mc_eval_device call against the unfused sequence (bits, or -- the one-kernel route, whose exponential is not the leaf kernel's --
    1e-12 max(1, root scale)) and against the oracle; returns (roots, dK, dT)"""
    K, T = host_inputs(z, dim, beta, B, key)
    dK, dT = component_major(cuda, K, T)
    got = mc_roots(h, dK, dT, beta, B, t.n_root, st)
    want = unfused_roots(f_ref, z, dim, beta, dK, dT, B, st)
    if bitwise:
        assert same(got, want), (what, B, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:4])
    else:
        lv = oracle.leaf_values(*tab_args(z, 0)[:6], K, T, KF, beta, LAM)
        lv[:, z["leaf_type"] == 0] = 1.0
        with np.errstate(all="ignore"):
            scale = np.maximum(1.0, oracle.root_scale(t, lv))
        ok = np.isfinite(want) & np.isfinite(scale)
        assert np.array_equal(np.isfinite(got), np.isfinite(want)), (what, B)
        assert np.all(np.abs(got - want)[ok] <= TOL * scale[ok]), (what, B)
    if t.n_node == 0:                                   # every leaf is a root: the leaves themselves
        assert (got[:, z["leaf_type"] == 0] == 1.0).all(), (what, B, "a leaf without a formula is not 1.0")
        check_leaves(z, got, K, T, KF, beta, LAM)
    check_against_oracle(t, z, K, T, beta, got, (what, B))
    return got, dK, dT


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_split_and_fused_routes_on_random_graphs(libfdg, cuda, fdgopt, seed):
    """FDG_MC_ROUTE=split on the tables as drawn, =fused on the tables with the interaction orders clipped to 3 (FDG_E_UNSUPPORTED on the
    others), and the library's own choice, on an ISA-specialised and a HIP-source handle, B = 1, 65, 1000: mc_eval_device gives the bits
    of the unfused sequence and lies within check_against_oracle's bar of the oracle; mc_accumulate_device lies within
    1e-12 max(1, sum |w root|) of the host's sum over those roots.

    (The bar against the oracle is check_against_oracle's: 1e-12 max(1, root scale) plus the reference's own uncertainty; measured on an
    MI355X the plain 1e-12 max(1, root scale) holds on 14 seeds -- largest figure 9e-13, seed 0 -- and seeds 7 and 10, whose graphs cancel
    inside, give 2.2e-9 and 1.3e-8 of the root scale at B = 1000 on every route alike.)"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    t, z_any, dim, beta = case(seed)
    _, z_clip, _, _ = case(seed, clip=True)
    live = t.root_slot != FDG_NO_ROOT
    for spec in ("isa", True):
        f_ref = fd.compile_table(t, specialize=spec)
        for route, z in (("split", z_any), ("fused", z_clip), (None, z_any)):
            if route:
                fdgopt.set("FDG_MC_ROUTE", route)
            else:
                fdgopt.unset("FDG_MC_ROUTE")
            f = fd.compile_table(t, specialize=spec)
            if route == "fused" and high_order(z_any):
                bad, _keep_bad = capi.make_leaf_tables(*tab_args(z_any, dim))
                with pytest.raises(capi.FdgError) as e:
                    f.handle.specialize_fused(bad)
                assert e.value.code == capi.FDG_E_UNSUPPORTED
            tab, _keep = capi.make_leaf_tables(*tab_args(z, dim))
            f.handle.specialize_fused(tab)
            # left to itself an ISA handle takes the one-kernel route for graphs above 300 operations (its own exponential: not the bits)
            bitwise = route is not None or spec is True or f.info()["flops_alg"] <= 300
            for B in (1, 65, 1000):
                what = (seed, spec, route)
                got, dK, dT = check_mc_eval(f_ref, f.handle, t, z, dim, beta, B, 100 * seed + B, st, cuda, bitwise, what)
                w = torch.rand(B, dtype=torch.float64, device=cuda)
                acc = torch.zeros(t.n_root, dtype=torch.float64, device=cuda)
                f.handle.mc_accumulate_device(dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, KF, beta, LAM, w.data_ptr(), acc.data_ptr(), B, st)
                torch.cuda.synchronize()
                wr = np.where(live[None, :], got, 0.0) * w.cpu().numpy()[:, None]
                fin = np.isfinite(wr).all(axis=0) & live
                assert np.all(np.abs(acc.cpu().numpy() - wr.sum(0))[fin] <= TOL * np.maximum(1.0, np.abs(wr).sum(0))[fin]), (what, B)


# --------------------------------------------------------------------------- #
# 3. one handle, many calls
# --------------------------------------------------------------------------- #
def s3_case(kind, seed, dim=None):
    t, z, dim, beta = case(seed, min_type0=2, dim=dim)
    assert (z["leaf_type"] == 0).sum() >= 2 and (z["leaf_type"] != 0).any()
    return (leaves_table(t.n_leaf) if kind == "leaves" else t), z, dim, beta


@pytest.mark.gpu
@pytest.mark.parametrize("seed", S3_SEEDS)
@pytest.mark.parametrize("kind", ["leaves", "random"])
def test_split_route_one_handle_many_batch_sizes(libfdg, cuda, fdgopt, kind, seed):
    """The chunk of leaves of the split route is leaf-major with the call's own leaf stride (the batch rounded up to 64, at most the chunk
    size).  One handle, one stream, B = 1000, 100, 64, 1000, 4099, 1: every call gives the bits of the unfused sequence -- the columns of
    the leaves without a formula are 1.0 at the stride of that call, not where an earlier call left them.  The same with FDG_MC_CHUNK=128
    (B = 1000 in eight chunks, then 70).

    Measured on an MI355X: before the constant columns were stored per call all eight cases failed at the second or third call (stale
    leaves in the place of 1.0)."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    t, z, dim, beta = s3_case(kind, seed)
    fdgopt.set("FDG_MC_ROUTE", "split")
    for spec in ("isa", True):
        f_ref = fd.compile_table(t, specialize=spec)
        tab, _keep = capi.make_leaf_tables(*tab_args(z, dim))
        for chunk, sizes in ((None, (1000, 100, 64, 1000, 4099, 1)), ("128", (1000, 70))):
            f = fd.compile_table(t, specialize=spec, options={"FDG_MC_CHUNK": chunk} if chunk else None)
            f.handle.specialize_fused(tab)
            for n, B in enumerate(sizes):
                check_mc_eval(f_ref, f.handle, t, z, dim, beta, B, 1000 * seed + 10 * n + 1, st, cuda, True, (kind, seed, spec, chunk, n))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", S3_SEEDS[:2])
@pytest.mark.parametrize("kind", ["leaves", "random"])
@pytest.mark.parametrize("order", ["isa_then_split", "split_then_isa"])
def test_handle_moved_between_the_one_kernel_and_the_split_route(libfdg, cuda, kind, seed, order):
    """Routes 2 and 3 share one buffer of the handle: route 3 packs (K, T) that are not component-major into it, route 2 keeps its chunk of
    leaves there.  A handle specialised for one route, run at B = 4099 on sample-major K and T (so that route 3 does use the buffer), then
    specialised for the other and run at B = 1000: each call is right -- the split route finds no ones from an earlier call, and must not
    need them."""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    t, z, dim, beta = s3_case(kind, seed, dim=3)
    f_ref = fd.compile_table(t, specialize="isa")
    f = fd.compile_table(t, specialize="isa")
    tab, _keep = capi.make_leaf_tables(*tab_args(z, dim))
    routes = ["isa", "split"] if order == "isa_then_split" else ["split", "isa"]
    for n, (route, B) in enumerate(zip(routes, (4099, 1000) if order == "isa_then_split" else (1000, 4099))):
        f.handle.set_option("FDG_MC_ROUTE", route)
        f.handle.specialize_fused(tab)
        what = (kind, seed, order, route)
        if route == "split":
            check_mc_eval(f_ref, f.handle, t, z, dim, beta, B, 77 * seed + n, st, cuda, True, what)
            continue
        # the one-kernel route on sample-major inputs; its exponential is not the leaf kernel's: the tolerance of its own tests
        K, T = host_inputs(z, dim, beta, B, 77 * seed + n)
        dK, ks, kc, dT, ts, tc = kt_on_device(cuda, K, T, "sample")
        root = torch.full((B, t.n_root), PREFILL, dtype=torch.float64, device=cuda)
        f.handle.mc_eval_device(dK.data_ptr(), ks, kc, dT.data_ptr(), ts, tc, KF, beta, LAM, root.data_ptr(), t.n_root, 1, B, st)
        torch.cuda.synchronize()
        got = root.cpu().numpy()
        if t.n_node == 0:
            assert (got[:, z["leaf_type"] == 0] == 1.0).all(), what
            check_leaves(z, got, K, T, KF, beta, LAM)
        check_against_oracle(t, z, K, T, beta, got, what)


def wide_table(L=9, R=30):
    """30 roots, all live, two levels deep: sums and products of leaves, then of leaves and the first four nodes"""
    rng = np.random.default_rng(30)
    nodes = []
    for n in range(R):
        pool = L if n < 4 else L + 4
        ch = [(int(rng.integers(0, pool)), float(rng.choice([1.0, -1.0, 0.5, 2.0]))) for _ in range(2 + n % 2)]
        nodes.append((OP_SUM if n % 3 else OP_PROD, 0, ch))
    return from_program(L, nodes, [L + n for n in range(R)], "wide_30")


def assert_close(got, want, scale, what):
    """the accumulate tests' bar: |d| <= 1e-12 max(1, scale) per entry"""
    r = np.abs(got - want) / np.maximum(1.0, scale)
    print(what, "max |d| / max(1, scale) =", float(r.max()))
    assert np.all(r <= TOL), (what, np.argwhere(~(r <= TOL))[:4], float(r.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("spec", ["isa", True])
def test_split_route_binned_calls_with_a_short_last_chunk(libfdg, cuda, spec):
    """The binned, moments and VEGAS accumulate calls cut the batch into chunks of the root scratch and run the Monte-Carlo step once per
    chunk: R = 30 with FDG_ROOT_SCRATCH_MB=1 gives chunks of 4352 samples, B = 4352 + 100 a last chunk of 100 -- a second call into the
    chunk of leaves with another leaf stride inside one entry point.  Through the split route, and through the one-kernel route on a
    second handle, with the assertions of tests/test_*_accumulate.py for each route: the sums against the host's sums over that route's
    own mc_eval_device roots at 1e-12 max(1, sum of |terms|), the moments call's first moment the bits of the binned call, the VEGAS call's
    moments the bits of the moments call without bins.  The split route's roots are the bits of the unfused sequence; the one-kernel
    route's lie within 1e-12 max(1, root scale) of them.  No bin, and no cell of the training histogram, stays empty in either chunk."""
    import torch
    from test_binned_accumulate import host_binned
    from test_moments_accumulate import assert_bits, host_moments
    from test_vegas_accumulate import host_hist
    st = torch.cuda.current_stream().cuda_stream
    t = wide_table()
    L, R = t.n_leaf, t.n_root
    z, dim, beta = with_type0(random_leaf_tables(3, L), 2), 3, 3.0
    B, n_bin, base, D, G, vseed, voff = 4352 + 100, 5, 1, 2, 4, 41, 1_000_003
    assert ((1 << 20) // (8 * R)) & ~63 == 4352
    K, T = host_inputs(z, dim, beta, B, 5)
    dK, dT = component_major(cuda, K, T)
    rng = np.random.default_rng(6)
    h_w = rng.uniform(0.5, 1.5, size=B)
    h_bins = (np.arange(B) % n_bin + base).astype(np.int32)
    h_coef = rng.uniform(-1.0, 1.0, size=R)
    w, bins = torch.from_numpy(h_w).to(cuda), torch.from_numpy(h_bins).to(cuda)
    tab, _keep = capi.make_leaf_tables(*tab_args(z, dim))
    kt = (dK.data_ptr(), 1, B, dT.data_ptr(), 1, B, KF, beta, LAM)
    f_ref = fd.compile_table(t, specialize=spec)
    unfused = unfused_roots(f_ref, z, dim, beta, dK, dT, B, st)
    assert np.isfinite(unfused).all()
    check_against_oracle(t, z, K, T, beta, unfused, "unfused")
    lv = oracle.leaf_values(*tab_args(z, 0)[:6], K, T, KF, beta, LAM)
    lv[:, z["leaf_type"] == 0] = 1.0
    root_scale = np.maximum(1.0, oracle.root_scale(t, lv))
    for route in ("split", "isa"):
        if route == "isa" and spec != "isa":
            continue                                     # (the one-kernel route belongs to the optimizing back end)
        f = fd.compile_table(t, specialize=spec, options={"FDG_MC_ROUTE": route, "FDG_ROOT_SCRATCH_MB": "1"})
        h = f.handle
        h.specialize_fused(tab)
        roots = mc_roots(h, dK, dT, beta, B, R, st)
        if route == "split":
            assert same(roots, unfused)
        else:
            assert np.all(np.abs(roots - unfused) <= TOL * root_scale)
        for hw, dw in ((h_w, w.data_ptr()), (None, 0)):
            terms = roots if hw is None else roots * hw[:, None]
            # plain accumulation
            acc = torch.zeros(R, dtype=torch.float64, device=cuda)
            h.mc_accumulate_device(*kt, dw, acc.data_ptr(), B, st)
            # binned
            accb = torch.zeros((n_bin, R), dtype=torch.float64, device=cuda)
            h.mc_accumulate_device_binned(*kt, bins.data_ptr(), base, n_bin, dw, accb.data_ptr(), B, st)
            # moments, with the bins and without
            m = torch.zeros((2, n_bin, R), dtype=torch.float64, device=cuda)
            h.mc_accumulate_device_moments(*kt, bins.data_ptr(), base, n_bin, dw, m[0].data_ptr(), m[1].data_ptr(), B, st)
            m1 = torch.zeros((2, R), dtype=torch.float64, device=cuda)
            h.mc_accumulate_device_moments(*kt, 0, 0, 1, dw, m1[0].data_ptr(), m1[1].data_ptr(), B, st)
            torch.cuda.synchronize()
            what = (spec, route, hw is None)
            assert_close(acc.cpu().numpy(), terms.sum(0), np.abs(terms).sum(0), what + ("accumulate",))
            want, scale = host_binned(roots, h_bins, n_bin, hw, base)
            assert (scale > 0).all()
            for lo, hi in ((0, 4352), (4352, B)):        # every bin has samples in both chunks
                assert len(np.unique(h_bins[lo:hi])) == n_bin
            assert_close(accb.cpu().numpy(), want, scale, what + ("binned",))
            assert_bits(m[0].cpu().numpy(), accb.cpu().numpy(), what + ("moments tie",))
            s1, a1, s2 = host_moments(roots, h_bins, n_bin, hw, base)
            assert_close(m[0].cpu().numpy(), s1, a1, what + ("moments",))
            assert_close(m[1].cpu().numpy(), s2, s2, what + ("second moments",))
            # VEGAS: both moments and the training histogram
            for coef in (None, h_coef):
                v = torch.zeros((2, R), dtype=torch.float64, device=cuda)
                hist = torch.zeros((D, G), dtype=torch.float64, device=cuda)
                h.mc_accumulate_device_vegas(*kt, dw, coef, vseed, voff, D, G, v[0].data_ptr(), v[1].data_ptr(), hist.data_ptr(), B, st)
                torch.cuda.synchronize()
                assert_bits(v.cpu().numpy(), m1.cpu().numpy(), what + ("vegas tie", coef is None))
                hwant = host_hist(roots, hw, coef, vseed, voff, D, G)
                assert (hwant > 0).all()
                assert_close(hist.cpu().numpy(), hwant, hwant, what + ("vegas histogram", coef is None))
