"""Evaluation and fused accumulation at the thresholds where the optimizing back end changes kernel variant.

csrc/fdg_runtime.hip builds up to eleven variants per graph and picks among them by the graph's leaf count L and root count R:

 * build_acc_program: R <= 40 accumulators in value registers (reserve_pairs = R + 2, a further register condition from R = 17 on);
   41 <= R <= 124 accumulators in AGPR pairs (n_acc_used + R <= 124: at R = 124 the AGPR file has no spill slot left); R > 124 no fused
   kernel, the sum goes through the column-major root scratch and fdg_weighted_partials;
 * build_variants / build_rl: the row-major accumulating kernels _rm_acc / _rl_acc are built for R <= 40 only;
 * build_rm_program: no row-major variant below L = 16; two waves per SIMD with two staging buffers up to (L + 15) / 16 = 8 chunks,
   four buffers and one wave beyond;
 * build_rl: the linear row-major variant while a 64-row tile fits 160 KiB / 3 - 4 KiB (L <= 98).

The sweep below puts one graph on either side of each edge (synthetic_parquet_like, seed 5), so that an off-by-one in a rule and a kernel
that is wrong only at its family's extreme shape (one chunk at L = 16, the longest two-buffer row at L = 128, rows that end on the
half-wave last load at L = 17, 99, 129, 42 reserved register pairs at R = 40, no AGPR spill slot at R = 124) both show.  Two more shapes
cross L = 99 with R = 40 / 41 (the R <= 40 rule of _rm_acc away from the linear variant), and the AGPR shapes R = 41 and R = 124 come once
more with one root slot absent (FDG_NO_ROOT): the rules count slots, so those kernels must skip an accumulator they have reserved.

The shapes, their flags (kernel_info() after FDG_SPEC_ISA, no tuned choice) and the kernel each call takes on whole tiles (B >= 64; the
last B % 64 rows and every batch below 64 go through the plain kernels, fdg_isa_eval / fdg_isa_eval_acc):

  id        n_node arg  nodes  L    R    has_acc has_rm has_rl rm_bufs waves_per_cu | eval: rows  padded rows | accumulate: rows  padded rows
  L15       300         286    15   2    1       0      1      0       8/8/0        | _rl         plain       | _rl_acc           _acc
  L16       300         275    16   2    1       1      1      2       8/8/8        | _rl         _rm         | _rl_acc           _rm_acc
  L17       300         275    17   2    1       1      1      2       8/8/8        | _rl         _rm         | _rl_acc           _rm_acc
  L98       300         291    98   2    1       1      1      2       8/8/8        | _rl         _rm         | _rl_acc           _rm_acc
  L99       300         295    99   2    1       1      0      2       8/8/8        | _rm         _rm         | _rm_acc           _rm_acc
  L128      300         321    128  2    1       1      0      2       8/8/8        | _rm         _rm         | _rm_acc           _rm_acc
  L129      300         330    129  2    1       1      0      4       8/8/5        | _rm         _rm         | _rm_acc           _rm_acc
  R16       1500        1474   40   16   1       1      1      4       8/8/4        | _rl         _rm         | _rl_acc           _rm_acc
  R17       1500        1475   40   17   1       1      1      4       8/8/4        | _rl         _rm         | _rl_acc           _rm_acc
  R40       1500        1498   40   40   1       1      1      4       8/8/4        | _rl         _rm         | _rl_acc           _rm_acc
  R41       1500        1499   40   41   1       1      1      4       8/4/4        | _rl         _rm         | _acc              _acc
  R124      1500        1582   40   124  1       1      1      4       8/4/4        | _rl         _rm         | _acc              _acc
  R125      1500        1583   40   125  0       1      1      4       8/0/4        | _rl         _rm         | plain + partials  plain + partials
  L99-R40   1500        1548   99   40   1       1      0      4       8/8/4        | _rm         _rm         | _rm_acc           _rm_acc
  L99-R41   1500        1549   99   41   1       1      0      4       8/4/4        | _rm         _rm         | _acc              _acc
  R41-absent, R124-absent: the R41 and R124 rows with root slot R // 2 absent.

Leaf-major and tile-major batches take the plain kernels at every shape: fdg_isa_eval[_nt], and fdg_isa_eval_acc[_nt] where has_acc.  No
shape has the pooled or the cooperative variant, so the rules above decide alone.

The CPU part needs no device: the flags still straddle their edges, every listing is clean against the emitter's wait-state table, the
allocated one-wave program replays to the oracle's bits.  The GPU part runs every shape in every layout at B in {1, 63, 64, 65, 337}:
every path here is decided by L, R and whether B reaches 64."""
import dataclasses
import glob
import os
import re

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT, synthetic_parquet_like
from test_next_rows import replay
from test_random_graphs import same
from test_tile_major import from_tiles, to_tiles

TOL = 1e-12                        # tests/test_gpu_parity.py: |d| <= TOL * max(1, sum |w root|) per root
BATCHES = (1, 63, 64, 65, 64 * 5 + 17)
PLAIN = ("fdg_isa_eval", "fdg_isa_eval_nt")
PLAIN_ACC = ("fdg_isa_eval_acc", "fdg_isa_eval_acc_nt")


@dataclasses.dataclass(frozen=True)
class Shape:
    n_node: int
    L: int
    R: int
    absent: bool = False


SWEEP = {f"L{L}": Shape(300, L, 2) for L in (15, 16, 17, 98, 99, 128, 129)}
SWEEP.update({f"R{R}": Shape(1500, 40, R) for R in (16, 17, 40, 41, 124, 125)})
SWEEP.update({"L99-R40": Shape(1500, 99, 40), "L99-R41": Shape(1500, 99, 41)})
SWEEP.update({"R41-absent": Shape(1500, 40, 41, True), "R124-absent": Shape(1500, 40, 124, True)})

# (what differs, the shape on either side of the edge)
STRADDLES = [("has_rm", "L15", "L16"), ("has_rl", "L98", "L99"), ("rm_bufs", "L128", "L129"), ("has_acc", "R124", "R125"),
             ("acc_waves_per_cu", "R40", "R41"), ("rl_acc_built", "R40", "R41"), ("rm_acc_built", "L99-R40", "L99-R41")]

_TABLES, _SPECS = {}, {}


def table(sid):
    if sid not in _TABLES:
        s = SWEEP[sid]
        t = synthetic_parquet_like(n_node=s.n_node, n_leaf=s.L, n_root=s.R, seed=5)
        assert (t.n_leaf, t.n_root) == (s.L, s.R)
        if s.absent:
            slot = t.root_slot.copy()
            slot[s.R // 2] = FDG_NO_ROOT
            t = dataclasses.replace(t, root_slot=slot, name=f"{t.name}:absent")
        _TABLES[sid] = t
    return _TABLES[sid]


def leaves(B, L, seed):
    return oracle.philox_uniform(B, L, seed) * 2 - 0.5


@pytest.fixture(scope="module")
def specialised(libfdg, tmp_path_factory):
    """sid -> (function, kernel_info, listings, names of the kernels in the listings): each shape specialised once, into a cache directory
    of its own, without the shipped code objects and without a remembered tuner's choice"""
    def get(sid):
        if sid not in _SPECS:
            d = tmp_path_factory.mktemp(sid.replace("-", "_"))
            os.chmod(d, 0o700)
            f = fd.compile_table(table(sid), specialize="isa", cache_dir=str(d), flags=capi.FDG_SPEC_KEEP_SOURCE,
                                 options={"FDG_CACHE_RO_DIR": "", "FDG_IGNORE_TUNED": "1"})
            texts = [open(p).read() for p in sorted(glob.glob(os.path.join(str(d), "*.s")))]
            names = {n for x in texts for n in re.findall(r"^\s*\.globl\s+(\S+)", x, re.M)}
            _SPECS[sid] = (f, f.kernel_info(), texts, names)
        return _SPECS[sid]
    return get


def flag(spec, what):
    _, ki, _, names = spec
    if what == "acc_waves_per_cu":
        return ki["waves_per_cu"][1]
    if what.endswith("_built"):
        return int("fdg_isa_eval_" + what[:-len("_built")] in names)
    return ki[what]


# --------------------------------------------------------------------------- #
# CPU part
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("what,below,above", STRADDLES)
def test_sweep_still_straddles_the_threshold(specialised, what, below, above):
    a, b = flag(specialised(below), what), flag(specialised(above), what)
    assert a != b, (f"{what} is {a} at {below} and at {above}: a threshold has moved.  Move the pair of shapes to the new edge "
                    f"(SWEEP, STRADDLES and the table in this file's docstring) rather than delete the case")


@pytest.mark.parametrize("sid", list(SWEEP))
def test_every_shape_specialises_with_the_named_kernels_only(specialised, sid):
    """The expectations of the GPU part are written for handles whose row and accumulate variants are the only ones beside the plain kernels."""
    _, ki, texts, names = specialised(sid)
    assert texts, "FDG_SPEC_KEEP_SOURCE left no listing"
    assert ki["has_pool"] == 0 and ki["has_coop"] == 0 and "fdg_isa_eval_w2" not in names, (ki, sorted(names))
    assert ("fdg_isa_eval_acc" in names) == bool(ki["has_acc"]) and ("fdg_isa_eval_rm" in names) == bool(ki["has_rm"])
    assert ("fdg_isa_eval_rl" in names) == bool(ki["has_rl"]) and (ki["rm_bufs"] > 0) == bool(ki["has_rm"])
    # csrc/fdg_runtime.hip, build_variants: "if (V.rm_bufs && V.acc && g->prog.R >= 1 && g->prog.R <= 40 && ...)", build_rl likewise
    R = SWEEP[sid].R
    assert ("fdg_isa_eval_rm_acc" in names) == bool(ki["has_rm"] and ki["has_acc"] and R <= 40), sorted(names)
    assert ("fdg_isa_eval_rl_acc" in names) == bool(ki["has_rl"] and ki["has_acc"] and R <= 40), sorted(names)


@pytest.mark.parametrize("sid", list(SWEEP))
def test_listings_are_clean_against_the_hazard_table(specialised, sid):
    for text in specialised(sid)[2]:
        n, rep = capi.isa_check_hazards(text)
        assert n == 0, rep


@pytest.mark.parametrize("sid", list(SWEEP))
def test_allocated_program_replays_to_the_oracle(specialised, sid):
    f = specialised(sid)[0]
    t = table(sid)
    leaf = leaves(7, t.n_leaf, 11)
    ops, nr, nl, nm = f.handle.opt_program()
    got = replay(ops, nr, nl, nm, f.handle.last_n_acc, leaf, t.n_root)
    live = t.root_slot != FDG_NO_ROOT
    assert same(got[:, live], oracle.eval_static(t, leaf)[:, live])


# --------------------------------------------------------------------------- #
# GPU part
# --------------------------------------------------------------------------- #
def expected_eval_kernel(ki, rows, B):
    """run_isa / fdg_run_locked: whole tiles of contiguous rows take the linear variant when there is one, rows of any pitch the chunked one;
    a batch below one tile, and a graph without a row variant, goes through the transposition in front of the plain kernel (row-major roots
    have sample stride R: launch_isa's line_aligned(rt1, rrs, rrk) fails and the streaming twin is not taken)"""
    if B >= 64 and rows == "contiguous" and ki["has_rl"]:
        return ("fdg_isa_eval_rl",)
    if B >= 64 and ki["has_rm"]:
        return ("fdg_isa_eval_rm",)
    return ("fdg_isa_eval",)


def expected_acc_kernel(ki, R, rows, B):
    """fdg_run_locked: "rl_shape = rl_rows && (... (mode == 1 && g->kern[FDG_K_RL_ACC].present && g->kern[FDG_K_ACC].present ...))";
    IsaRun::wants_rm: "(fused_acc && K(FDG_K_RM_ACC).present && K(FDG_K_RM_ACC).fn)"; both kernels are built for R <= 40 only
    (build_variants, build_rl: "g->prog.R >= 1 && g->prog.R <= 40"), and only next to the fused kernel ("V.rl && V.acc", "V.rm_bufs && V.acc")"""
    if B >= 64 and R <= 40 and ki["has_acc"]:
        if rows == "contiguous" and ki["has_rl"]:
            return ("fdg_isa_eval_rl_acc",)
        if ki["has_rm"]:
            return ("fdg_isa_eval_rm_acc",)
    return PLAIN_ACC if ki["has_acc"] else PLAIN


def check_acc(got, acc0, terms, live, what):
    """|d| <= TOL * max(1, sum |w root| + |acc0|) per live root; an absent root's entry keeps its bits"""
    want = acc0 + terms.sum(0)
    scale = np.maximum(1.0, np.abs(terms).sum(0) + np.abs(acc0))
    d = np.abs(got - want)
    assert np.all(d[live] <= TOL * scale[live]), (what, int(np.argmax(d / scale)), float((d / scale)[live].max()))
    assert np.array_equal(got[~live].view(np.uint64), acc0[~live].view(np.uint64)), (what, "absent root's entry written")


@pytest.mark.gpu
@pytest.mark.parametrize("sid", list(SWEEP))
def test_eval_and_accumulate_in_every_layout_on_device(libfdg, cuda, sid):
    import torch
    t = table(sid)
    L, R = t.n_leaf, t.n_root
    live = t.root_slot != FDG_NO_ROOT
    f = fd.compile_table(t, specialize="isa")
    ki = f.kernel_info()
    assert ki["has_pool"] == 0 and ki["has_coop"] == 0, ki
    last = lambda: f.kernel_info()["last_kernel"]
    for B in BATCHES:
        T = (B + 63) // 64
        h_leaf = leaves(B, L, 100 + B)
        want = oracle.eval_static(t, h_leaf, np.full((B, R), 9.0))
        assert np.isfinite(want).all() and (want[:, ~live] == 9.0).all()
        rng = np.random.default_rng(B)
        h_w, acc0 = rng.uniform(0.5, 1.5, B), rng.uniform(-3.0, 3.0, R)
        d_w = torch.from_numpy(h_w).to(cuda)
        pad = torch.full((B, L + 3), float("nan"), dtype=torch.float64, device=cuda)
        pad[:, :L] = torch.from_numpy(h_leaf).to(cuda)
        layouts = {"leaf-major": torch.from_numpy(np.ascontiguousarray(h_leaf.T)).to(cuda).t(),
                   "contiguous": torch.from_numpy(h_leaf).to(cuda), "padded": pad[:, :L]}
        tiles = torch.from_numpy(to_tiles(h_leaf)).to(cuda)

        # ---- evaluation: the oracle's bits, 9.0 left in an absent root's column ----
        for lay, leaf in layouts.items():
            root = torch.full((B, R), 9.0, dtype=torch.float64, device=cuda)
            f(root, leaf)
            torch.cuda.synchronize()
            k = last()
            assert same(root.cpu().numpy(), want), (sid, lay, B, k)
            assert k in (PLAIN if lay == "leaf-major" else expected_eval_kernel(ki, lay, B)), (sid, lay, B, k)
        if B == BATCHES[-1]:                  # a Julia B x R matrix next to row-major leaves, once per shape
            for lay in ("contiguous", "padded"):
                root = torch.full((R, B), 9.0, dtype=torch.float64, device=cuda).t()
                f(root, layouts[lay])
                torch.cuda.synchronize()
                assert same(root.cpu().numpy(), want), (sid, lay, B, "column-major roots", last())
        rt = torch.full((T, R, 64), 9.0, dtype=torch.float64, device=cuda)
        f.eval_tiled(rt, tiles, B)
        torch.cuda.synchronize()
        h_rt = rt.cpu().numpy()
        assert same(from_tiles(h_rt, B, R), want), (sid, "tile-major", B, last())
        assert (h_rt.transpose(0, 2, 1).reshape(-1, R)[B:] == 9.0).all(), (sid, "tile-major", B, "lanes behind the batch written")
        assert last() in PLAIN, (sid, "tile-major", B, last())

        # ---- accumulation on top of what acc holds, with weights and with weight NULL = 1 ----
        for weighted in (True, False):
            terms = np.where(live[None, :], want, 0.0) * (h_w[:, None] if weighted else 1.0)
            w = d_w if weighted else None
            for lay, leaf in layouts.items():
                acc = torch.from_numpy(acc0).to(cuda)
                f.accumulate(leaf, w, acc)
                torch.cuda.synchronize()
                k = last()
                check_acc(acc.cpu().numpy(), acc0, terms, live, (sid, lay, B, weighted, k))
                if lay == "leaf-major":
                    assert k in (PLAIN_ACC if ki["has_acc"] else PLAIN), (sid, lay, B, k)
                else:
                    assert k in expected_acc_kernel(ki, R, lay, B), (sid, lay, B, k)
                assert ("_acc" in k) == bool(ki["has_acc"]), (sid, lay, B, k)
            acc = torch.from_numpy(acc0).to(cuda)
            f.accumulate_tiled(tiles, w, acc, B)
            torch.cuda.synchronize()
            check_acc(acc.cpu().numpy(), acc0, terms, live, (sid, "tile-major", B, weighted, last()))
            assert last() in (PLAIN_ACC if ki["has_acc"] else PLAIN), (sid, "tile-major", B, last())


@pytest.mark.gpu
@pytest.mark.parametrize("n_bin", [1, 5])
@pytest.mark.parametrize("sid", ["R17", "R125"])
def test_moments_at_the_root_slice_and_the_unfused_edge(libfdg, cuda, sid, n_bin):
    """R = 17: one full slice of sixteen roots plus a slice of one; R = 125: the first root count without a fused kernel.  First and second
    moments against the host binning of the oracle's roots, |d| <= TOL * max(1, sum over the bin of |t|, resp. of t * t)."""
    import torch
    t = table(sid)
    L, R, B = t.n_leaf, t.n_root, BATCHES[-1]
    f = fd.compile_table(t, specialize="isa")
    h_leaf = leaves(B, L, 100 + B)
    roots = oracle.eval_static(t, h_leaf)
    rng = np.random.default_rng(n_bin)
    h_w = rng.uniform(-1.0, 2.0, B)
    if n_bin == 1:
        h_bins, j = None, np.zeros(B, dtype=np.int64)
    else:                                    # a few samples out of range on either side: they add nothing
        h_bins = rng.integers(-1, n_bin + 1, size=B).astype(np.int32)
        j = h_bins.astype(np.int64)
    ok = (j >= 0) & (j < n_bin)
    terms = roots[ok] * h_w[ok, None]
    s1, a1, s2 = np.zeros((n_bin, R)), np.zeros((n_bin, R)), np.zeros((n_bin, R))
    np.add.at(s1, j[ok], terms)
    np.add.at(a1, j[ok], np.abs(terms))
    np.add.at(s2, j[ok], terms * terms)
    d_w = torch.from_numpy(h_w).to(cuda)
    d_bins = None if h_bins is None else torch.from_numpy(h_bins).to(cuda)
    batches = {"leaf-major": torch.from_numpy(np.ascontiguousarray(h_leaf.T)).to(cuda).t(), "contiguous": torch.from_numpy(h_leaf).to(cuda),
               "tile-major": torch.from_numpy(to_tiles(h_leaf)).to(cuda)}
    for lay, leaf in batches.items():
        acc, acc2 = f.accumulate_moments(leaf, d_bins, n_bin, d_w, n_sample=B)
        torch.cuda.synchronize()
        for got, ref, scale, what in ((acc, s1, a1, "acc"), (acc2, s2, s2, "acc2")):
            d = np.abs(got.cpu().numpy() - ref)
            assert np.all(d <= TOL * np.maximum(1.0, scale)), (sid, lay, n_bin, what, float(d.max()))
