"""Resident waves of the claimed walk (csrc/fdg_runtime.hip: IsaRun::mem_waves_of, grid_cl): where the launch plan takes the `_cl` twin of a
root-writing one-wave kernel of a graph with 24 leaves or more, the grid is THREE workgroups per CU instead of the static walk's four
(DESIGN.md 6a); FDG_ISA_MEM_WAVES still overrides both, the static walk and the graphs below 24 leaves keep their grids, and the library's
rule decides on the static walk's grid which launches claim (256 rounds of it).  A smaller grid moves every boundary of "first run by
workgroup id, the rest claimed, the last claims past the end": batches of n - 1, n, n + 1 and 3 n + 5 runs for the new n, full and with a
ragged last tile, are held bit for bit against the oracle (computed once, over the whole largest batch: a tile's roots do not depend on the
batch) and against the static walk."""
import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import workloads

NAN_BITS = 0x7FF8DEAD0000BEEF      # what the root buffers hold before a launch: whatever is not written keeps it
K = 4                              # tiles per claim (the library's run)
_state = {}


def headline(dev):
    """parquet_sigma4 on the device with the claim forced: the grid n of its claimed walk, a tile-major batch of 3 n + 5 runs and the
    oracle's roots for all of it as int64 bit patterns on the device"""
    if not _state:
        import torch
        import oracle
        from feynmandiagram_jl_amd import capi
        t = workloads.get("parquet_sigma4")
        f = fd.compile_table(t, specialize="isa", options={"FDG_ISA_TILE_CLAIM": "1"})
        L, R = t.n_leaf, t.n_root
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        T = K * (3 * 3 * n_cu + 4) + 1
        leaf = torch.empty((T, L, 64), dtype=torch.float64, device=dev)
        capi.fill_uniform_device_tiled(leaf.data_ptr(), 64 * T, L, 1, 64, 64 * L, 77, 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        h_leaf = np.ascontiguousarray(leaf.cpu().numpy().transpose(0, 2, 1).reshape(-1, L))
        want = oracle.eval_static(t, h_leaf).reshape(T, 64, R).transpose(0, 2, 1)
        _state.update(t=t, f=f, n_cu=n_cu, T=T, leaf=leaf, want=torch.from_numpy(np.ascontiguousarray(want)).to(dev).view(torch.int64))
    return _state


def fresh_roots(s):
    import torch
    return torch.full((s["T"] + 2, s["t"].n_root, 64), NAN_BITS, dtype=torch.int64, device=s["leaf"].device).view(torch.float64)


def check(s, root, B, what):
    """the first B samples carry the oracle's bits; lanes past B and tiles past the end keep the pattern"""
    import torch
    got = root.view(torch.int64)
    full, rest = B // 64, B % 64
    assert torch.equal(got[:full], s["want"][:full]), what
    if rest:
        assert torch.equal(got[full, :, :rest], s["want"][full, :, :rest]), what
        assert bool((got[full, :, rest:] == NAN_BITS).all()), what + ": lanes past the batch were written"
    assert bool((got[full + (1 if rest else 0):] == NAN_BITS).all()), what + ": tiles past the batch were written"


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("size", ["1 tile", "n-1", "n", "n+1", "3n+5"])
def test_claimed_walk_from_three_waves_gives_the_oracles_bits(libfdg, cuda, size, ragged):
    import torch
    s = headline(cuda)
    n = 3 * s["n_cu"]
    T = {"1 tile": 1, "n-1": K * (n - 1), "n": K * n, "n+1": K * n + 1, "3n+5": K * (3 * n + 4) + 1}[size]
    B = 64 * (T - 1) + 37 if ragged else 64 * T
    f = s["f"]
    out = {}
    try:
        for claim in ("1", "0"):
            f.handle.set_option("FDG_ISA_TILE_CLAIM", claim)
            out[claim] = fresh_roots(s)
            f.eval_tiled(out[claim], s["leaf"], B)
            torch.cuda.synchronize()
            ki = f.kernel_info()
            assert ki["last_kernel"] == "fdg_isa_eval_nt" and ki["tile_walk"] == ("claimed" if claim == "1" else "static"), ki
            assert ki["last_grid"] == (min((T + K - 1) // K, n) if claim == "1" else min(T, 4 * s["n_cu"])), ki
    finally:
        f.handle.set_option("FDG_ISA_TILE_CLAIM", "1")
    check(s, out["1"], B, f"{size} ragged={ragged} claimed")
    check(s, out["0"], B, f"{size} ragged={ragged} static")


@pytest.mark.gpu
def test_the_option_overrides_the_claimed_walks_waves_and_small_graphs_keep_theirs(libfdg, cuda):
    """FDG_ISA_MEM_WAVES sets the resident waves of both walks (4: the grid the claimed walk had); with it removed the rule is back.  A graph
    below 24 leaves claims from the five waves per CU of its static walk."""
    import torch
    s = headline(cuda)
    f, B = s["f"], 64 * s["T"]
    try:
        for waves, grid in (("4", 4), ("2", 2), (None, 3)):
            f.handle.set_option("FDG_ISA_MEM_WAVES", waves)
            root = fresh_roots(s)
            f.eval_tiled(root, s["leaf"], B)
            torch.cuda.synchronize()
            ki = f.kernel_info()
            assert ki["tile_walk"] == "claimed" and ki["last_grid"] == grid * s["n_cu"], (waves, ki)
            check(s, root, B, f"FDG_ISA_MEM_WAVES={waves}")
    finally:
        f.handle.set_option("FDG_ISA_MEM_WAVES", None)
    t = workloads.get("parquet_sigma2")
    assert t.n_leaf < 24
    g = fd.compile_table(t, specialize="isa")
    leaf = torch.zeros((16384, t.n_leaf, 64), dtype=torch.float64, device=cuda)
    grids = {}
    for claim in ("0", "1"):
        g.handle.set_option("FDG_ISA_TILE_CLAIM", claim)
        g.eval_tiled(None, leaf)
        torch.cuda.synchronize()
        ki = g.kernel_info()
        assert ki["tile_walk"] == ("claimed" if claim == "1" else "static"), ki
        grids[claim] = ki["last_grid"]
    assert grids["0"] == grids["1"] == 5 * s["n_cu"], grids


@pytest.mark.gpu
def test_the_rule_counts_its_rounds_on_the_static_walks_grid(libfdg, cuda):
    """With FDG_ISA_TILE_CLAIM unset a launch claims from 256 rounds of the static walk's grid (4 waves per CU) on, as before the claimed walk
    had a grid of its own: one tile fewer keeps the static walk and its grid.  (Walks only: the leaves are whatever the allocation holds.)"""
    import torch
    s = headline(cuda)
    t = s["t"]
    f = fd.compile_table(t, specialize="isa")
    T = 256 * 4 * s["n_cu"]
    leaf = torch.empty((T, t.n_leaf, 64), dtype=torch.float64, device=cuda)
    root = torch.empty((T, t.n_root, 64), dtype=torch.float64, device=cuda)
    for tiles, walk, grid in ((T, "claimed", 3), (T - 1, "static", 4)):
        f.eval_tiled(root, leaf, 64 * tiles)
        torch.cuda.synchronize()
        ki = f.kernel_info()
        assert ki["last_kernel"] == "fdg_isa_eval_nt" and ki["tile_walk"] == walk and ki["last_grid"] == grid * s["n_cu"], (tiles, ki)
    del leaf, root
    torch.cuda.empty_cache()      # (11 GB: not kept for the rest of the session)
