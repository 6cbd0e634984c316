"""Claimed tiles (option FDG_ISA_TILE_CLAIM; csrc/fdg_isa.cpp: `claim`, csrc/fdg_runtime.hip: IsaRun::plan): in the `_cl` variants of the
root-writing one-wave kernels a wave's first tile is its workgroup id and every further one comes from a returning atomic add on a counter
in the caller stream's workspace, which the host zeroes on the launch stream in front of every launch.  The counter is NOT cumulative, so
there is no base arithmetic to wrap.  One claim is good for a run of K consecutive tiles (option FDG_ISA_CLAIM_RUN at specialisation; the
library's K is 4, K = 1 is a claim per tile).  The places where "first run static, rest claimed, last claim fails" can go wrong are
batches of n - 1, n, n + 1 and 3 n + 5 runs for a grid of n workgroups -- with K = 1 that is n - 1, n, n + 1 and 3 n + 5 tiles --, the
last run begun by a single tile where it is not whole, each with a full and with a ragged (37 samples) last tile."""
import glob
import hashlib
import os
import re

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, workloads

NAN_BITS = 0x7FF8DEAD0000BEEF      # what the root buffers hold before a launch: whatever is not written keeps it


def listing(name, tmp, **options):
    d = os.path.join(str(tmp), name + "_" + "_".join(options))
    os.makedirs(d)
    fd.compile_table(workloads.get(name), specialize="isa", cache_dir=d, flags=capi.FDG_SPEC_KEEP_SOURCE, options=options)
    (src,) = glob.glob(d + "/fdg_isa_*.s")
    return open(src).read()


def without_claimed_kernels(text):
    """The listing without the text of the `_cl` kernels and without their entries in the code object's metadata."""
    keep = []
    for part in text.split("\t.text\n"):
        m = re.match(r"\t\.protected\t(\S+)\n", part)
        if m and m.group(1).endswith("_cl"):
            continue
        if part.startswith("\t.amdgpu_metadata"):
            head, *entries = part.split("  - .agpr_count")
            out = [head]
            for e in entries:
                body, sep, tail = e.partition("amdhsa.target:")
                if re.search(r"\.name: \S+_cl\n", body):
                    out.append(sep + tail)
                else:
                    out.append("  - .agpr_count" + e)
            part = "".join(out)
        keep.append(part)
    return "\t.text\n".join(keep)


@pytest.mark.parametrize("name", ["parquet_sigma2", "parquet_sigma4"])
def test_the_claimed_kernels_assemble_and_the_printers_offsets_hold(name, tmp_path):
    """FDG_ISA_CHECK_OFF makes the assembler hold the printer's running offset against its own location counter every 32 instructions
    (assembling fails on a mismatch): the claim's three instructions at the head of a tile and the two at the back edge are sized like
    every other.  The listing passes the hazard table, which knows the returning atomic as a memory operation that writes a VGPR."""
    text = listing(name, tmp_path, FDG_ISA_CHECK_OFF="1")
    for k in ("fdg_isa_eval_cl", "fdg_isa_eval_nt_cl"):
        body = text.split("\t.protected\t" + k + "\n")[1].split("\t.text\n")[0]
        assert body.count("Emit::off is wrong") >= 1, k
        assert body.count("global_atomic_add ") == 1 and body.count("v_readfirstlane_b32 ") == 1, k
    rc, report = capi.isa_check_hazards(listing(name, tmp_path))
    assert rc == 0, report[:2000]


# sha256 of the whole listing as the commit before the claimed kernels printed it (default options)
PARENT_LISTING = {"parquet_sigma2": "b19b88278dcbd74bce3cf004796d294bd069fa87e8191eab385a8767303bc970",
                  "parquet_sigma4": "1b7ec1fb2e9aa88b7c26106277f2520bffd8addc1c6ffa14015cc1f7b2f387ab"}


@pytest.mark.parametrize("name", sorted(PARENT_LISTING))
def test_everything_but_the_claimed_kernels_is_the_text_it_was(name, tmp_path):
    """The claimed kernels stand behind every other kernel of the code object; with their text and their metadata entries taken out, the
    listing is byte for byte what the emitter printed before it knew them -- the static walk's kernels, which every launch with the option
    off uses, have not changed.  (A change that means to alter the other kernels pins new digests here.)"""
    text = listing(name, tmp_path)
    assert "\t.protected\tfdg_isa_eval_cl\n" in text and "\t.protected\tfdg_isa_eval_nt_cl\n" in text
    assert hashlib.sha256(without_claimed_kernels(text).encode()).hexdigest() == PARENT_LISTING[name]


# ---- on the device ------------------------------------------------------------------------------------------------------------------------

class Case:
    """One graph on the device: the handle, the grid n of a memory-bound launch, a tile-major batch of 3 n + 5 tiles and, computed once,
    the static walk's roots for it (a tile's roots do not depend on the batch size, so every smaller batch is held against a prefix)."""

    def __init__(self, name, run, dev):
        import torch
        self.t = workloads.get(name)
        self.K = run
        self.f = fd.compile_table(self.t, specialize="isa", options={"FDG_ISA_TILE_CLAIM": "1", "FDG_ISA_CLAIM_RUN": str(run)})
        L, R = self.t.n_leaf, self.t.n_root
        st = torch.cuda.current_stream().cuda_stream
        probe = torch.zeros((16384, L, 64), dtype=torch.float64, device=dev)      # more tiles than any grid: the launch shows the grid
        self.f.eval_tiled(None, probe)
        torch.cuda.synchronize()
        ki = self.f.kernel_info()
        assert ki["tile_walk"] == "claimed" and ki["last_kernel"] == "fdg_isa_eval_nt", ki
        self.n = ki["last_grid"]
        assert 0 < self.n < 16384 // 4
        del probe
        self.T = self.tiles("3n+5")
        self.leaf = torch.empty((self.T, L, 64), dtype=torch.float64, device=dev)
        capi.fill_uniform_device_tiled(self.leaf.data_ptr(), 64 * self.T, L, 1, 64, 64 * L, 77, 0, st)
        self.f.handle.set_option("FDG_ISA_TILE_CLAIM", "0")
        self.static = self.fresh_roots()
        self.f.eval_tiled(self.static, self.leaf, 64 * self.T)
        torch.cuda.synchronize()
        assert self.f.kernel_info()["last_kernel"] == "fdg_isa_eval_nt" and self.f.kernel_info()["tile_walk"] == "static"
        self.f.handle.set_option("FDG_ISA_TILE_CLAIM", "1")
        self.static_bits = self.static.view(torch.int64)

    def fresh_roots(self):
        """root buffer of the whole batch and two tiles more, every word the NaN pattern"""
        import torch
        bits = torch.full((self.T + 2, self.t.n_root, 64), NAN_BITS, dtype=torch.int64, device=self.leaf.device)
        return bits.view(torch.float64)

    def tiles(self, size):
        """tiles of a batch of n - 1, n, n + 1, 3 n + 5 runs (the last two end in a run of one tile when K > 1)"""
        K, n = self.K, self.n
        return {"n-1": K * (n - 1), "n": K * n, "n+1": K * n + 1, "3n+5": K * (3 * n + 4) + 1}[size]

    def grid(self, T):
        return min((T + self.K - 1) // self.K, self.n)

    def check(self, root, B, what):
        """the first B samples carry the static walk's bits; lanes past B and tiles past the end keep the pattern"""
        import torch
        got = root.view(torch.int64)
        full, rest = B // 64, B % 64
        assert torch.equal(got[:full], self.static_bits[:full]), what
        if rest:
            assert torch.equal(got[full, :, :rest], self.static_bits[full, :, :rest]), what
            assert bool((got[full, :, rest:] == NAN_BITS).all()), what + ": lanes past the batch were written"
        assert bool((got[full + (1 if rest else 0):] == NAN_BITS).all()), what + ": tiles past the batch were written"


_cases = {}


@pytest.fixture
def case(request, libfdg, cuda):
    key = request.param
    if key not in _cases:
        _cases[key] = Case(key[0], key[1], cuda)
    return _cases[key]


# (graph, tiles per claim): a claim per tile and the library's run on the small graph, the headline graph once
SIZES = ([(("parquet_sigma2", K), s, r) for K in (1, 4) for s in ("n-1", "n", "n+1", "3n+5") for r in (False, True)] +
         [(("parquet_sigma4", 4), "3n+5", True)])


@pytest.mark.gpu
@pytest.mark.parametrize("case,size,ragged", SIZES, indirect=["case"])
def test_claimed_walk_gives_the_static_walks_and_the_oracles_bits(case, size, ragged):
    """Three launches in a row into three buffers (the counter is zeroed in front of each), every one bit-equal to the static walk's roots,
    nothing written behind the batch; a sample of the rows -- the last tile's among them -- against the oracle."""
    import torch
    import oracle
    T = case.tiles(size)
    B = 64 * (T - 1) + 37 if ragged else 64 * T
    roots = [case.fresh_roots() for _ in range(3)]
    for r in roots:
        case.f.eval_tiled(r, case.leaf, B)
    torch.cuda.synchronize()
    ki = case.f.kernel_info()
    assert ki["tile_walk"] == "claimed" and ki["last_grid"] == case.grid(T), ki
    for i, r in enumerate(roots):
        case.check(r, B, f"{size} ragged={ragged} launch {i}")
    rng = np.random.default_rng(5)
    rows = np.unique(np.concatenate([rng.integers(0, B, 200), np.arange(max(0, B - 70), B), np.arange(0, 64)]))
    idx = torch.from_numpy(rows).to(case.leaf.device)
    h_leaf = case.leaf[idx // 64, :, idx % 64].cpu().numpy()
    got = roots[0][idx // 64, :, idx % 64].cpu().numpy()
    assert np.array_equal(got, oracle.eval_static(case.t, np.ascontiguousarray(h_leaf)))


@pytest.mark.gpu
@pytest.mark.parametrize("case,size,ragged", SIZES, indirect=["case"])
def test_two_streams_on_one_handle_claim_from_their_own_counters(case, size, ragged):
    """Launches of one handle on two streams at once: each stream's workspace has its own counter, so neither sees the other's claims."""
    import torch
    T = case.tiles(size)
    B = 64 * (T - 1) + 37 if ragged else 64 * T
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    roots = [[case.fresh_roots() for _ in range(3)] for _ in streams]
    torch.cuda.synchronize()
    for k in range(3):
        for s, st in enumerate(streams):
            with torch.cuda.stream(st):
                case.f.eval_tiled(roots[s][k], case.leaf, B)
    torch.cuda.synchronize()
    assert case.f.kernel_info()["tile_walk"] == "claimed"
    for s in range(2):
        for k in range(3):
            case.check(roots[s][k], B, f"{size} ragged={ragged} stream {s} launch {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("case,size,ragged", SIZES, indirect=["case"])
def test_claimed_and_static_walks_alternate_on_one_handle(case, size, ragged):
    """The option switches the walk per call: kernel_info tells the walk each call used (the variant's name stays), and the bits do not change."""
    import torch
    T = case.tiles(size)
    B = 64 * (T - 1) + 37 if ragged else 64 * T
    try:
        for k in range(4):
            claimed = k % 2 == 0
            case.f.handle.set_option("FDG_ISA_TILE_CLAIM", "1" if claimed else "0")
            root = case.fresh_roots()
            case.f.eval_tiled(root, case.leaf, B)
            torch.cuda.synchronize()
            ki = case.f.kernel_info()
            assert ki["last_kernel"] == "fdg_isa_eval_nt" and ki["tile_walk"] == ("claimed" if claimed else "static")
            case.check(root, B, f"{size} ragged={ragged} call {k} claimed={claimed}")
    finally:
        case.f.handle.set_option("FDG_ISA_TILE_CLAIM", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("parquet_sigma2", 4)], indirect=True)
def test_a_matrix_batch_claims_its_tiles_too(case):
    """A leaf-major matrix (not tile-major, ragged): the same launch path, the plain or streaming claimed kernel, the static walk's bits."""
    import torch
    L, R = case.t.n_leaf, case.t.n_root
    B = 64 * (case.tiles("3n+5") - 1) + 37
    leaf = torch.rand((L, B), dtype=torch.float64, device=case.leaf.device).t()
    out = {}
    try:
        for claim in ("0", "1"):
            case.f.handle.set_option("FDG_ISA_TILE_CLAIM", claim)
            root = torch.full((R, B), float("nan"), dtype=torch.float64, device=leaf.device).t()
            case.f(root, leaf)
            torch.cuda.synchronize()
            assert case.f.kernel_info()["tile_walk"] == ("claimed" if claim == "1" else "static")
            out[claim] = root
    finally:
        case.f.handle.set_option("FDG_ISA_TILE_CLAIM", "1")
    assert not bool(torch.isnan(out["1"]).any())
    assert torch.equal(out["0"], out["1"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("parquet_sigma2", 4)], indirect=True)
def test_claimed_launches_are_graph_capturable(case):
    """The counter's reset is a memset on the launch stream: a captured graph holds it as a node in front of the kernel, so every replay
    starts from zero like the eager call (nothing allocated, nothing waited for once the handle is warm)."""
    import torch
    B = 64 * (case.tiles("3n+5") - 1) + 37
    roots = [case.fresh_roots() for _ in range(2)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        case.f.eval_tiled(roots[0], case.leaf, B)          # warm-up on this stream: its workspace exists
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for r in roots:
                case.f.eval_tiled(r, case.leaf, B)
        assert case.f.kernel_info()["tile_walk"] == "claimed"
        for k in range(3):
            for r in roots:
                r.view(torch.int64).fill_(NAN_BITS)
            g.replay()
            torch.cuda.synchronize()
            for i, r in enumerate(roots):
                case.check(r, B, f"replay {k} launch {i}")
