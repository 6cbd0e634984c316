"""Power{N} nodes at the edges of fp64, on every back end and in every kernel variant of the optimizing one.

For N outside {2, 3} every back end spells out Julia's pow_body: csrc/fdg_powi.h (the interpreter), the prelude of csrc/fdg_emit.cpp (the
HIP-source kernels), Builder::powi in csrc/fdg_opt.cpp with the M_DIV1 / M_SEL / M_FMAK / M_CONST cases of csrc/fdg_isa.cpp (a hand-printed
correctly rounded reciprocal, a v_cmp_class_f64 select whose false arm may carry a negation), and, independently, oracle/fdg_oracle.c.  The
other device tests feed Power nodes uniform numbers, on which isfinite(x) and isfinite(err) hold in every lane: neither select's false arm,
nor the scaling that v_div_scale / v_div_fmas / v_div_fixup exist for, nor lanes of one wave on different arms were ever reached.

Inputs.  X holds the values the edges are made of -- zeros, infinities, NaN, subnormals, DBL_MIN and DBL_MAX and their neighbours, squares
that just do / do not overflow or underflow, and per pow_body exponent one value whose power is the subnormal 2^-1040 -- 93 in all.  Column j
of a batch is X rotated by 3 j, so the 64 lanes of a wave hold every class at once.  NS: -9 ... 9 without 0 and 1, and 12, -13, 16, -16, 31,
-32.  pow_edges(ns): 16 leaves, their negations (a negated operand), sums of neighbours (an interior operand), and per exponent five Power
roots (FORMS).  `wide` = pow_edges(NS) has R = 115 (AGPR accumulators); `narrow` has R = 16 (accumulators in value registers, next to the
division's four temporary pairs): the exponents -7, -4, -1, 5, each without one of the five forms: with all twenty roots the handle builds no fused accumulating kernel
(build_acc_program's register condition from R = 17 on).  `wide9` is `wide` with |N| <= 9, for finite sums.

The oracle itself is held to exact rational arithmetic first (fractions.Fraction, correctly rounded by int / int; 5e-324 as the unit below
DBL_MIN).  Bounds, from the roundings each form performs: 0.5 ulp for N = 2 and -1, 2 ulp for N = 3, 3 ulp for N = -2, 1 ulp for pow_body.
Measured (oracle.powi and the library's fdg_powi alike, which agree bit for bit), worst error in ulp per exponent over X:

  -9: 0.500, -8: 0.452, -7: 0.500, -6: 0.462, -5: 0.500, -4: 0.473, -3: 0.500, -2: 1.372, -1: 0.500, 2: 0.480, 3: 0.807, 4: 0.592, 5: 0.471,
  6: 0.479, 7: 0.473, 8: 0.463, 9: 0.499, 12: 0.465, -13: 0.500, 16: 0.375, -16: 0.459, 31: 0.496, -32: 0.447

and +-inf exactly where the correctly rounded value is.  pow_body's signs are Julia's, not the mathematical ones ((-0.0)^9 is +0.0: the last
fma adds err = +0.0), and the device must match them.

What `wide` and `narrow` specialise to (FDG_SPEC_ISA, FDG_IGNORE_TUNED=1, no shipped cache): fdg_isa_eval[_nt][_cl], _acc[_nt], _rl, _rm;
`narrow` also _rl_acc and _rm_acc; FDG_ISA_POOL=1 adds _pool to both, FDG_ISA_COOP=1 adds _coop to `wide` only (build_coop_once deals whole
roots to the waves from R > 4 * waves on, and a Power root has a single term to deal otherwise), so the cooperative variant runs `wide`.

The CPU part needs no device; the GPU part asserts from kernel_info()["last_kernel"] that the plain, _rl, _rm, _coop, _pool, _acc, _rl_acc
and _rm_acc kernels each ran on these batches."""
import glob
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi
from feynmandiagram_jl_amd.nodetable import OP_POWER, OP_PROD, OP_SUM, from_program
from test_next_rows import replay
from test_random_graphs import same
from test_tile_major import from_tiles, to_tiles

TOL = 1e-12                        # tests/test_gpu_parity.py: |d| <= TOL * max(1, sum |w root|) per root
INF, NAN = math.inf, math.nan
DBL_MIN, DBL_MAX, TINY = 2.2250738585072014e-308, 1.7976931348623157e308, 5e-324

NS = tuple(n for n in range(-9, 10) if n not in (0, 1)) + (12, -13, 16, -16, 31, -32)
LITERAL = (2, 3, -1, -2)                                  # Base.literal_pow; every other exponent is pow_body
BODY = tuple(n for n in NS if n not in LITERAL)
NARROW_NS = (-7, -4, -1, 5)

# |x|^N = 2^-1040 (to a few ulp): a subnormal result for every pow_body exponent, alternating in sign
TUNED = [(-1.0) ** i * 2.0 ** (-1040.0 / n) for i, n in enumerate(BODY)]


def _both(*v):
    return [s * x for x in v for s in (1.0, -1.0)]


# Order matters only to the nodes leaf_j + leaf_(j+1), whose operands are X[m] + X[m + 3] (column j is X rotated by 3 j): the head of the
# list makes those sums +0, -0, a subnormal whose reciprocal overflows and a number whose reciprocal is subnormal, in either sign; every
# tuned value stands three places from values below its last bit, so the sum returns it; the infinities meet finite numbers.  What this
# has to achieve is asserted in test_edge_batch_reaches_every_arm_of_every_root.
_HEAD = [0.0, -0.0, 5e-324, 0.0, -0.0, 1.5e-323, -5e-324, DBL_MAX / 2, -DBL_MAX / 2, -1.5e-323, DBL_MAX / 4, -DBL_MAX / 4]
_SMALL = _both(6.3e-322, 3.3e-310, 7.7e-315, DBL_MIN, math.nextafter(DBL_MIN, 0.0), DBL_MIN / 2, 1e-300, 1e-103) + [0.0, -0.0]
_REST = (_both(1.0, INF, DBL_MAX, 1e300, 2.0 ** 512, math.nextafter(2.0 ** 512, 0.0), 1.4916681462400413e-154, 1e155, 1e103, 1e77, 1e-77,
               2.0 ** -512, 2.0 ** 511, 2.0 ** 147, 3.0 ** -30)
         + [NAN, 1 + 2.0 ** -52, 1 - 2.0 ** -52, 1 - 2.0 ** -53, math.pi, -math.e, 0.1, -0.3, 3.0, -7.0, 1 / 3, 1e10, -1e-10, 1.5])


def _interleave(tuned, small):
    """s s s t t t s s s t t t s s s ...: every t three places from an s on either side"""
    out, small = list(small[:3]), list(small[3:])
    for i in range(0, len(tuned), 3):
        out += tuned[i:i + 3] + small[:3]
        small = small[3:]
    return out + small


X = np.array(_HEAD + _interleave(TUNED, _SMALL) + _REST)
BATCHES = (len(X), 64, 65, 337)
L = 16
FORMS = ("leaf", "negated", "sum * -1", "leaf * 0.125", "sum * 3")


def pow_edges(ns, skip=None, name="pow_edges"):
    """L = 16 leaves; nodes -leaf_j (a Prod with factor -1: its consumer's operand carries the negation), nodes leaf_j + leaf_(j+1) (an interior
    operand; j < 15, so that every one adds entries of X three places apart); per exponent one Power root in each of the five FORMS (but the
    one `skip` names for it), the operands spread over the leaves.  Returns (table, [(N, form, operand column(s))] per root)."""
    nodes = [(OP_PROD, 0, [(j, -1.0)]) for j in range(L)]
    nodes += [(OP_SUM, 0, [(j, 1.0), (j + 1, 1.0)]) for j in range(L - 1)]
    neg, add = L, 2 * L
    roots, what, k = [], [], 0
    for n in ns:
        for f in range(5):
            if skip and skip.get(n) == f:
                continue
            j, s = k % L, k % (L - 1)
            child = [(j, 1.0), (neg + j, 1.0), (add + s, -1.0), (j, 0.125), (add + s, 3.0)][f]
            roots.append(L + len(nodes))
            nodes.append((OP_POWER, int(n), [child]))
            what.append((int(n), f, s if f in (2, 4) else j))
            k += 1
    return from_program(L, nodes, roots, name), what


WIDE, WIDE_ROOTS = pow_edges(NS, name="pow_edges_wide")
# R <= 16, the accumulators in value registers: four exponents, each without one of the five forms (a different one each)
NARROW, NARROW_ROOTS = pow_edges(NARROW_NS, skip={-7: 4, -4: 3, -1: 2, 5: 1}, name="pow_edges_narrow")


def leaves(B, x=X):
    """column j is x rotated by 3 j; batches longer than x repeat it"""
    b, j = np.meshgrid(np.arange(B), np.arange(L), indexing="ij")
    return np.ascontiguousarray(x[(b + 3 * j) % len(x)])


def operands(what, leaf):
    """the operand of every root's Power node, [B, R]"""
    with np.errstate(all="ignore"):
        return np.stack([leaf[:, j] + leaf[:, j + 1] if f in (2, 4) else -leaf[:, j] if f == 1 else leaf[:, j] for _, f, j in what], axis=1)


# |N| <= 9 on finite operands of moderate size: every root finite, the batch of the accumulation tests
NS9 = tuple(n for n in NS if abs(n) <= 9)
WIDE9, WIDE9_ROOTS = pow_edges(NS9, name="pow_edges_wide9")
XF = X[np.isfinite(X) & (np.abs(X) >= 1e-30) & (np.abs(X) <= 1e30)]

TABLES = {"wide": WIDE, "narrow": NARROW, "wide9": WIDE9}
ROOTS = {"wide": WIDE_ROOTS, "narrow": NARROW_ROOTS, "wide9": WIDE9_ROOTS}
OPTS = {"FDG_CACHE_RO_DIR": "", "FDG_IGNORE_TUNED": "1"}
PLAIN = ("fdg_isa_eval", "fdg_isa_eval_nt", "fdg_isa_eval_cl", "fdg_isa_eval_nt_cl")
PLAIN_ACC = ("fdg_isa_eval_acc", "fdg_isa_eval_acc_nt")

_WANT = {}


def want(tid, B, x=X):
    """(leaves, the oracle's roots) of a batch: computed once, shared, read-only"""
    key = (tid, B, len(x))
    if key not in _WANT:
        leaf = leaves(B, x)
        with np.errstate(all="ignore"):
            r = oracle.eval_static(TABLES[tid], leaf)
        leaf.setflags(write=False)
        r.setflags(write=False)
        _WANT[key] = (leaf, r)
    return _WANT[key]


def subnormal(v):
    return (v != 0) & (np.abs(v) < DBL_MIN)


def differs(got, r, what):
    """[] where `same`; else the first places that differ: (row, (N, form, operand column), device, oracle)"""
    if same(got, r):
        return []
    n = np.isnan(r)
    ne = (np.isnan(got) != n) | (~n & ((got != r) | (np.signbit(got) != np.signbit(r))))
    return [(int(b), (what[k][0], FORMS[what[k][1]], what[k][2]), float(got[b, k]), float(r[b, k])) for b, k in np.argwhere(ne)[:5]]


# --------------------------------------------------------------------------- #
# CPU part
# --------------------------------------------------------------------------- #
def ulp_error(got, exact):
    """|got - exact| in units of the last place of the correctly rounded exact value (5e-324 below DBL_MIN); the rounded value"""
    try:
        rounded = float(exact)               # int / int: correctly rounded, subnormals included
    except OverflowError:
        return None, INF if exact > 0 else -INF
    if math.isinf(got):
        return INF, rounded
    return abs(Fraction(got) - exact) / Fraction(max(math.ulp(rounded), TINY)), rounded


def bound(n):
    """what each form's roundings allow: x * x and 1 / x are one rounding; x * x * x two; (1 / x)^2 three (the reciprocal's error doubles
    in the square: 2 * 0.5 + 0.5, and another half where the square falls into the binade below); pow_body is compensated to 1 ulp"""
    return {2: 0.5, -1: 0.5, 3: 2.0, -2: 3.0}.get(n, 1.0)


@pytest.mark.parametrize("impl", ["oracle", "capi"])
def test_scalar_power_against_exact_rational_arithmetic(libfdg, impl):
    powi = oracle.powi if impl == "oracle" else capi.powi
    worst, bad = {}, []
    for n in NS:
        w = Fraction(0)
        for x in X[np.isfinite(X) & (X != 0)].tolist():
            exact = Fraction(x) ** n
            got = powi(x, n)
            err, rounded = ulp_error(got, exact)
            if err is None or math.isinf(rounded):
                if got != rounded:
                    bad.append((x, n, got, "the correctly rounded value is", rounded))
                continue
            if math.isinf(got) or math.isnan(got):
                bad.append((x, n, got, "the correctly rounded value is finite:", rounded))
                continue
            if got != 0 and (got < 0) != (exact < 0):
                bad.append((x, n, got, "sign"))
            if err > bound(n):
                bad.append((x, n, got, float(err), "ulp >", bound(n)))
            w = max(w, err)
        worst[n] = float(w)
    print(f"{impl}.powi, worst error in ulp per exponent: " + ", ".join(f"{n}: {worst[n]:.3f}" for n in NS))
    assert not bad, bad[:10]


def test_library_scalar_equals_the_oracle_bit_for_bit(libfdg):
    for n in NS + (0, 1):
        for x in X.tolist():
            a, b = capi.powi(x, n), oracle.powi(x, n)
            assert (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b)), (x, n, a, b)


def test_edge_batch_reaches_every_arm_of_every_root():
    """The batch cannot hide a dead arm: per pow_body root a NaN, an infinite, a zero, a subnormal and a normal result; per negative exponent
    operands 0 and inf, an operand whose reciprocal overflows and one whose reciprocal is subnormal; rows with NaN, inf and finite roots."""
    leaf, r = want("wide", len(X))
    x = operands(WIDE_ROOTS, leaf)
    with np.errstate(all="ignore"):
        rx = 1.0 / x
    for k, (n, f, j) in enumerate(WIDE_ROOTS):
        c = r[:, k]
        if n in BODY:
            have = {"nan": np.isnan(c).any(), "inf": np.isinf(c).any(), "zero": (c == 0).any(), "subnormal": subnormal(c).any(),
                    "normal": (np.isfinite(c) & (np.abs(c) >= DBL_MIN)).any()}
            assert all(have.values()), (n, FORMS[f], j, have)
        if n < 0:
            for s in (1.0, -1.0):            # each in either sign
                have = {"x = 0": ((x[:, k] == 0) & (np.copysign(1.0, x[:, k]) == s)).any(), "x = inf": (x[:, k] == s * INF).any(),
                        "1 / x = inf": ((x[:, k] != 0) & (rx[:, k] == s * INF)).any(), "1 / x subnormal": (subnormal(rx[:, k]) & (rx[:, k] * s > 0)).any()}
                assert all(have.values()), (n, FORMS[f], j, s, have)
    mixed = np.isnan(r).any(1) & np.isinf(r).any(1) & np.isfinite(r).any(1)
    assert mixed.any()
    assert WIDE.n_root == 5 * len(NS) and NARROW.n_root <= 16


BUDGETS = [dict(), dict(n_reg=120, n_lds=80, n_acc=124), dict(n_reg=24, n_lds=3, n_acc=2), dict(n_reg=16, n_lds=0, n_acc=0)]


@pytest.mark.parametrize("budget", BUDGETS, ids=["default", "120-80-124", "24-3-2", "16-0-0"])
@pytest.mark.parametrize("tid", ["wide", "narrow"])
def test_allocated_program_replays_to_the_oracle_on_the_edge_batch(libfdg, tid, budget):
    t = TABLES[tid]
    h = capi.GraphHandle(t)
    ops, nr, nl, nm = h.opt_program(**budget)
    kind = ops["kind"]
    sel = ops[kind == 19]
    assert (kind == 23).any() and (kind == 22).any() and (kind == 24).any(), "no M_DIV1 / M_FMAK / M_CONST"
    assert len(sel) and (sel["imm"] == 2.0).all() and sel["negb"].any(), "no isfinite select, or none whose false arm carries a negation"
    leaf, r = want(tid, len(X))
    with np.errstate(all="ignore"):
        got = replay(ops, nr, nl, nm, h.last_n_acc, leaf, t.n_root)
    assert not differs(got, r, ROOTS[tid]), differs(got, r, ROOTS[tid])


VARIANTS = {"plain": {}, "coop": {"FDG_ISA_COOP": "1"}, "pool": {"FDG_ISA_POOL": "1"}}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("tid", ["wide", "narrow"])
def test_every_variant_assembles_with_the_division_and_the_class_compare(libfdg, tmp_path, tid, variant):
    os.chmod(tmp_path, 0o700)
    f = fd.compile_table(TABLES[tid], specialize="isa", cache_dir=str(tmp_path), flags=capi.FDG_SPEC_KEEP_SOURCE, options={**OPTS, **VARIANTS[variant]})
    texts = [open(p).read() for p in sorted(glob.glob(os.path.join(str(tmp_path), "*.s")))]
    assert texts, "FDG_SPEC_KEEP_SOURCE left no listing"
    for text in texts:
        n, rep = capi.isa_check_hazards(text)
        assert n == 0, rep
    text = "".join(texts)
    assert "v_div_fixup_f64" in text and "v_cmp_class_f64" in text
    ki = f.kernel_info()
    assert (ki["has_rm"], ki["has_rl"], ki["has_acc"]) == (1, 1, 1), ki
    assert ("fdg_isa_eval_rl_acc:" in text) == ("fdg_isa_eval_rm_acc:" in text) == (tid == "narrow")
    # build_coop_once deals whole roots to the waves from R > 4 * waves on, and these roots have one term each: no cooperative form of `narrow`
    assert ki["has_coop"] == int(variant == "coop" and tid == "wide") and ("fdg_isa_eval_coop:" in text) == bool(ki["has_coop"]), ki
    assert ki["has_pool"] == int(variant == "pool") and ("fdg_isa_eval_pool:" in text) == bool(ki["has_pool"]), ki


# --------------------------------------------------------------------------- #
# GPU part
# --------------------------------------------------------------------------- #
def compiled(tid, spec, tmp_path, **options):
    """every specialisation into a cache directory of its own, without the shipped code objects and without a remembered tuner's choice"""
    os.chmod(tmp_path, 0o700)
    return fd.compile_table(TABLES[tid], specialize=spec, cache_dir=str(tmp_path) if spec else None, options={**OPTS, **options})


def device_layouts(cuda, h_leaf):
    import torch
    B = h_leaf.shape[0]
    rows = torch.tensor(h_leaf, device=cuda)
    pad = torch.full((B, L + 3), 7.0, dtype=torch.float64, device=cuda)
    pad[:, :L] = rows
    return {"rows": rows, "padded rows": pad[:, :L], "leaf-major": rows.t().contiguous().t()}


@pytest.mark.gpu
@pytest.mark.parametrize("spec", [False, True, "isa"], ids=["interp", "hipjit", "isa"])
def test_three_back_ends_on_the_edge_batch(libfdg, cuda, tmp_path, spec):
    import torch
    f = compiled("wide", spec, tmp_path)
    R = WIDE.n_root
    last = lambda: f.kernel_info()["last_kernel"]
    seen = set()
    for B in BATCHES:
        h_leaf, r = want("wide", B)
        lay = device_layouts(cuda, h_leaf)
        for name in ("rows", "leaf-major") + (("padded rows",) if spec == "isa" else ()):
            root = torch.full((B, R), 9.0, dtype=torch.float64, device=cuda)
            f(root, lay[name])
            torch.cuda.synchronize()
            seen.add((last(), B >= 64))
            assert not differs(root.cpu().numpy(), r, WIDE_ROOTS), (spec, name, B, last(), differs(root.cpu().numpy(), r, WIDE_ROOTS))
        root = torch.full((R, B), 9.0, dtype=torch.float64, device=cuda).t()          # a Julia B x R matrix next to a Julia B x L matrix
        f(root, lay["leaf-major"])
        torch.cuda.synchronize()
        assert not differs(root.cpu().numpy(), r, WIDE_ROOTS), (spec, "column-major leaves and roots", B, last(), differs(root.cpu().numpy(), r, WIDE_ROOTS))
        if spec == "isa":
            assert last() in PLAIN, last()
            rt = torch.full(((B + 63) // 64, R, 64), 9.0, dtype=torch.float64, device=cuda)
            f.eval_tiled(rt, torch.tensor(to_tiles(h_leaf), device=cuda), B)
            torch.cuda.synchronize()
            h_rt = rt.cpu().numpy()
            assert not differs(from_tiles(h_rt, B, R), r, WIDE_ROOTS), (spec, "tile-major", B, last(), differs(from_tiles(h_rt, B, R), r, WIDE_ROOTS))
            assert (h_rt.transpose(0, 2, 1).reshape(-1, R)[B:] == 9.0).all(), ("tile-major", B, "lanes behind the batch written")
            assert last() in PLAIN, last()
    if spec == "isa":
        names = {k for k, _ in seen}
        assert {"fdg_isa_eval_rl", "fdg_isa_eval_rm"} <= names and names & set(PLAIN), sorted(seen)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,tid,options,off", [("coop", "wide", {"FDG_ISA_COOP": "1", "FDG_COOP_WAVES": "4"}, "FDG_ISA_NO_COOP"),
                                                     ("coop", "wide", {"FDG_ISA_COOP": "1", "FDG_COOP_WAVES": "8"}, "FDG_ISA_NO_COOP"),
                                                     ("pool", "narrow", {"FDG_ISA_POOL": "1"}, "FDG_ISA_NO_POOL")],
                         ids=["coop-4-waves", "coop-8-waves", "pool"])
def test_cooperative_and_pooled_variants_on_the_edge_batch(libfdg, cuda, tmp_path, variant, tid, options, off):
    """The variants' own temporaries next to the division's: leaf-major batches through the variant, then the same handle with the variant
    switched off -- the oracle's roots, and the same bytes both ways.  (`narrow` has no cooperative form -- whole roots are dealt to the waves
    from R > 4 * waves on -- so that variant runs `wide`.)"""
    import torch
    f = compiled(tid, "isa", tmp_path, **options)
    assert f.kernel_info()["has_" + variant] == 1, f.kernel_info()
    R, what = TABLES[tid].n_root, ROOTS[tid]
    for B in BATCHES:
        h_leaf, r = want(tid, B)
        leaf = device_layouts(cuda, h_leaf)["leaf-major"]
        got = []
        for switch in (None, "1"):
            f.handle.set_option(off, switch)
            root = torch.full((B, R), 9.0, dtype=torch.float64, device=cuda)
            f(root, leaf)
            torch.cuda.synchronize()
            k = f.kernel_info()["last_kernel"]
            assert (k == "fdg_isa_eval_" + variant) == (switch is None), (variant, B, switch, k)
            assert not differs(root.cpu().numpy(), r, what), (variant, B, switch, k, differs(root.cpu().numpy(), r, what))
            got.append(root)
        assert torch.equal(got[0].view(torch.int64), got[1].view(torch.int64)), (variant, B, "the variant and the one-wave kernel differ in bytes")


def fsum_columns(terms):
    return np.array([math.fsum(terms[:, k].tolist()) for k in range(terms.shape[1])])


def accumulate_forms(f, cuda, h_leaf, d_w, R):
    """form -> (device sum, the kernel that made it); every form twice, the two calls equal in bytes"""
    import torch
    B = h_leaf.shape[0]
    out = {}
    lay = device_layouts(cuda, h_leaf)
    lay["tile-major"] = torch.tensor(to_tiles(h_leaf), device=cuda)
    for name, leaf in lay.items():
        two = []
        for _ in range(2):
            acc = torch.zeros(R, dtype=torch.float64, device=cuda)
            if name == "tile-major":
                f.accumulate_tiled(leaf, d_w, acc, B)
            else:
                f.accumulate(leaf, d_w, acc)
            torch.cuda.synchronize()
            two.append(acc)
        k = f.kernel_info()["last_kernel"]
        assert torch.equal(two[0].view(torch.int64), two[1].view(torch.int64)), (name, B, k, "two calls differ")
        out[name] = (two[0].cpu().numpy(), k)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tid", ["narrow", "wide9"])
def test_fused_accumulation_beside_the_macro_temporaries(libfdg, cuda, tmp_path, tid):
    """`narrow`: R + 2 value-register pairs reserved next to the division's four; `wide9`: the accumulators in AGPR pairs.  Finite operands
    (1e-30 <= |x| <= 1e30, |N| <= 9), so every root is finite and the sum is compared with math.fsum of the oracle's terms."""
    import torch
    f = compiled(tid, "isa", tmp_path)
    R = TABLES[tid].n_root
    assert f.kernel_info()["has_acc"] == 1
    seen = set()
    for B in (63, 64, 337):
        h_leaf, r = want(tid, B, XF)
        assert np.isfinite(r).all(), (tid, B, "the finite batch has a non-finite root")
        h_w = np.random.default_rng(B).uniform(0.5, 1.5, B)
        terms = r * h_w[:, None]
        ref, scale = fsum_columns(terms), np.maximum(1.0, fsum_columns(np.abs(terms)))
        for name, (got, k) in accumulate_forms(f, cuda, h_leaf, torch.from_numpy(h_w).to(cuda), R).items():
            d = np.abs(got - ref)
            print(tid, B, name, k, "max |d| / scale", float((d / scale).max()))
            assert np.all(d <= TOL * scale), (tid, B, name, k, int(np.argmax(d / scale)), float((d / scale).max()))
            assert "_acc" in k, (tid, B, name, k)
            seen.add(k)
    if tid == "narrow":
        assert {"fdg_isa_eval_rl_acc", "fdg_isa_eval_rm_acc"} <= seen and seen & set(PLAIN_ACC), sorted(seen)
    else:
        assert seen <= set(PLAIN_ACC), sorted(seen)


def classify(terms):
    """per root what a sum of these terms is in any order: 'nan' (a NaN term, or infinities of both signs), '+inf' / '-inf' (infinite terms of
    one sign), 'finite'; and math.fsum of |finite terms|, infinite where that overflows"""
    R = terms.shape[1]
    cls, mass = [], np.zeros(R)
    for k in range(R):
        c = terms[:, k]
        pos, neg = bool((c == INF).any()), bool((c == -INF).any())
        cls.append("nan" if np.isnan(c).any() or (pos and neg) else "+inf" if pos else "-inf" if neg else "finite")
        try:
            mass[k] = math.fsum(np.abs(c[np.isfinite(c)]).tolist())
        except OverflowError:
            mass[k] = INF
    return np.array(cls), mass


EDGE_ROWS = (3, 26, 49, 72)


def seeded_batch(tid, B):
    """the finite batch with four rows of the edge batch in it (rows 3, B // 3, 2 B // 3 and B - 2: other tiles and lanes at every B)"""
    leaf = leaves(B, XF)
    leaf[[3, B // 3, 2 * B // 3, B - 2]] = want("wide", len(X))[0][list(EDGE_ROWS)]
    with np.errstate(all="ignore"):
        return leaf, oracle.eval_static(TABLES[tid], leaf)


@pytest.mark.gpu
@pytest.mark.parametrize("tid,least", [("wide", 15), ("narrow", 3)])
def test_non_finite_rows_reach_only_their_own_roots(libfdg, cuda, tmp_path, tid, least):
    """Fused accumulation with AGPR accumulators (`wide`) and with value-register accumulators (`narrow`, also through the row-major kernels).
    Over the whole edge batch every root meets the NaN of X, which would show nothing, so four of its rows stand in the finite batch: of the
    115 roots of `wide` 26 then have a NaN term or infinite terms of both signs (13 the latter alone), 39 and 27 infinite terms of one sign,
    23 finite terms only; of the 16 of `narrow` 3, 6, 4 and 3 (`least` of each asserted).  A root's sum is NaN or infinite exactly where its
    terms say so, and a root whose terms are all finite keeps the bound of the finite batch, whatever the accumulators next to it hold.  A
    root whose finite terms add up to DBL_MAX / 4 or more in magnitude is left out (one per table, at B = 337): there one order of summation
    may overflow where another does not."""
    import torch
    f = compiled(tid, "isa", tmp_path)
    R = TABLES[tid].n_root
    what = ROOTS[tid]
    seen = set()
    for B in (64, len(X), 337):
        h_leaf, r = seeded_batch(tid, B)
        h_w = np.random.default_rng(B).uniform(0.5, 1.5, B)
        with np.errstate(all="ignore"):
            terms = r * h_w[:, None]
        cls, mass = classify(terms)
        settled = mass < DBL_MAX / 4
        count = {c: int((settled & (cls == c)).sum()) for c in ("nan", "+inf", "-inf", "finite")}
        assert min(count.values()) >= least and settled.sum() >= R - 1, count
        assert (~np.isnan(terms).any(0) & (cls == "nan")).any(), "no root is NaN by infinite terms of both signs alone"
        fin = settled & (cls == "finite")
        ref = fsum_columns(np.where(fin[None, :], terms, 0.0))
        for name, (got, k) in accumulate_forms(f, cuda, h_leaf, torch.from_numpy(h_w).to(cuda), R).items():
            assert "_acc" in k, (tid, B, name, k)
            seen.add(k)
            is_cls = np.where(np.isnan(got), "nan", np.where(got == INF, "+inf", np.where(got == -INF, "-inf", "finite")))
            wrong = settled & (is_cls != cls)
            assert not wrong.any(), (tid, B, name, k, [(what[i], cls[i], got[i]) for i in np.flatnonzero(wrong)[:5]])
            d = np.abs(got[fin] - ref[fin])
            assert np.all(d <= TOL * np.maximum(1.0, mass[fin])), (tid, B, name, k, float((d / np.maximum(1.0, mass[fin])).max()))
    assert ({"fdg_isa_eval_rl_acc", "fdg_isa_eval_rm_acc"} <= seen) == (tid == "narrow") and seen & set(PLAIN_ACC), sorted(seen)
