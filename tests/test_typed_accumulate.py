"""Fused weighted accumulation for the element types other than Float64 (include/fdg.h: fdg_accumulate_device_typed; the integrand's
``sum weight * root over samples`` around the generic ``eval_graph!``).

CPU part: the symbol is declared, exported and bound, every refusal runs before any device work, the per-type source carries the
second kernel ``fdg_spec_typed_acc`` and still cross-compiles for gfx950, and the text of the evaluating kernel ``fdg_spec_typed`` is
what it was before the second kernel joined it (tests/golden/typed_eval_kernel_text.json: SHA-256 of that text, recorded from the
commit before).  GPU part: the sums against the typed twin's roots (oracle.eval_static_typed) widened to Float64 / ComplexF64,
multiplied by the weights and summed in Float64 on the host, within the project's accumulate tolerance (tests/test_gpu_parity.py::
test_accumulate: 1e-12 of max(1, sum |w x|) per component; only the order of a Float64 sum differs from the host's)."""
import hashlib
import json
import os
import re

import numpy as np
import pytest

import oracle
import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, workloads
from feynmandiagram_jl_amd.nodetable import FDG_NO_ROOT, OP_PROD, OP_SUM, from_program

from test_typed import NP, cancelling_product_case, dev_typed, rand_leaves, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fdg.h")
GOLD_TEXT = os.path.join(os.path.dirname(__file__), "golden", "typed_eval_kernel_text.json")
NAME = "fdg_accumulate_device_typed"
TOL = 1e-12
DTYPES = ["Float32", "ComplexF64", "ComplexF32"]
FAKE, FAKE2, FAKE3 = 0x10000, 0x20000, 0x30000      # pointers the checks only compare with NULL or with each other: nothing is read through them


# ---------------------------------------------------------------------------------------------------------- CPU


def test_symbol_is_declared_exported_and_bound(libfdg):
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", open(HDR).read())
    assert NAME in capi.EXPORTS and hasattr(libfdg, NAME)
    assert hasattr(capi.GraphHandle, "accumulate_device_typed")
    text = open(HDR).read()
    assert "No fused accumulation" not in text


def _call(h, dtype, B, d_leaf=FAKE, d_acc=FAKE2, d_acc2=FAKE3):
    return capi.lib().fdg_accumulate_device_typed(h._h if h else None, dtype, d_leaf, 8, 1, None, d_acc, d_acc2, B, None)


def test_refusals_need_no_device(libfdg, tmp_path):
    h = capi.GraphHandle(workloads.get("sigma2"))
    h.specialize_typed(capi.FDG_DT_F32, str(tmp_path))
    F32, C32, F64 = capi.FDG_DT_F32, capi.FDG_DT_C32, capi.FDG_DT_F64
    assert _call(None, F32, 100) == capi.FDG_E_INVALID                      # null handle
    for bad in (-1, 4, 7):
        assert _call(h, bad, 100) == capi.FDG_E_INVALID                     # unknown dtype
    for dt in (F32, F64):
        assert _call(h, dt, -1) == capi.FDG_E_INVALID                       # n_sample < 0
        assert _call(h, dt, 100, d_acc=None) == capi.FDG_E_INVALID
        assert _call(h, dt, 100, d_acc2=FAKE2) == capi.FDG_E_INVALID        # d_acc == d_acc2
        assert _call(h, dt, 100, d_leaf=None) == capi.FDG_E_INVALID
        assert _call(h, dt, 100, d_leaf=None, d_acc2=None) == capi.FDG_E_INVALID
    assert _call(h, C32, 100) == capi.FDG_E_INVALID                         # a type not yet specialised
    assert "fdg_graph_specialize_typed" in capi.lib().fdg_last_error().decode()
    assert _call(h, capi.FDG_DT_C64, 0) == capi.FDG_E_INVALID               # ... whatever the batch
    # nothing to do: no device work, no error
    assert _call(h, F32, 0) == capi.FDG_OK
    assert _call(h, F32, 0, d_acc2=None) == capi.FDG_OK
    assert _call(h, F64, 0, d_acc2=None) == capi.FDG_OK
    e = capi.GraphHandle(from_program(2, [], [], name="no_roots"))
    e.specialize_typed(F32, str(tmp_path))
    assert _call(e, F32, 100) == capi.FDG_OK
    # the Python method forwards the library's answer
    with pytest.raises(capi.FdgError) as err:
        h.accumulate_device_typed(C32, FAKE, 8, 1, 0, FAKE2, 0, 100)
    assert err.value.code == capi.FDG_E_INVALID


def _eval_kernel_text(src):
    i = src.index('extern "C" __global__ void __launch_bounds__(256) fdg_spec_typed(')
    return src[i:src.index("\n}\n", i) + 3]


@pytest.mark.parametrize("name", ["sigma2", "parquet_sigma3", "gv_sigma4"])
def test_source_carries_both_kernels_and_the_evaluating_one_is_unchanged(libfdg, no_shipped_cache, tmp_path, name):
    gold = json.load(open(GOLD_TEXT))
    g = capi.GraphHandle(workloads.get(name))
    for dtype in DTYPES:
        d = tmp_path / dtype
        d.mkdir()
        g.specialize_typed(capi.DTYPES[dtype], str(d), capi.FDG_SPEC_KEEP_SOURCE)          # hiprtc cross-compiles without a device
        files = sorted(os.listdir(d))
        assert [f[-4:] for f in files] == [".hip", "saco"], files                         # the source and its gfx950 code object
        assert os.path.getsize(d / files[1]) > 0
        src = open(d / files[0]).read()
        assert "fdg_spec_typed_acc(" in src and "__shfl_xor" in src and "atomic" not in src
        # the markers of tests/test_typed.py, then the whole text of the evaluating kernel
        T = {"Float32": "float", "ComplexF64": "fdg_cx<double>", "ComplexF32": "fdg_cx<float>"}[dtype]
        ev = _eval_kernel_text(src)
        assert f"fdg_spec_typed(const {T} *__restrict__ leaf" in ev and "const auto v" in ev and "fdg_spec_typed_acc" not in ev
        assert {"sha256": hashlib.sha256(ev.encode()).hexdigest(), "bytes": len(ev)} == gold[f"{name}:{dtype}"]
        # the accumulating kernel runs the same scheduled body: every statement of the evaluating kernel's body, in order
        body = ev[ev.index("*lp = leaf + b * ss;\n"):ev.rindex(f"    {T} *rp = root")]
        assert body in src[src.index("fdg_spec_typed_acc("):]


def test_julia_shim_binds_the_entry_point():
    text = open(os.path.join(ROOT, "feynmandiagram.jl_amd", "julia", "hip_compiler.jl")).read()
    assert text.count(":" + NAME + ",") == 1


# ---------------------------------------------------------------------------------------------------------- GPU

_FUNCS, _ROOTS = {}, {}
B_MAX = 4099


def func(name):
    """One handle per graph for the whole file (the typed kernels are added to it on first use)."""
    if name not in _FUNCS:
        _FUNCS[name] = fd.compile_table(workloads.get(name), specialize="isa")
    return _FUNCS[name]


def leaves_and_roots(name, dtype):
    """Leaves and the twin's roots of B_MAX samples, computed once and shared (never written to)."""
    if (name, dtype) not in _ROOTS:
        t = workloads.get(name)
        x = rand_leaves(B_MAX, t.n_leaf, dtype, 5)
        r = oracle.eval_static_typed(t, x, dtype)
        x.setflags(write=False); r.setflags(write=False)
        _ROOTS[name, dtype] = (x, r)
    return _ROOTS[name, dtype]


def parts(a):
    """The components the sums run over, in Float64: the value itself, or (re, im)."""
    a = np.asarray(a)
    return [a.real.astype(np.float64), a.imag.astype(np.float64)] if np.iscomplexobj(a) else [a.astype(np.float64)]


def close(got, roots, w, mult=1.0, base=None, what=""):
    """|got - sum_b w_b x_b| <= mult * TOL * max(1, sum_b |w_b x_b|), per component; returns the figures."""
    w = np.ones(roots.shape[0]) if w is None else w
    for c, (g, x) in enumerate(zip(parts(got), parts(roots))):
        t = x * w[:, None]
        want, scale = mult * t.sum(0), np.abs(t).sum(0)
        if base is not None:
            want = want + parts(base)[c]
        err = np.abs(g - want)
        print(what, "component", c, "max |d| / (TOL max(1, scale)) =", float(np.max(err / (TOL * np.maximum(1.0, scale)))))
        assert np.all(err <= mult * TOL * np.maximum(1.0, scale)), (what, c, err, scale)


def close2(got2, roots, w, mult=1.0, what=""):
    w = np.ones(roots.shape[0]) if w is None else w
    for c, (g, x) in enumerate(zip(parts(got2), parts(roots))):
        t2 = (x * w[:, None]) ** 2
        err = np.abs(g - mult * t2.sum(0))
        print(what, "squares, component", c, "max |d| / (TOL max(1, scale)) =", float(np.max(err / (TOL * np.maximum(1.0, t2.sum(0))))))
        assert np.all(err <= mult * TOL * np.maximum(1.0, t2.sum(0))), (what, c, err)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def weights(B, cuda, seed=8):
    import torch
    w = np.random.default_rng(seed).random(B) - 0.25
    return w, torch.from_numpy(w).to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["sample_major", "leaf_major", "padded"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["sigma2", "parquet_sigma3", "gv_sigma4"])
def test_sums_match_the_typed_twin(libfdg, cuda, name, dtype, layout):
    """B = 1, 63, 65, 257, 4099: one lane, a wave short by one lane, a second wave with one lane, a second block with one lane, many
    blocks with a ragged end."""
    import torch
    f = func(name)
    x, r = leaves_and_roots(name, dtype)
    for B in (1, 63, 65, 257, 4099):
        leaf = dev_typed(cuda, x[:B], layout)
        wn, wd = weights(B, cuda)
        for w_host, w_dev in ((wn, wd), (None, None)):
            acc = f.accumulate(leaf, w_dev)
            if f.last_typed_kernel != f"fdg_spec_typed_acc<{dtype}>":          # only ComplexF64 rows of 64 samples or more may take the other route
                assert dtype == "ComplexF64" and layout != "leaf_major" and B >= 64 and f.last_typed_kernel.endswith(" (ComplexF64 rows)")
            assert acc.dtype == (torch.complex128 if dtype.startswith("Complex") else torch.float64) and tuple(acc.shape) == (r.shape[1],)
            close(host(acc), r[:B], w_host, what=f"{name} {dtype} {layout} B={B}")
            acc1, acc2 = torch.zeros_like(acc), torch.zeros_like(acc)
            assert f.accumulate(leaf, w_dev, acc1, acc2) is acc1
            close(host(acc1), r[:B], w_host, what=f"{name} {dtype} {layout} B={B} (with acc2)")
            close2(host(acc2), r[:B], w_host, what=f"{name} {dtype} {layout} B={B}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["sample_major", "leaf_major"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_equal_bits_for_equal_arguments_and_adding_on_top(libfdg, cuda, dtype, layout):
    import torch
    name = "parquet_sigma3"
    f = func(name)
    x, r = leaves_and_roots(name, dtype)
    leaf = dev_typed(cuda, x, layout)
    wn, wd = weights(B_MAX, cuda)
    a1, q1 = f.accumulate(leaf, wd), None
    a2 = f.accumulate(leaf, wd)
    assert same_bits(host(a1), host(a2))
    b1, q1 = torch.zeros_like(a1), torch.zeros_like(a1)
    b2, q2 = torch.zeros_like(a1), torch.zeros_like(a1)
    f.accumulate(leaf, wd, b1, q1)
    f.accumulate(leaf, wd, b2, q2)
    assert same_bits(host(b1), host(b2)) and same_bits(host(q1), host(q2))
    # onto a filled accumulator: twice the sum
    top, top2 = a1.clone(), q1.clone()
    again, again2 = a1.clone(), q1.clone()
    f.accumulate(leaf, wd, top)
    f.accumulate(leaf, wd, again)
    assert same_bits(host(top), host(again))
    close(host(top), r, wn, mult=2.0, what=f"{dtype} {layout} twice")
    f.accumulate(leaf, wd, b1, top2)
    f.accumulate(leaf, wd, b2, again2)
    assert same_bits(host(top2), host(again2))
    close2(host(top2), r, wn, mult=2.0, what=f"{dtype} {layout} twice")


@pytest.mark.gpu
def test_a_second_round_of_the_grid_stride_loop(libfdg, cuda):
    """The launch's grid is min(cld(B, 256), 8 blocks per CU) blocks of 256 lanes (fdg_accumulate_device_typed); one batch just above
    256 x that grid makes 257 lanes run the loop's body twice (256 CUs: 524 288 + 257 samples of 8 leaves)."""
    import torch
    grid = 8 * torch.cuda.get_device_properties(cuda).multi_processor_count
    B = 256 * grid + 257
    t = workloads.get("sigma2")
    f = func("sigma2")
    x = rand_leaves(B, t.n_leaf, "ComplexF32", 17)
    r = oracle.eval_static_typed(t, x, "ComplexF32")
    wn, wd = weights(B, cuda)
    leaf = dev_typed(cuda, x, "leaf_major")
    acc, acc2 = torch.zeros(t.n_root, dtype=torch.complex128, device=cuda), torch.zeros(t.n_root, dtype=torch.complex128, device=cuda)
    f.accumulate(leaf, wd, acc, acc2)
    assert f.last_typed_kernel == "fdg_spec_typed_acc<ComplexF32>"
    close(host(acc), r, wn, what=f"second round B={B}")
    close2(host(acc2), r, wn, what=f"second round B={B}")
    close(host(f.accumulate(dev_typed(cuda, x, "sample_major"), None)), r, None, what=f"second round B={B}, rows, unit weights")


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["last", "first"])
def test_lanes_past_the_end_do_not_poison_an_infinite_sum(libfdg, cuda, where):
    """Root 0 = g0 * g0 overflows to +inf in Float32 on one sample of B = 65: the sum is +inf.  A lane past the end that were clamped
    to that sample with weight 0 (as the Float64 generic kernel clamps) would add 0 * inf = NaN."""
    import torch
    t = from_program(2, [(OP_PROD, 0, [(0, 1.0), (0, 1.0)])], [2, 1], name="overflow").normalized()
    B = 65
    x = rand_leaves(B, 2, "Float32", 23)
    x[-1 if where == "last" else 0, 0] = np.float32(1e30)
    with np.errstate(over="ignore"):
        r = oracle.eval_static_typed(t, x, "Float32")
    assert np.isposinf(r[:, 0]).sum() == 1 and np.isfinite(r[:, 1]).all()
    f = fd.compile_table(t, specialize="isa")
    wn = np.random.default_rng(4).random(B) + 0.5                    # positive weights: the infinite term is +inf
    for w_host in (wn, None):
        for layout in ("sample_major", "leaf_major"):
            acc, acc2 = torch.zeros(2, dtype=torch.float64, device=cuda), torch.zeros(2, dtype=torch.float64, device=cuda)
            f.accumulate(dev_typed(cuda, x, layout), None if w_host is None else torch.from_numpy(w_host).to(cuda), acc, acc2)
            assert f.last_typed_kernel == "fdg_spec_typed_acc<Float32>"
            a, a2 = host(acc), host(acc2)
            assert np.isposinf(a[0]) and np.isposinf(a2[0]), (a, a2)
            close(a[1:], r[:, 1:], w_host, what=f"infinite sample {where}")
            close2(a2[1:], r[:, 1:], w_host, what=f"infinite sample {where}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_missing_root_keeps_the_bits_of_its_column(libfdg, cuda, dtype):
    import torch
    # value 3 = g0 * g1, value 4 = g2 * 2.5 + value 3; roots: value 3, an id no graph contains, value 4
    t = from_program(3, [(OP_PROD, 0, [(0, 1.0), (1, 1.0)]), (OP_SUM, 0, [(2, 2.5), (3, 1.0)])], [3, FDG_NO_ROOT, 4], name="missing").normalized()
    assert int(t.root_slot[1]) == FDG_NO_ROOT
    B = 257
    x = rand_leaves(B, 3, dtype, 31)
    r = oracle.eval_static_typed(t, x, dtype)
    f = fd.compile_table(t, specialize="isa")
    leaf = dev_typed(cuda, x, "leaf_major")
    wn, wd = weights(B, cuda)
    adt = torch.complex128 if dtype.startswith("Complex") else torch.float64
    for fill in (complex(-7.0, 3.5) if dtype.startswith("Complex") else -7.0, -0.0):
        acc, acc2 = torch.full((3,), fill, dtype=adt, device=cuda), torch.full((3,), fill, dtype=adt, device=cuda)
        if fill == 0:
            acc, acc2 = -torch.zeros(3, dtype=adt, device=cuda), -torch.zeros(3, dtype=adt, device=cuda)      # -0.0 in every component
        before = host(acc).copy()
        assert all(np.signbit(p).all() for p in parts(before)) or fill != 0
        f.accumulate(leaf, wd, acc, acc2)
        assert f.last_typed_kernel == f"fdg_spec_typed_acc<{dtype}>"
        a, a2 = host(acc), host(acc2)
        assert same_bits(a[1:2], before[1:2]) and same_bits(a2[1:2], before[1:2])
        live = [0, 2]
        close(a[live], r[:, live], wn, base=before[live], what=f"missing root {dtype} fill={fill}")
        for c, (g, x2, b0) in enumerate(zip(parts(a2[live]), parts(r[:, live]), parts(before[live]))):
            t2 = (x2 * wn[:, None]) ** 2
            assert np.all(np.abs(g - (b0 + t2.sum(0))) <= TOL * np.maximum(1.0, t2.sum(0)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gv_sigma4", "parquet_sigma4"])
def test_complex_rows_go_through_the_spelled_out_graph(libfdg, cuda, name):
    import torch
    t = workloads.get(name)
    f = func(name)
    x = rand_leaves(B_MAX, t.n_leaf, "ComplexF64", 5)
    r = oracle.eval_static_typed(t, x, "ComplexF64")
    wn, wd = weights(B_MAX, cuda)
    rows = f.accumulate(dev_typed(cuda, x, "sample_major"), wd)
    assert "_acc" in f.last_typed_kernel and "ComplexF64 rows" in f.last_typed_kernel, f.last_typed_kernel
    cols = f.accumulate(dev_typed(cuda, x, "leaf_major"), wd)
    assert f.last_typed_kernel == "fdg_spec_typed_acc<ComplexF64>"
    close(host(rows), r, wn, what=f"{name} rows")
    close(host(cols), r, wn, what=f"{name} columns")
    for g, c, x_ in zip(parts(host(rows)), parts(host(cols)), parts(r)):
        assert np.all(np.abs(g - c) <= TOL * np.maximum(1.0, np.abs(x_ * wn[:, None]).sum(0)))
    # with the squares: the spelled-out graph's moments call
    a, a2 = torch.zeros_like(rows), torch.zeros_like(rows)
    f.accumulate(dev_typed(cuda, x, "sample_major"), wd, a, a2)
    assert "ComplexF64 rows" in f.last_typed_kernel
    close(host(a), r, wn, what=f"{name} rows (with acc2)")
    close2(host(a2), r, wn, what=f"{name} rows")
    # fewer than 64 samples: the per-type kernel
    small = f.accumulate(dev_typed(cuda, x[:63], "sample_major"), wd[:63])
    assert f.last_typed_kernel == "fdg_spec_typed_acc<ComplexF64>"
    close(host(small), r[:63], wn[:63], what=f"{name} rows B=63")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["ComplexF64", "ComplexF32"])
def test_signs_of_the_cancelling_product_case(libfdg, cuda, dtype):
    import torch
    t, z = cancelling_product_case()
    z = z.astype(NP[dtype])
    r = oracle.eval_static_typed(t, z, dtype)
    f = fd.compile_table(t, specialize="isa")
    for leaf in (torch.from_numpy(z).to(cuda), dev_typed(cuda, z, "leaf_major")):
        close(host(f.accumulate(leaf, None)), r, None, what=f"cancelling product {dtype}")


@pytest.mark.gpu
def test_float32_sum_is_over_the_widened_reading(libfdg, cuda):
    """tests/test_typed.py::test_float32_values_are_widened_by_a_factor_literal through accumulate: the sum is over Julia's reading
    (the Float64 literal widens its term; the root is rounded once, at the store), not over all-single arithmetic."""
    import torch
    t = from_program(3, [(OP_PROD, 0, [(1, 1.0), (2, 1.0)]), (OP_SUM, 0, [(0, 2.5), (3, 1.0)])], [4], name="promo").normalized()
    a = np.float32(0.1) + np.arange(1000, dtype=np.float32) * np.float32(1e-3)
    b = np.float32(1.7) - np.arange(1000, dtype=np.float32) * np.float32(3e-4)
    c = np.float32(0.3) + np.arange(1000, dtype=np.float32) * np.float32(7e-4)
    leaf = np.stack([a, b, c], axis=1)
    julia = (a.astype(np.float64) * 2.5 + (b * c).astype(np.float64)).astype(np.float32)
    single = a * np.float32(2.5) + b * c
    assert same_bits(oracle.eval_static_typed(t, leaf, "Float32")[:, 0], julia)
    sj, ss = julia.astype(np.float64).sum(), single.astype(np.float64).sum()
    bound = TOL * max(1.0, np.abs(julia.astype(np.float64)).sum())
    assert abs(sj - ss) > 2 * bound, (sj, ss, bound)                 # the two readings' sums are further apart than the tolerance
    f = fd.compile_table(t, specialize="isa")
    got = host(f.accumulate(dev_typed(cuda, leaf, "leaf_major"), None))
    assert f.last_typed_kernel == "fdg_spec_typed_acc<Float32>"
    assert abs(got[0] - sj) <= bound and abs(got[0] - ss) > bound, (got, sj, ss)


@pytest.mark.gpu
def test_python_refusals_and_the_float64_path_of_the_handle(libfdg, cuda):
    import torch
    t = workloads.get("sigma2")
    f = fd.compile_table(t, specialize="isa")
    B = 300
    z = torch.from_numpy(rand_leaves(B, t.n_leaf, "ComplexF32", 2)).to(cuda)
    with pytest.raises(TypeError):
        f.accumulate(torch.ones((B, t.n_leaf), dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError):
        f.accumulate(z, None, torch.zeros(t.n_root, dtype=torch.float64, device=cuda))          # complex leaves: a complex128 acc
    with pytest.raises(ValueError):
        f.accumulate(z.real.contiguous(), None, torch.zeros(t.n_root, dtype=torch.complex128, device=cuda))
    with pytest.raises(ValueError):
        f.accumulate(z, None, None, torch.zeros(t.n_root, dtype=torch.complex64, device=cuda))
    with pytest.raises(ValueError):
        f.accumulate(z, None, torch.zeros(t.n_root - 1, dtype=torch.complex128, device=cuda))
    with pytest.raises(ValueError):
        f.accumulate(z, None, torch.zeros(2 * t.n_root, dtype=torch.complex128, device=cuda)[::2])
    with pytest.raises(ValueError):
        f.accumulate(z, None, torch.zeros(t.n_root, dtype=torch.complex128))                      # on the host
    same = torch.zeros(t.n_root, dtype=torch.complex128, device=cuda)
    with pytest.raises(ValueError):
        f.accumulate(z, None, same, same)
    with pytest.raises(ValueError):
        f.accumulate(z, torch.ones(B, dtype=torch.float32, device=cuda))
    x64 = torch.from_numpy(rand_leaves(B, t.n_leaf, "Float64", 6)).to(cuda)
    with pytest.raises(ValueError):
        f.accumulate(x64, None, None, torch.zeros(t.n_root, dtype=torch.float64, device=cuda))    # Float64 squares: accumulate_moments
    f.accumulate(z, None)                                                                          # the typed kernels join the handle
    assert f.last_typed_kernel == "fdg_spec_typed_acc<ComplexF32>"
    w = torch.rand(B, dtype=torch.float64, device=cuda)
    fresh = fd.compile_table(t, specialize="isa")
    assert same_bits(host(f.accumulate(x64, w)), host(fresh.accumulate(x64, w)))
    # FDG_DT_F64 through the typed entry: the ordinary calls' bits
    acc = torch.zeros(t.n_root, dtype=torch.float64, device=cuda)
    with torch.cuda.device(cuda):
        f.handle.accumulate_device_typed(capi.FDG_DT_F64, x64.data_ptr(), x64.stride(0), x64.stride(1), w.data_ptr(), acc.data_ptr(), 0, B,
                                         torch.cuda.current_stream(cuda).cuda_stream)
    assert same_bits(host(acc), host(fresh.accumulate(x64, w)))
    m1, m2 = fresh.accumulate_moments(x64, weight=w)
    a1, a2 = torch.zeros(t.n_root, dtype=torch.float64, device=cuda), torch.zeros(t.n_root, dtype=torch.float64, device=cuda)
    with torch.cuda.device(cuda):
        f.handle.accumulate_device_typed(capi.FDG_DT_F64, x64.data_ptr(), x64.stride(0), x64.stride(1), w.data_ptr(), a1.data_ptr(), a2.data_ptr(),
                                         B, torch.cuda.current_stream(cuda).cuda_stream)
    assert same_bits(host(a1), host(m1).reshape(-1)) and same_bits(host(a2), host(m2).reshape(-1))
