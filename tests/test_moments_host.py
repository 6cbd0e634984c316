"""Second-moment accumulation without a device (include/fdg.h: fdg_accumulate_device_moments, fdg_mc_accumulate_device_moments): the header
declares both entry points, libfdg.so exports them, every argument check runs before any device work, the Python method forwards the
library's answer, the Julia shim binds both, and mc_estimate turns hand-computed sums into a mean and a standard error."""
import math
import os
import re

import numpy as np
import pytest

import feynmandiagram_jl_amd as fd
from feynmandiagram_jl_amd import capi, workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "fdg.h")
JL = os.path.join(ROOT, "feynmandiagram.jl_amd", "julia", "hip_compiler.jl")
NAMES = ("fdg_accumulate_device_moments", "fdg_mc_accumulate_device_moments")
FAKE = 0x10000          # pointers the checks only compare with NULL or with each other: nothing is ever read through them here
FAKE2 = 0x20000


def test_header_declares_moments_entry_points(libfdg):
    text = open(HDR).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in capi.EXPORTS
        assert hasattr(libfdg, name), name


def _acc(h, n_bin, B, d_leaf=FAKE, d_bin=FAKE, d_acc=FAKE, d_acc2=FAKE2, lts=0):
    return capi.lib().fdg_accumulate_device_moments(h._h if h else None, d_leaf, 1, 8, lts, d_bin, 0, n_bin, None, d_acc, d_acc2, B, None)


def _mc(h, n_bin, B, d_bin=FAKE, d_acc=FAKE, d_acc2=FAKE2, d_K=FAKE, d_T=FAKE):
    return capi.lib().fdg_mc_accumulate_device_moments(h._h if h else None, d_K, 1, 8, d_T, 1, 8, 1.0, 2.0, 0.5, d_bin, 1, n_bin, None,
                                                       d_acc, d_acc2, B, None)


def test_argument_checks_need_no_device(libfdg):
    h = capi.GraphHandle(workloads.get("sigma2"))
    for call in (_acc, _mc):
        assert call(h, 4, 100, d_acc=None) == capi.FDG_E_INVALID
        assert call(h, 4, 100, d_acc2=None) == capi.FDG_E_INVALID
        assert call(h, 4, 100, d_acc2=FAKE) == capi.FDG_E_INVALID           # d_acc == d_acc2
        assert call(h, 4, 100, d_bin=None) == capi.FDG_E_INVALID            # no bins: one bin only
        assert call(h, capi.FDG_BIN_MAX, 100, d_bin=None) == capi.FDG_E_INVALID
        assert call(h, 0, 100) == capi.FDG_E_INVALID
        assert call(h, 0, 100, d_bin=None) == capi.FDG_E_INVALID
        assert call(h, 4, -1) == capi.FDG_E_INVALID
        assert call(None, 4, 100) == capi.FDG_E_INVALID
        assert call(h, capi.FDG_BIN_MAX + 1, 100) == capi.FDG_E_UNSUPPORTED
        # valid arguments and nothing to do: no device work, no error
        assert call(h, capi.FDG_BIN_MAX, 0) == capi.FDG_OK
        assert call(h, 1, 0, d_bin=None) == capi.FDG_OK
    assert _acc(h, 4, 100, d_leaf=None) == capi.FDG_E_INVALID
    assert _mc(h, 4, 100, d_K=None) == capi.FDG_E_INVALID
    assert _mc(h, 4, 100, d_T=None) == capi.FDG_E_INVALID
    # a handle that never met fdg_graph_specialize_fused: the MC entry point refuses before touching the device
    assert _mc(h, 4, 100) == capi.FDG_E_INVALID
    assert _mc(h, 1, 100, d_bin=None) == capi.FDG_E_INVALID
    # a tile-major batch on a handle without FDG_SPEC_ISA
    assert _acc(h, 4, 100, lts=8 * 64) == capi.FDG_E_UNSUPPORTED


def test_python_method_forwards_the_error_code(libfdg):
    h = capi.GraphHandle(workloads.get("sigma2"))
    for kw, code in (({"n_bin": 0}, capi.FDG_E_INVALID), ({"d_acc2": FAKE}, capi.FDG_E_INVALID), ({"d_bin": 0}, capi.FDG_E_INVALID),
                     ({"n_bin": capi.FDG_BIN_MAX + 1}, capi.FDG_E_UNSUPPORTED)):
        a = dict(d_leaf=FAKE, ss=1, ls=8, lts=0, d_bin=FAKE, bin_base=0, n_bin=4, d_weight=0, d_acc=FAKE, d_acc2=FAKE2, B=100)
        a.update(kw)
        with pytest.raises(capi.FdgError) as e:
            h.accumulate_device_moments(**a)
        assert e.value.code == code, kw
    with pytest.raises(capi.FdgError) as e:
        h.mc_accumulate_device_moments(FAKE, 1, 8, FAKE, 1, 8, 1.0, 2.0, 0.5, FAKE, 1, 4, 0, FAKE, 0, 100)
    assert e.value.code == capi.FDG_E_INVALID


def test_julia_shim_binds_moments_entry_points():
    text = open(JL).read()
    export = re.search(r"^export\s+([^\n]*)", text, flags=re.M).group(1)
    for fn, sym in (("accumulate_device_moments!", NAMES[0]), ("mc_accumulate_device_moments!", NAMES[1])):
        m = re.search(r"function\s+" + re.escape(fn) + r"\(.*?\nend\b", text, flags=re.S)
        assert m, fn
        assert ":" + sym in m.group(0), fn
        assert "bin_base::Integer=1" in m.group(0), fn          # Julia's indices are 1-based
        assert "d_acc2::Ptr{Float64}" in m.group(0), fn
        assert fn in [x.strip() for x in export.split(",")], fn


def test_mc_estimate_on_hand_computed_sums():
    # samples 1, 2, 3, 6 in one bin: mean 3, sample variance (4 + 1 + 0 + 9) / 3 = 14/3, standard error sqrt(14/3 / 4)
    x = np.array([1.0, 2.0, 3.0, 6.0])
    acc, acc2 = np.array([[x.sum()]]), np.array([[(x * x).sum()]])
    mean, err = fd.mc_estimate(acc, acc2, 4)
    assert mean.shape == err.shape == (1, 1)
    assert mean[0, 0] == 3.0
    assert math.isclose(err[0, 0], math.sqrt(14.0 / 3.0 / 4.0), rel_tol=1e-15)
    # two bins, two roots; a sample outside a bin counts in N with a 0: bin 1 holds 5 of the N = 6 samples
    y = np.array([0.5, -1.0, 2.0, 4.0, 1.5])
    acc = np.array([[1.0, 2.0], [y.sum(), -y.sum()]])
    acc2 = np.array([[1.0, 4.0], [(y * y).sum(), (y * y).sum()]])
    mean, err = fd.mc_estimate(acc, acc2, 6)
    full = np.concatenate([y, [0.0]])
    assert np.allclose(mean[1], [full.mean(), -full.mean()], rtol=1e-15)
    assert np.allclose(err[1], full.std(ddof=1) / math.sqrt(6), rtol=1e-13)
    assert np.allclose(err[0], [math.sqrt((1 / 6 - 1 / 36) / 5), math.sqrt((4 / 6 - 4 / 36) / 5)], rtol=1e-13)
    # a constant integrand: zero error, and a difference that rounds below zero gives 0, not nan
    mean, err = fd.mc_estimate(np.array([0.3 * 3]), np.array([0.09 * 3 * (1 - 1e-16)]), 3)
    assert np.isfinite(err).all() and (err >= 0).all()


def test_mc_estimate_torch_and_too_few_samples():
    import torch
    acc, acc2 = torch.tensor([[6.0, 0.0]], dtype=torch.float64), torch.tensor([[14.0, 0.0]], dtype=torch.float64)
    mean, err = fd.mc_estimate(acc, acc2, 3)
    assert torch.is_tensor(mean) and torch.is_tensor(err)
    assert mean.tolist() == [[2.0, 0.0]]
    assert math.isclose(err[0, 0].item(), math.sqrt((14.0 / 3 - 4.0) / 2), rel_tol=1e-15) and err[0, 1].item() == 0.0
    for n in (1, 0, -5):
        with pytest.raises(ValueError):
            fd.mc_estimate(acc, acc2, n)
    with pytest.raises(ValueError):
        fd.mc_estimate(acc, acc2[:, :1], 3)
