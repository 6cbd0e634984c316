"""``Compilers`` -- the back-end API surface of the reference, with the HIP
evaluator as the product path.

Mirrors src/backend/compiler.jl:16-18 + static.jl + compiler_python.jl:

* ``compile(graphs; root) -> (GraphFunc, leafmap)``  (static.jl:221-227).  The
  returned callable has the generated function's semantics:
  ``f(root, leafVal)`` mutates ``root`` in place and returns the last assigned
  root value (test/compiler.jl:15,28); it also accepts a ``[B, L]`` leaf matrix
  with a ``[B, R]`` root matrix (the batched layout of compile_Python,
  compiler_python.jl:23,28,45-47) and torch CUDA tensors (zero copy).
* ``compile_Julia / compile_C / compile_Python(graphs, filename; root,
  func_name)`` append source text to a file and return ``leafmap``
  (static.jl:244-251, 269-279; compiler_python.jl:53-60).
* ``to_julia_str / to_Cstr / to_python_str`` (re-exported from lowering).

``GraphFunc`` is the name BASELINE.json's north_star uses for the callable; the
reference itself returns a RuntimeGeneratedFunction.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import capi
from .graph import Graph
from .lowering import lower, to_Cstr, to_julia_str, to_python_str
from .nodetable import FDG_NO_ROOT, NodeTable

__all__ = ["compile", "compile_hip", "compile_table", "GraphFunc", "compile_Julia", "compile_C",
           "compile_Python", "to_julia_str", "to_Cstr", "to_python_str"]


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def mc_estimate(acc, acc2, n_sample: int):
    """Mean and standard error per (bin, root) from the moments of :meth:`GraphFunc.accumulate_moments` over ``n_sample`` samples:
    ``mean = S1 / N`` and ``err = sqrt((S2 / N - mean**2) / (N - 1))``, with ``S1 = acc``, ``S2 = acc2`` and ``N = n_sample``.
    ``N`` is the whole batch, every sample whether or not it fell into the bin (a sample outside a bin contributes 0 to it).
    ``acc`` and ``acc2`` are torch tensors or numpy arrays of one shape; the results are of the same kind.  ``N < 2`` raises
    ``ValueError``: one sample has no error bar.

    Cancellation: ``S2 / N - mean**2`` subtracts two numbers of size ``mean**2``.  When ``|mean| >> std`` their difference keeps only
    about ``16 - 2 log10(|mean| / std)`` significant digits, and at ``|mean| / std`` near 1e8 nothing of the variance is left.  A
    difference that rounds below zero is reported as an error of 0, not as nan.  For such integrands shift the integrand by a known
    estimate of its mean (or centre each batch) before accumulating."""
    N = int(n_sample)
    if N < 2:
        raise ValueError(f"mc_estimate needs n_sample >= 2 (got {N}): the standard error of one sample is undefined")
    if tuple(acc.shape) != tuple(acc2.shape):
        raise ValueError("acc and acc2 must have the same shape")
    mean = acc / N
    var = (acc2 / N - mean * mean) / (N - 1)
    if _is_torch(var):
        err = var.clamp(min=0.0).sqrt()
    else:
        import numpy as np
        err = np.sqrt(np.maximum(var, 0.0))
    return mean, err


def mc_covariance(obs, cov, n_sample: int):
    """Mean and covariance of the mean of the observables of :meth:`GraphFunc.accumulate_observables` over ``n_sample`` samples:
    ``mean = S / N`` and ``C = (cov / N - mean (x) mean) / (N - 1)``, with ``S = obs [..., n_obs]``, ``cov [..., n_obs, n_obs]`` and
    ``N = n_sample`` the whole batch, as in :func:`mc_estimate`.  The diagonal of ``C`` is clamped at 0 as ``mc_estimate`` clamps its
    variance, so ``sqrt(diag(C))`` equals its error bar bit for bit; the off-diagonal entries are left as they come out.  The error of
    ``a . o`` is ``sqrt(a^T C a)``.  torch tensors or numpy arrays; the results are of the same kind."""
    N = int(n_sample)
    if N < 2:
        raise ValueError(f"mc_covariance needs n_sample >= 2 (got {N}): the covariance of one sample is undefined")
    if tuple(cov.shape) != tuple(obs.shape) + (obs.shape[-1],):
        raise ValueError("cov must have the shape of obs plus one more axis of n_obs")
    mean = obs / N
    C = (cov / N - mean[..., :, None] * mean[..., None, :]) / (N - 1)
    if _is_torch(C):
        import torch
        d = torch.diagonal(C, dim1=-2, dim2=-1)
        d.copy_(d.clamp(min=0.0))
    else:
        import numpy as np
        i = np.arange(C.shape[-1])
        C[..., i, i] = np.maximum(C[..., i, i], 0.0)
    return mean, C


class GraphFunc:
    """Callable evaluator bound to one lowered graph set (one ``fdg_graph``)."""

    def __init__(self, table: NodeTable, specialize=False, cache_dir: Optional[str] = None,
                 flags: int = 0, opt: Optional[dict] = None, association: str = "static", options: Optional[dict] = None):
        """``specialize``: "auto" (ISA, else HIP source), "isa" / "isa-autotune" (optimizing back end,
        gfx950 assembly), True / "hip" (straight-line HIP source through hiprtc), False (table
        interpreter, no JIT).
        ``options``: handle options set before anything is specialised (``fdg_graph_set_option``; what used to be FDG_* environment
        switches: ``{"FDG_ISA_W2": "1"}``).
        ``association``: which of the reference's two evaluators the results equal bit for bit -- "static", the function
        ``Compilers.compile`` generates (static.jl:13-46), or "eval", the interpreter ``eval!`` the reference's examples and
        tests call (eval.jl:1-3,15-39; example/benchmark.jl:84-86), whose products fold the already scaled operands."""
        if association not in ("static", "eval"):
            raise ValueError('association must be "static" or "eval"')
        self.table = table.normalized()
        self._specialize, self._cache_dir, self._flags = specialize, cache_dir, flags
        self.association = association
        self.handle = capi.GraphHandle(self.table)
        self.handle.set_options(options)
        if association == "eval":
            self.handle.set_association(capi.FDG_ASSOC_INTERP)
        self.n_leaf, self.n_root = self.table.n_leaf, self.table.n_root
        if specialize == "auto":
            # best available: gfx950 assembly (every Power{N}: pow_body spelled out); a graph it refuses for another reason (too few
            # registers for its roots, ...) goes through the HIP-source JIT.  Both are JIT back ends of the same ABI, not fallbacks to a CPU.
            try:
                self.handle.specialize(cache_dir, flags | capi.FDG_SPEC_ISA)
                # compile_Python's row-major [B, L] is the reference's batched layout.  Most graphs read it in place through
                # the ISA back end's row-major variant (LDS staging: 4-loop self-energies 5.7e9 evals/s against 1.7e9 for
                # the HIP-source kernels).  Handles without that variant (fewer than 16 leaves, the tiny-graph
                # configuration, plans that would re-fetch too much) would transpose chunks in front of the ISA kernel, so
                # for small graphs the HIP-source kernels, whose lanes read their own rows, ride along as a companion
                # (2-loop self-energy: 4.3e10 vs 1.5e10 evals/s).  The handle says which case it is.
                if not self.handle.kernel_info()["has_rm"] and self.n_leaf > 1 and self.table.n_node <= 4000:
                    self.handle.specialize(cache_dir, flags | capi.FDG_SPEC_ROW_MAJOR_COMPANION)
            except capi.FdgError as e:
                if e.code != capi.FDG_E_UNSUPPORTED:
                    raise
                self.handle.specialize(cache_dir, flags)
        elif specialize in ("isa", "isa-autotune"):
            if opt:
                self.handle.set_opt_params(**opt)
            if specialize == "isa-autotune":
                flags |= capi.FDG_SPEC_AUTOTUNE
            self.handle.specialize(cache_dir, flags | capi.FDG_SPEC_ISA)
        elif specialize:
            self.handle.specialize(cache_dir, flags)

    # -- introspection ------------------------------------------------------- #
    def info(self) -> dict:
        return self.handle.info()

    def kernel_info(self) -> dict:
        return self.handle.kernel_info()

    def specialize(self, cache_dir: Optional[str] = None, flags: int = 0) -> "GraphFunc":
        self.handle.specialize(cache_dir, flags)
        return self

    def _last_root_value(self, root_row):
        slots = [k for k in range(self.n_root) if int(self.table.root_slot[k]) != FDG_NO_ROOT]
        if not slots:
            return None
        # the generated function returns its last assignment: the root whose
        # statement comes last in emission order (static.jl:126-128)
        k = max(slots, key=lambda k: self._emission_rank(int(self.table.root_slot[k])))
        return float(root_row[k])

    def _emission_rank(self, v: int):
        """Position of value v's statement in the emitted text: internal node n is the (n+1)-th internal statement; a
        leaf's load comes after ``leaf_pos`` internal statements (and after the loads of lower-numbered leaves there)."""
        L = self.table.n_leaf
        if v >= L:
            return (v - L + 1, 0, 0)
        return (int(self.table.leaf_positions()[v]), 1, v) if L else (0, 1, v)

    # -- the call ------------------------------------------------------------- #
    def __call__(self, root, leafVal):
        if _is_torch(leafVal):
            return self._call_torch(root, leafVal)
        if isinstance(leafVal, np.ndarray) and leafVal.dtype in (np.float32, np.complex128, np.complex64):
            return self._call_numpy_typed(root, leafVal)
        leaf = np.asarray(leafVal, dtype=np.float64)
        if leaf.ndim == 1:
            if leaf.shape[0] < self.n_leaf:
                raise IndexError(f"BoundsError: attempt to access {leaf.shape[0]}-element leafVal at index [{self.n_leaf}]")
            if len(root) < self.n_root:
                raise IndexError(f"BoundsError: attempt to access {len(root)}-element root at index [{self.n_root}]")
            r = np.array([float(root[k]) for k in range(self.n_root)], dtype=np.float64).reshape(1, -1)
            self.handle.eval_host(leaf[None, :self.n_leaf], r)
            for k in range(self.n_root):
                root[k] = r[0, k]
            return self._last_root_value(r[0])
        if leaf.ndim != 2:
            raise ValueError("leafVal must be a vector or a [B, L] matrix")
        B = leaf.shape[0]
        if root is None:
            root = np.zeros((B, self.n_root), dtype=np.float64)
        if not (isinstance(root, np.ndarray) and root.dtype == np.float64 and (root.flags.c_contiguous or root.flags.f_contiguous)
                and root.shape == (B, self.n_root)):
            raise ValueError("root must be a contiguous float64 array of shape [B, R]")
        self.handle.eval_host(leaf, root)
        return root

    def _call_torch(self, root, leaf):
        import torch
        if not leaf.is_cuda:
            raise RuntimeError("torch leafVal must live on the GPU (no CPU fallback); pass a numpy array for host data")
        if leaf.dtype != torch.float64:
            return self._call_torch_typed(root, leaf)
        squeeze = leaf.dim() == 1
        if squeeze:
            leaf = leaf[None, :]
        B, Lc = leaf.shape
        if Lc < self.n_leaf:
            raise IndexError("BoundsError: leafVal has fewer columns than the graph has leaves")
        if root is None:
            root = torch.zeros((self.n_root,) if squeeze else (B, self.n_root), dtype=torch.float64, device=leaf.device)
        r2 = root[None, :] if squeeze else root
        if r2.dim() != 2 or r2.dtype != torch.float64 or r2.shape[0] != B or r2.shape[1] < self.n_root:
            raise ValueError("root must be a float64 [B, R] tensor on the same device")
        st = torch.cuda.current_stream(leaf.device).cuda_stream
        with torch.cuda.device(leaf.device):
            self.handle.eval_device(leaf.data_ptr(), leaf.stride(0), leaf.stride(1), r2.data_ptr(),
                                    r2.stride(0), r2.stride(1), B, st)
        return root

    # -- tile-major batches (fdg_eval_device_tiled): the layout the evaluator streams best ------------------------------ #
    @staticmethod
    def tile_major_empty(n_sample: int, n_col: int, device, dtype=None):
        """An uninitialised tile-major batch for ``n_sample`` samples of ``n_col`` values: a ``[cld(B, 64), n_col, 64]``
        tensor (tile, value, sample-in-tile) -- memory order of a Julia ``Array{Float64,3}(undef, 64, n_col, cld(B, 64))``."""
        import torch
        return torch.empty(((n_sample + 63) // 64, n_col, 64), dtype=dtype or torch.float64, device=device)

    def row_major_pair(self, n_sample: int, device, calibrate: bool = True, chunk_bytes: int = 0, verbose: bool = False) -> "PairedBatch":
        """The same for ``compile_Python``'s row-major layout: ``.leaf`` is ``[B, L]``, ``.root`` ``[B, R]`` (rows contiguous)."""
        return PairedBatch(self, n_sample, device, calibrate, chunk_bytes, verbose, capi.BATCH_PAIR_ROW_MAJOR)

    def leaf_major_pair(self, n_sample: int, device, calibrate: bool = True, verbose: bool = False) -> "PairedBatch":
        """The same for a Julia column-major pair: ``.leaf`` is ``[B, L]`` with strides ``(1, B')``, ``.root`` ``[B, R]`` with ``(1, B')``
        (``B'``: the mapped sample count).  One window -- the whole batch --, whole root matrices as candidates: pays for batches of up to a
        few tens of GB."""
        return PairedBatch(self, n_sample, device, calibrate, 0, verbose, capi.BATCH_PAIR_LEAF_MAJOR)

    def tile_major_pair(self, n_sample: int, device, calibrate: bool = True, chunk_bytes: int = 0, verbose: bool = False, extra_flags: int = 0) -> "PairedBatch":
        """The leaf and root arrays of a tile-major batch of this function, allocated by the library so that every part of the leaves
        streams next to its part of the roots at the fast rate (``fdg_batch_alloc_pair``: the root chunks are chosen by timing this
        function's own kernel on (leaf window, root chunk) pairs).  ``.leaf`` / ``.root`` are ``[cld(B, 64), L | R, 64]`` tensors viewing
        library-owned memory; call ``.free()`` (or drop the object) when done."""
        return PairedBatch(self, n_sample, device, calibrate, chunk_bytes, verbose, extra_flags)

    @staticmethod
    def tile_major_(dst, src, n_sample: Optional[int] = None):
        """``tile_major!(dst, src)``: a matrix in one of the reference's layouts -- ``src[b, c]`` with any strides: a Julia column-major
        ``B x C`` matrix (torch: ``x.t()`` of a ``[C, B]`` tensor) or ``compile_Python``'s row-major ``[B, C]`` -- into the tile-major
        ``dst[t, c, l]`` (:meth:`tile_major_empty`).  One pass at copy speed (``fdg_repack_tile_major``); returns ``dst``."""
        import torch
        if not (_is_torch(src) and src.is_cuda and src.dtype == torch.float64 and src.dim() == 2):
            raise ValueError("src must be a 2-d float64 CUDA tensor [samples, columns]")
        B = src.shape[0] if n_sample is None else int(n_sample)
        C_ = src.shape[1]
        if dst is None:
            dst = GraphFunc.tile_major_empty(B, C_, src.device)
        if not (_is_torch(dst) and dst.is_cuda and dst.dtype == torch.float64 and dst.dim() == 3 and dst.shape[2] == 64 and dst.shape[1] == C_
                and dst.is_contiguous() and dst.shape[0] >= (B + 63) // 64 and B <= src.shape[0]):
            raise ValueError("dst must be a contiguous float64 CUDA tensor [cld(B, 64), columns, 64]")
        with torch.cuda.device(src.device):
            capi.repack_tile_major(src.data_ptr(), src.stride(0), src.stride(1), dst.data_ptr(), B, C_, torch.cuda.current_stream(src.device).cuda_stream)
        return dst

    @staticmethod
    def from_tile_major_(dst, src, n_sample: Optional[int] = None):
        """``from_tile_major!(dst, src)``: the inverse of :meth:`tile_major_` -- tile-major ``src[t, c, l]`` into the matrix ``dst[b, c]`` (any strides)."""
        import torch
        if not (_is_torch(dst) and dst.is_cuda and dst.dtype == torch.float64 and dst.dim() == 2):
            raise ValueError("dst must be a 2-d float64 CUDA tensor [samples, columns]")
        B = dst.shape[0] if n_sample is None else int(n_sample)
        C_ = dst.shape[1]
        if not (_is_torch(src) and src.is_cuda and src.dtype == torch.float64 and src.dim() == 3 and src.shape[2] == 64 and src.shape[1] == C_
                and src.is_contiguous() and src.shape[0] >= (B + 63) // 64 and B <= dst.shape[0]):
            raise ValueError("src must be a contiguous float64 CUDA tensor [cld(B, 64), columns, 64]")
        with torch.cuda.device(dst.device):
            capi.unpack_tile_major(src.data_ptr(), dst.data_ptr(), dst.stride(0), dst.stride(1), B, C_, torch.cuda.current_stream(dst.device).cuda_stream)
        return dst

    def _check_tiled(self, x, n_col, what):
        import torch
        if not (_is_torch(x) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 3 and x.shape[2] == 64 and x.shape[1] >= n_col):
            raise ValueError(f"{what} must be a float64 CUDA tensor of shape [tiles, >= {n_col}, 64] (tile, value, sample in tile)")

    def eval_tiled(self, root, leaf, n_sample: Optional[int] = None):
        """``root[t, k, l] = root_k(sample 64 t + l)`` from ``leaf[t, i, l]``: both tile-major (see :meth:`tile_major_empty`),
        any strides.  ``n_sample`` defaults to all ``64 * tiles`` samples; lanes past it are neither read nor written."""
        import torch
        self._check_tiled(leaf, self.n_leaf, "leaf")
        T = leaf.shape[0]
        B = 64 * T if n_sample is None else int(n_sample)
        if not (0 <= B <= 64 * T):
            raise ValueError("n_sample exceeds the batch")
        if root is None:
            root = self.tile_major_empty(64 * T, self.n_root, leaf.device)
        self._check_tiled(root, self.n_root, "root")
        if root.shape[0] < (B + 63) // 64 or root.device != leaf.device:
            raise ValueError("root holds fewer tiles than the samples need, or lives on another device")
        st = torch.cuda.current_stream(leaf.device).cuda_stream
        with torch.cuda.device(leaf.device):
            self.handle.eval_device_tiled(leaf.data_ptr(), leaf.stride(2), leaf.stride(1), leaf.stride(0), root.data_ptr(),
                                          root.stride(2), root.stride(1), root.stride(0), B, st)
        return root

    def accumulate_tiled(self, leaf, weight=None, acc=None, n_sample: Optional[int] = None):
        """``acc[k] += sum_b weight[b] * root_k(b)`` over a tile-major leaf batch (``weight``: plain vector indexed by sample)."""
        self._check_tiled(leaf, self.n_leaf, "leaf")
        B = 64 * leaf.shape[0] if n_sample is None else int(n_sample)
        if not (0 <= B <= 64 * leaf.shape[0]):
            raise ValueError("n_sample exceeds the batch")
        acc = self._out(acc, (self.n_root,), leaf, "acc", at_least=True)
        weight = self._weight(weight, B, leaf)
        w = 0 if weight is None else weight.data_ptr()
        with self._stream(leaf) as st:
            self.handle.accumulate_device_tiled(leaf.data_ptr(), leaf.stride(2), leaf.stride(1), leaf.stride(0), w, acc.data_ptr(), B, st)
        return acc

    def accumulate_binned(self, leaf, bins, n_bin: int, weight=None, acc=None, bin_base: int = 0, n_sample: Optional[int] = None):
        """The ``measure`` step of an observable that is a function of an external variable:
        ``acc[j, k] += weight[b] * root_k(b)`` for every sample ``b`` with ``0 <= j = bins[b] - bin_base < n_bin`` (other samples add
        nothing).  ``leaf`` is a float64 ``[B, L]`` CUDA tensor (any strides) or a tile-major ``(T, L, 64)`` batch (as
        :meth:`accumulate_tiled` takes it); ``bins`` an int32 CUDA vector and ``weight`` a float64 one, both indexed by sample; ``acc`` a
        contiguous float64 ``[n_bin, R]`` tensor (zeros when omitted), returned.  Deterministic: no float atomics (fdg_accumulate_device_binned)."""
        B, n_bin, bins, weight, strides = self._binned_args(leaf, bins, n_bin, weight, n_sample)
        w = 0 if weight is None else weight.data_ptr()
        acc = self._out(acc, (n_bin, self.n_root), leaf, "acc")
        with self._stream(leaf) as st:
            self.handle.accumulate_device_binned(leaf.data_ptr(), *strides, bins.data_ptr(), int(bin_base), n_bin, w, acc.data_ptr(), B, st)
        return acc

    def accumulate_moments(self, leaf, bins=None, n_bin: int = 1, weight=None, acc=None, acc2=None, bin_base: int = 0,
                           n_sample: Optional[int] = None):
        """:meth:`accumulate_binned` with the second moment, for Monte-Carlo error bars: with ``t = weight[b] * root_k(b)``,
        ``acc[j, k] += t`` and ``acc2[j, k] += t * t`` for the samples in bin ``j``.  ``bins=None``: every sample is in bin 0 and
        ``n_bin`` must be 1.  ``acc`` comes out with the bits :meth:`accumulate_binned` gives for the same arguments (an all-zero
        ``bins`` for ``bins=None``).  Returns ``(acc, acc2)``, two float64 ``[n_bin, R]`` tensors (zeros when omitted), added to.
        :func:`mc_estimate` turns them into a mean and a standard error (fdg_accumulate_device_moments)."""
        B, n_bin, bins, weight, strides = self._binned_args(leaf, bins, n_bin, weight, n_sample, bins_optional=True)
        w = 0 if weight is None else weight.data_ptr()
        acc = self._out(acc, (n_bin, self.n_root), leaf, "acc")
        acc2 = self._out(acc2, (n_bin, self.n_root), leaf, "acc2")
        self._distinct("acc and acc2", acc, acc2)
        with self._stream(leaf) as st:
            self.handle.accumulate_device_moments(leaf.data_ptr(), *strides, 0 if bins is None else bins.data_ptr(), int(bin_base), n_bin,
                                                  w, acc.data_ptr(), acc2.data_ptr(), B, st)
        return acc, acc2

    def accumulate_vegas(self, leaf, weight, hist, seed: int, sample_offset: int, n_dim: int, n_grid: int, coef=None, acc=None, acc2=None,
                         n_sample: Optional[int] = None):
        """The accumulate step of one VEGAS iteration: :meth:`accumulate_moments` with ``bins=None`` (``acc``, ``acc2``: the same bits)
        plus the training histogram ``hist[d, c] += (weight[b] * sum_k coef[k] * root_k(b))**2`` for every variable ``d < n_dim``, ``c``
        the cell of sample ``b`` in ``d`` recomputed from the Philox counter ``(sample_offset + b, d)`` and ``seed`` -- the arguments
        ``capi.vegas_sample_device`` drew the samples with.  ``hist``: a contiguous float64 ``[n_dim, n_grid]`` CUDA tensor, added to
        (zeros when None); ``coef``: host sequence of ``n_root`` factors or None (the plain sum of the roots).  Returns
        ``(acc, acc2, hist)``.  Deterministic: no float atomics (fdg_accumulate_device_vegas)."""
        B, _, _, weight, strides = self._binned_args(leaf, None, 1, weight, n_sample, bins_optional=True)
        n_dim, n_grid = self._vegas_map(n_dim, n_grid)
        w = 0 if weight is None else weight.data_ptr()
        acc = self._out(acc, (1, self.n_root), leaf, "acc")
        acc2 = self._out(acc2, (1, self.n_root), leaf, "acc2")
        hist = self._out(hist, (n_dim, n_grid), leaf, "hist")
        self._distinct("acc, acc2 and hist", acc, acc2, hist)
        with self._stream(leaf) as st:
            self.handle.accumulate_device_vegas(leaf.data_ptr(), *strides, w, coef, int(seed), int(sample_offset), n_dim, n_grid,
                                                acc.data_ptr(), acc2.data_ptr(), hist.data_ptr(), B, st)
        return acc, acc2, hist

    def accumulate_vegas_binned(self, leaf, bins, n_bin: int, weight, hist, hist_bin, seed: int, sample_offset: int, n_dim: int, n_grid: int,
                                coef=None, acc=None, acc2=None, bin_base: int = 0, n_sample: Optional[int] = None, train_bins: bool = True):
        """The accumulate step of one VEGAS iteration with a discrete variable: :meth:`accumulate_moments` with ``bins`` (``acc``, ``acc2``
        ``[n_bin, R]``: the same bits), the training histogram of :meth:`accumulate_vegas` over the samples whose bin is in range (the same
        bits when every one is), and ``hist_bin[j] += (weight[b] * sum_k coef[k] * root_k(b))**2`` over the samples of bin ``j`` -- what
        ``vegas.DiscreteMap.refine`` takes.  ``hist``: contiguous float64 ``[n_dim, n_grid]``, ``hist_bin``: contiguous float64 ``[n_bin]``,
        both CUDA tensors, added to (zeros when None; ``train_bins=False``: no ``hist_bin``, None is returned for it).  The roots of a chunk
        are evaluated once.  Returns ``(acc, acc2, hist, hist_bin)``.  Deterministic: no float atomics (fdg_accumulate_device_vegas_binned)."""
        B, n_bin, bins, weight, strides = self._binned_args(leaf, bins, n_bin, weight, n_sample)
        n_dim, n_grid = self._vegas_map(n_dim, n_grid)
        w = 0 if weight is None else weight.data_ptr()
        acc = self._out(acc, (n_bin, self.n_root), leaf, "acc")
        acc2 = self._out(acc2, (n_bin, self.n_root), leaf, "acc2")
        hist = self._out(hist, (n_dim, n_grid), leaf, "hist")
        if hist_bin is not None or train_bins:            # (a hist_bin given with train_bins=False is checked, then left alone)
            hist_bin = self._out(hist_bin, (n_bin,), leaf, "hist_bin")
        if not train_bins:
            hist_bin = None
        self._distinct("acc, acc2, hist and hist_bin", acc, acc2, hist, hist_bin)
        with self._stream(leaf) as st:
            self.handle.accumulate_device_vegas_binned(leaf.data_ptr(), *strides, bins.data_ptr(), int(bin_base), n_bin, w, coef, int(seed),
                                                       int(sample_offset), n_dim, n_grid, acc.data_ptr(), acc2.data_ptr(), hist.data_ptr(),
                                                       0 if hist_bin is None else hist_bin.data_ptr(), B, st)
        return acc, acc2, hist, hist_bin

    def accumulate_matsubara(self, leaf, T, freq, root_tau_in, root_tau_out, beta: float, fermionic: bool = True, bins=None, n_bin: int = 1,
                             weight=None, sums=None, bin_base: int = 0, n_sample: Optional[int] = None):
        """The ``measure`` step of Sigma(i omega_n) or a vertex at given frequencies: every root times the phase of ITS pair of external
        times.  With ``t = weight[b] * root_k(b)``, ``tau = T[b, root_tau_out[k] - 1] - T[b, root_tau_in[k] - 1]`` and
        ``(s, c) = capi.matsubara_phase(tau, beta, freq[f], fermionic)``, the samples of bin ``j`` add ``t * c``, ``t * s`` and the
        squares of both to entry ``[j, f, k]`` of ``sums[0] .. sums[3]``.  ``T``: float64 ``[B, n_tau]`` CUDA tensor (any strides);
        ``freq``: host sequence of at most ``capi.FDG_MATSUBARA_FREQ_MAX`` integers ``n``; the labels: host sequences of ``n_root``
        1-based indices (``workloads.root_times``); ``bins=None``: every sample in bin 0.  ``sums``: a contiguous float64
        ``[4, n_bin, n_freq, R]`` tensor, added to (zeros when None).  Returns ``(acc, acc2_re, acc2_im)``: ``acc`` the complex
        ``[n_bin, n_freq, R]`` sums of ``t * e^{i omega_n tau}`` (a copy), the other two views of ``sums``; :func:`mc_estimate` on
        ``(acc.real, acc2_re)`` and ``(acc.imag, acc2_im)`` gives the error bars.  Deterministic: no float atomics
        (fdg_accumulate_device_matsubara)."""
        import torch
        B, n_bin, bins, weight, strides = self._binned_args(leaf, bins, n_bin, weight, n_sample, bins_optional=True)
        if not (_is_torch(T) and T.is_cuda and T.device == leaf.device and T.dtype == torch.float64 and T.dim() == 2 and T.shape[0] >= B):
            raise ValueError("T must be a float64 [B, n_tau] CUDA tensor on the leaves' device")
        n_freq = len(freq)
        if not (1 <= n_freq <= capi.FDG_MATSUBARA_FREQ_MAX and n_bin * n_freq <= capi.FDG_BIN_MAX):
            raise ValueError(f"need 1 .. {capi.FDG_MATSUBARA_FREQ_MAX} frequencies and n_bin * n_freq <= {capi.FDG_BIN_MAX}")
        if len(root_tau_in) != self.n_root or len(root_tau_out) != self.n_root:
            raise ValueError("root_tau_in and root_tau_out hold one label per root")
        sums = self._out(sums, (4, n_bin, n_freq, self.n_root), leaf, "sums")
        p = [sums[i].data_ptr() for i in range(4)]
        desc, _keep = capi.make_matsubara(freq, fermionic, root_tau_in, root_tau_out, beta, T.shape[1], p[0], p[1], p[2], p[3],
                                          T.data_ptr(), T.stride(0), T.stride(1))
        with self._stream(leaf) as st:
            self.handle.accumulate_device_matsubara(leaf.data_ptr(), *strides, 0 if bins is None else bins.data_ptr(), int(bin_base), n_bin,
                                                    0 if weight is None else weight.data_ptr(), desc, B=B, stream=st)
        return torch.complex(sums[0], sums[1]), sums[2], sums[3]

    def accumulate_observables(self, leaf, coef, bins=None, n_bin: int = 1, weight=None, obs=None, cov=None, acc=None, acc2=None,
                               moments: bool = False, bin_base: int = 0, n_sample: Optional[int] = None):
        """Linear combinations of the roots and their second moments, for the error bar of a sum, a difference or a series of
        roots that share their samples: with ``t_k = weight[b] * root_k(b)`` and ``o_m = sum_k coef[m, k] * t_k`` (a left fold over
        ascending ``k``, zero coefficients skipped), the samples of bin ``j`` add ``o_m`` to ``obs[j, m]`` and ``o_a * o_c`` to
        ``cov[j, a, c]`` (symmetric, both triangles written).  ``coef``: host ``[n_obs, R]`` with ``n_obs <= capi.FDG_OBS_MAX``;
        ``obs`` / ``cov``: contiguous float64 ``[n_bin, n_obs]`` / ``[n_bin, n_obs, n_obs]`` CUDA tensors, added to (zeros when None).
        ``moments=True`` (or ``acc`` / ``acc2`` given): the per-root moments of :meth:`accumulate_moments` too, with its bits, from the
        same evaluation of the roots.  Returns ``(obs, cov)`` or ``(obs, cov, acc, acc2)``; :func:`mc_covariance` turns the first two
        into a mean and a covariance.  Real observables of unprojected roots only.  Deterministic: no float atomics
        (fdg_accumulate_device_observables)."""
        import numpy as np
        B, n_bin, bins, weight, strides = self._binned_args(leaf, bins, n_bin, weight, n_sample, bins_optional=True)
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != self.n_root or not (1 <= c.shape[0] <= capi.FDG_OBS_MAX):
            raise ValueError(f"coef must be [n_obs, n_root = {self.n_root}] with 1 <= n_obs <= {capi.FDG_OBS_MAX}")
        obs = self._out(obs, (n_bin, c.shape[0]), leaf, "obs")
        cov = self._out(cov, (n_bin, c.shape[0], c.shape[0]), leaf, "cov")
        moments = moments or acc is not None or acc2 is not None
        if moments:
            acc = self._out(acc, (n_bin, self.n_root), leaf, "acc")
            acc2 = self._out(acc2, (n_bin, self.n_root), leaf, "acc2")
        self._distinct("obs, cov, acc and acc2", obs, cov, acc, acc2)
        desc, _keep = capi.make_observables(c, obs.data_ptr(), cov.data_ptr())
        with self._stream(leaf) as st:
            self.handle.accumulate_device_observables(leaf.data_ptr(), *strides, 0 if bins is None else bins.data_ptr(), int(bin_base),
                                                      n_bin, 0 if weight is None else weight.data_ptr(), desc,
                                                      d_acc=acc.data_ptr() if moments else 0, d_acc2=acc2.data_ptr() if moments else 0,
                                                      B=B, stream=st)
        return (obs, cov, acc, acc2) if moments else (obs, cov)

    def accumulate_freq_observables(self, leaf, T, freq, root_tau_in, root_tau_out, beta: float, coef, fermionic: bool = True, bins=None,
                                    n_bin: int = 1, weight=None, fobs=None, fcov=None, sums=None, projection: bool = False,
                                    bin_base: int = 0, n_sample: Optional[int] = None):
        """Linear combinations of the PROJECTED roots and their second moments: the error bar of a frequency-resolved sum, difference
        or series of roots that share their samples.  With ``tre_k`` / ``tim_k`` the real and imaginary parts of root ``k`` times the
        phase of its own time pair at frequency ``f``, as :meth:`accumulate_matsubara` forms them, ``a_m = sum_k coef[m, k] * tre_k``
        and ``b_m`` the same with ``tim_k`` (left folds over ascending ``k``, zero coefficients skipped) and ``z = (a_0 .., b_0 ..)``,
        the samples of bin ``j`` add ``z_p`` to ``fobs[j, f, p]`` and ``z_p * z_q`` to ``fcov[j, f, p, q]`` (symmetric, both triangles
        written).  ``coef``: host real ``[M, R]`` with ``M <= capi.FDG_FREQ_OBS_MAX``; ``fobs`` / ``fcov``: contiguous float64
        ``[n_bin, n_freq, 2 M]`` / ``[n_bin, n_freq, 2 M, 2 M]`` CUDA tensors, added to (zeros when None).  ``projection=True`` (or
        ``sums`` given): the per-root sums of :meth:`accumulate_matsubara` too, with its bits, from the same evaluation of the roots.
        Returns ``(fobs, fcov)`` or ``(fobs, fcov, sums)``; :func:`mc_covariance` on ``fobs`` / ``fcov`` with the leading two axes
        folded gives the mean and covariance of the ``2 M`` real components.  Deterministic: no float atomics
        (fdg_accumulate_device_freq_observables)."""
        import numpy as np
        import torch
        B, n_bin, bins, weight, strides = self._binned_args(leaf, bins, n_bin, weight, n_sample, bins_optional=True)
        if not (_is_torch(T) and T.is_cuda and T.device == leaf.device and T.dtype == torch.float64 and T.dim() == 2 and T.shape[0] >= B):
            raise ValueError("T must be a float64 [B, n_tau] CUDA tensor on the leaves' device")
        n_freq = len(freq)
        if not (1 <= n_freq <= capi.FDG_MATSUBARA_FREQ_MAX and n_bin * n_freq <= capi.FDG_BIN_MAX):
            raise ValueError(f"need 1 .. {capi.FDG_MATSUBARA_FREQ_MAX} frequencies and n_bin * n_freq <= {capi.FDG_BIN_MAX}")
        if len(root_tau_in) != self.n_root or len(root_tau_out) != self.n_root:
            raise ValueError("root_tau_in and root_tau_out hold one label per root")
        c = np.ascontiguousarray(coef, dtype=np.float64)
        if c.ndim != 2 or c.shape[1] != self.n_root or not (1 <= c.shape[0] <= capi.FDG_FREQ_OBS_MAX):
            raise ValueError(f"coef must be [n_obs, n_root = {self.n_root}] with 1 <= n_obs <= {capi.FDG_FREQ_OBS_MAX}")
        P = 2 * c.shape[0]
        fobs = self._out(fobs, (n_bin, n_freq, P), leaf, "fobs")
        fcov = self._out(fcov, (n_bin, n_freq, P, P), leaf, "fcov")
        projection = projection or sums is not None
        if projection:
            sums = self._out(sums, (4, n_bin, n_freq, self.n_root), leaf, "sums")
        self._distinct("fobs, fcov and sums", fobs, fcov, sums)
        p = [sums[i].data_ptr() if projection else 0 for i in range(4)]
        desc, _keep = capi.make_matsubara(freq, fermionic, root_tau_in, root_tau_out, beta, T.shape[1], p[0], p[1], p[2], p[3],
                                          T.data_ptr(), T.stride(0), T.stride(1))
        fo, _keep_c = capi.make_freq_observables(c, fobs.data_ptr(), fcov.data_ptr())
        with self._stream(leaf) as st:
            self.handle.accumulate_device_freq_observables(leaf.data_ptr(), *strides, 0 if bins is None else bins.data_ptr(), int(bin_base),
                                                           n_bin, 0 if weight is None else weight.data_ptr(), fo, desc, B=B, stream=st)
        return (fobs, fcov, sums) if projection else (fobs, fcov)

    def _binned_args(self, leaf, bins, n_bin, weight, n_sample, bins_optional=False):
        """The checks of :meth:`accumulate_binned` / :meth:`accumulate_moments`: (n_sample, n_bin, bins, weight, leaf strides), bins and
        weight contiguous (the caller holds them until the launch is queued)."""
        import torch
        tiled = _is_torch(leaf) and leaf.dim() == 3
        if not (_is_torch(leaf) and leaf.is_cuda and leaf.dtype == torch.float64 and leaf.dim() in (2, 3)):
            raise TypeError("leaf must be a float64 [B, L] CUDA tensor or a tile-major [tiles, L, 64] one")
        if tiled:
            self._check_tiled(leaf, self.n_leaf, "leaf")
            cap = 64 * leaf.shape[0]
        else:
            if leaf.shape[1] < self.n_leaf:
                raise IndexError("BoundsError: leafVal has fewer columns than the graph has leaves")
            cap = leaf.shape[0]
        B = cap if n_sample is None else int(n_sample)
        if not (0 <= B <= cap):
            raise ValueError("n_sample exceeds the batch")
        n_bin = int(n_bin)
        if not (1 <= n_bin <= capi.FDG_BIN_MAX):
            raise ValueError(f"n_bin must lie in [1, {capi.FDG_BIN_MAX}]")
        if bins is None and bins_optional:
            if n_bin != 1:
                raise ValueError("bins=None puts every sample in bin 0: n_bin must be 1")
        else:
            if not (_is_torch(bins) and bins.is_cuda):
                raise TypeError("bins must be an int32 CUDA tensor")
            if bins.dtype != torch.int32:
                raise TypeError(f"bins must be an int32 CUDA tensor, not {bins.dtype}")
            if bins.dim() != 1 or bins.shape[0] < B or bins.device != leaf.device:
                raise ValueError("bins must be an int32 vector of at least n_sample elements on the leaves' device")
            bins = bins.contiguous()
        weight = self._weight(weight, B, leaf)
        strides = (leaf.stride(2), leaf.stride(1), leaf.stride(0)) if tiled else (leaf.stride(0), leaf.stride(1), 0)
        return B, n_bin, bins, weight, strides

    def _out(self, x, shape, leaf, what, at_least=False):
        """An output of the ``accumulate_*`` methods: ``x`` checked as a contiguous float64 CUDA tensor of ``shape`` on the leaves'
        device, zeros when None.  ``at_least`` (:meth:`accumulate_tiled`): any shape of at least ``n_root`` elements."""
        import torch
        if x is None:
            x = torch.zeros(shape, dtype=torch.float64, device=leaf.device)
        if (not _is_torch(x) or not x.is_cuda or x.device != leaf.device or x.dtype != torch.float64 or not x.is_contiguous()
                or (x.numel() < self.n_root if at_least else tuple(x.shape) != shape)):
            size = "tensor of at least n_root elements" if at_least else f"{list(shape)} tensor"
            raise ValueError(f"{what} must be a contiguous float64 {size} on the leaves' device")
        return x

    @staticmethod
    def _weight(weight, B, leaf):
        """``weight`` checked as a float64 vector of at least ``B`` elements on the leaves' device and made contiguous (None stays None)."""
        import torch
        if weight is None:
            return None
        if (not _is_torch(weight) or not weight.is_cuda or weight.device != leaf.device or weight.dtype != torch.float64
                or weight.dim() != 1 or weight.shape[0] < B):
            raise ValueError("weight must be a float64 vector of at least n_sample elements on the leaves' device")
        return weight.contiguous()

    @staticmethod
    def _vegas_map(n_dim, n_grid):
        n_dim, n_grid = int(n_dim), int(n_grid)
        if not (1 <= n_dim <= capi.FDG_VEGAS_DIM_MAX and 1 <= n_grid <= capi.FDG_VEGAS_GRID_MAX):
            raise ValueError(f"n_dim must lie in [1, {capi.FDG_VEGAS_DIM_MAX}] and n_grid in [1, {capi.FDG_VEGAS_GRID_MAX}]")
        return n_dim, n_grid

    @staticmethod
    def _distinct(names, *outs):
        """No two of the output tensors (None: not given) may start at the same address."""
        outs = [o for o in outs if o is not None]
        if len({o.data_ptr() for o in outs}) != len(outs):
            raise ValueError(f"{names} must be different tensors")

    @staticmethod
    @contextlib.contextmanager
    def _stream(leaf):
        """The leaves' device made current for the call; yields the raw handle of its current stream."""
        import torch
        st = torch.cuda.current_stream(leaf.device).cuda_stream
        with torch.cuda.device(leaf.device):
            yield st

    def _call_numpy_typed(self, root, leaf):
        """Host arrays of an element type other than Float64: staged through the device (there is no CPU evaluator behind the ABI)."""
        import torch
        if not torch.cuda.is_available():
            raise capi.FdgError(capi.FDG_E_NO_DEVICE, "no gfx950 device: the evaluator has no CPU fallback")
        vec = leaf.ndim == 1
        d_leaf = torch.from_numpy(np.ascontiguousarray(leaf)).cuda()
        live = [k for k in range(self.n_root) if int(self.table.root_slot[k]) != FDG_NO_ROOT]
        if vec:
            if leaf.shape[0] < self.n_leaf:
                raise IndexError(f"BoundsError: attempt to access {leaf.shape[0]}-element leafVal at index [{self.n_leaf}]")
            if root is None:
                root = np.zeros(self.n_root, dtype=leaf.dtype)
            if len(root) < self.n_root:
                raise IndexError(f"BoundsError: attempt to access {len(root)}-element root at index [{self.n_root}]")
        d_root = self._call_torch_typed(None, d_leaf)
        torch.cuda.synchronize()
        h = d_root.cpu().numpy()
        if vec:
            h = h.reshape(-1)
            for k in live:                   # (root[k] of an id that is in no graph keeps the caller's value, as in the generated function)
                root[k] = h[k]
            return h[max(live, key=lambda k: self._emission_rank(int(self.table.root_slot[k])))] if live else None
        if root is None:
            return h
        root[:, live] = h[:, live]
        return root

    def _typed_dtype(self, leaf) -> int:
        """FDG_DT_* of a Float32 / ComplexF64 / ComplexF32 tensor; the type's kernels are compiled on first use."""
        import torch
        dt = {torch.float32: capi.FDG_DT_F32, torch.complex128: capi.FDG_DT_C64, torch.complex64: capi.FDG_DT_C32}.get(leaf.dtype)
        if dt is None:
            raise TypeError(f"leafVal of element type {leaf.dtype} is not supported (Float64, Float32, ComplexF64, ComplexF32)")
        if not hasattr(self, "_typed_ready"):
            self._typed_ready = set()
        if dt not in self._typed_ready:
            # (FDG_SPEC_ISA: ComplexF64 rows -- compile_Python's row-major [B, L] -- additionally get the graph spelled out on real and
            # imaginary parts through the Float64 assembly back end; the library decides per call which kernel a layout takes)
            isa = self._specialize in ("isa", "isa-autotune", "auto")
            self.handle.specialize_typed(dt, self._cache_dir, capi.FDG_SPEC_ISA if isa else 0)
            self._typed_ready.add(dt)
        return dt

    def _call_torch_typed(self, root, leaf):
        """Element types other than Float64: the generated function is generic in ``eltype(leafVal)`` (static.jl:98-133; the
        types ``julia_to_C_typestr`` names, static.jl:135-153).  Float32, ComplexF64 and ComplexF32 tensors go through the
        per-type kernel of ``fdg_graph_specialize_typed`` (compiled on first use); ``root`` has the leaves' type."""
        import torch
        dt = self._typed_dtype(leaf)
        squeeze = leaf.dim() == 1
        if squeeze:
            leaf = leaf[None, :]
        B, Lc = leaf.shape
        if Lc < self.n_leaf:
            raise IndexError("BoundsError: leafVal has fewer columns than the graph has leaves")
        if root is None:
            root = torch.zeros((self.n_root,) if squeeze else (B, self.n_root), dtype=leaf.dtype, device=leaf.device)
        r2 = root[None, :] if squeeze else root
        if r2.dim() != 2 or r2.dtype != leaf.dtype or not r2.is_cuda or r2.shape[0] != B or r2.shape[1] < self.n_root:
            raise ValueError("root must be a [B, R] tensor of the leaves' element type on the same device")
        st = torch.cuda.current_stream(leaf.device).cuda_stream
        with torch.cuda.device(leaf.device):
            self.handle.eval_device_typed(dt, leaf.data_ptr(), leaf.stride(0), leaf.stride(1), r2.data_ptr(), r2.stride(0), r2.stride(1), B, st)
        self.last_typed_kernel = self.handle.kernel_info()["last_kernel"]
        return root

    def accumulate(self, leaf, weight=None, acc=None, acc2=None):
        """``acc[k] += sum_b weight[b] * root_k(b)`` on device (torch tensors).  ``leaf``: a float64, float32, complex128 or
        complex64 ``[B, L]`` CUDA tensor of any strides; ``weight``: a float64 vector (None: weight 1).  ``acc`` is float64 ``[R]``
        for real leaves and complex128 ``[R]`` for complex ones (the weights are real: real and imaginary parts are summed
        separately), zeros when omitted, returned.  For the types other than float64 the roots are summed as the evaluator would
        have stored them in the leaves' type, widened to double (fdg_accumulate_device_typed; ``last_typed_kernel`` names the
        kernel), and ``acc2``, when given, receives ``sum_b (weight[b] * root_k(b))**2`` per component.  For float64 leaves
        ``acc2`` is refused: :meth:`accumulate_moments` is that call."""
        import torch
        if not leaf.is_cuda or leaf.dim() != 2 or leaf.dtype not in (torch.float64, torch.float32, torch.complex128, torch.complex64):
            raise TypeError("leaf must be a float64, float32, complex128 or complex64 [B, L] CUDA tensor")
        if leaf.shape[1] < self.n_leaf:
            raise IndexError("BoundsError: leafVal has fewer columns than the graph has leaves")
        typed = leaf.dtype != torch.float64
        if acc2 is not None and not typed:
            raise ValueError("acc2 with float64 leaves: use accumulate_moments")
        adt = torch.complex128 if leaf.dtype.is_complex else torch.float64
        if acc is None:
            acc = torch.zeros(self.n_root, dtype=adt, device=leaf.device)
        for name, a in (("acc", acc), ("acc2", acc2)):
            if a is not None and (not _is_torch(a) or not a.is_cuda or a.device != leaf.device or a.dtype != adt or not a.is_contiguous()
                                  or a.numel() < self.n_root):
                raise ValueError(f"{name} must be a contiguous {adt} tensor of at least n_root elements on the leaves' device")
        if acc2 is not None:
            self._distinct("acc and acc2", acc, acc2)
        w = 0
        if weight is not None:
            if (not weight.is_cuda or weight.device != leaf.device or weight.dtype != torch.float64 or weight.dim() != 1
                    or weight.shape[0] < leaf.shape[0]):
                raise ValueError("weight must be a float64 vector of at least B elements on the leaves' device")
            weight = weight.contiguous()
            w = weight.data_ptr()
        dt = self._typed_dtype(leaf) if typed else capi.FDG_DT_F64
        st = torch.cuda.current_stream(leaf.device).cuda_stream
        with torch.cuda.device(leaf.device):
            if typed:
                self.handle.accumulate_device_typed(dt, leaf.data_ptr(), leaf.stride(0), leaf.stride(1), w, acc.data_ptr(),
                                                    0 if acc2 is None else acc2.data_ptr(), leaf.shape[0], st)
                self.last_typed_kernel = self.handle.kernel_info()["last_kernel"]
            else:
                self.handle.accumulate_device(leaf.data_ptr(), leaf.stride(0), leaf.stride(1), w, acc.data_ptr(),
                                              leaf.shape[0], st)
        return acc


def compile_table(table: NodeTable, specialize: bool = False, **kw) -> GraphFunc:
    return GraphFunc(table, specialize=specialize, **kw)


def compile(graphs: Sequence[Graph], root: Optional[Sequence[int]] = None, specialize="auto",
            **kw) -> Tuple[GraphFunc, Dict[int, Graph]]:
    """``Compilers.compile`` (static.jl:221-227): returns ``(f, leafmap)``."""
    table, leafmap, _ = lower(graphs, root)
    return GraphFunc(table, specialize=specialize, **kw), leafmap


compile_hip = compile


def _append(filename: str, text: str, header: str = "") -> None:
    with open(filename, "a") as f:
        if header and f.tell() == 0:
            f.write(header)
        f.write(text)


def compile_Julia(graphs, filename: str, root=None, func_name: str = "eval_graph!"):
    s, leafmap = to_julia_str(graphs, root=root, name=func_name)
    _append(filename, s)
    return leafmap


def compile_C(graphs, filename: str, datatype="Float64", root=None, func_name: str = "eval_graph"):
    s, leafmap = to_Cstr(graphs, root=root, datatype=datatype, name=func_name)
    _append(filename, s, "#include <math.h>\n")    # static.jl:272-276
    return leafmap


def compile_Python(graphs, filename: str, root=None, func_name: str = "eval_graph"):
    s, leafmap = to_python_str(graphs, root=root, name=func_name)
    _append(filename, s)
    return leafmap


class _DeviceView:
    """A device address as something ``torch.as_tensor`` can wrap without copying (CUDA array interface v2)."""

    def __init__(self, ptr: int, shape):
        self.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


class PairedBatch:
    """``GraphFunc.tile_major_pair``: tile-major leaves and roots backed by ``fdg_batch_alloc_pair`` (include/fdg.h)."""

    def __init__(self, func, n_sample, device, calibrate=True, chunk_bytes=0, verbose=False, extra_flags=0):
        import torch
        device = torch.device(device)
        if func.handle is None or device.type != "cuda":
            raise capi.FdgError(capi.FDG_E_UNSUPPORTED, "tile_major_pair needs a device handle specialised with the ISA back end and a CUDA device")
        L, R = func.n_leaf, func.n_root
        self.n_sample = int(n_sample)
        with torch.cuda.device(device):
            self._lp, self._rp, self.info = capi.batch_alloc_pair(func.handle, self.n_sample, chunk_bytes, calibrate, verbose, extra_flags)
            T = (self.n_sample + 63) // 64
            if extra_flags & capi.BATCH_PAIR_LEAF_MAJOR:
                Bp = int(self.info["chunk_tiles"]) * 64
                self.leaf = torch.as_tensor(_DeviceView(self._lp, (L, Bp)), device=device).t()[:self.n_sample]
                self.root = torch.as_tensor(_DeviceView(self._rp, (R, Bp)), device=device).t()[:self.n_sample]
            elif extra_flags & capi.BATCH_PAIR_ROW_MAJOR:
                self.leaf = torch.as_tensor(_DeviceView(self._lp, (self.info["leaf_bytes"] // (8 * L), L)), device=device)[:self.n_sample]
                self.root = torch.as_tensor(_DeviceView(self._rp, (self.info["root_bytes"] // (8 * R), R)), device=device)[:self.n_sample]
            else:
                self.leaf = torch.as_tensor(_DeviceView(self._lp, (self.info["leaf_bytes"] // (512 * L), L, 64)), device=device)[:T]
                self.root = torch.as_tensor(_DeviceView(self._rp, (self.info["root_bytes"] // (512 * R), R, 64)), device=device)[:T]
        if self.leaf.data_ptr() != self._lp or self.root.data_ptr() != self._rp:
            self.free()
            raise capi.FdgError(capi.FDG_E_INTERNAL, "torch copied the library's batch instead of viewing it")
        self._device = device

    def free(self):
        import torch
        lp, rp = getattr(self, "_lp", 0), getattr(self, "_rp", 0)
        self._lp = self._rp = 0
        self.leaf = self.root = None
        if lp or rp:
            with torch.cuda.device(self._device) if hasattr(self, "_device") else _nullcontext():
                if lp:
                    capi.batch_free(lp)
                if rp:
                    capi.batch_free(rp)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _nullcontext:
    def __enter__(self): return self
    def __exit__(self, *a): return False
