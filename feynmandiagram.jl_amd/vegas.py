"""VEGAS importance sampling for the device Monte-Carlo step (include/fdg.h: fdg_vegas_sample_device, fdg_mc_accumulate_device_vegas,
fdg_vegas_refine): a separable piecewise-linear map per integration variable, refined between iterations from a histogram of
``(f * jacobian)**2`` per variable and grid cell.  The reference's examples hand their integrand to MCIntegration, whose default solver
this is (example/benchmark.jl:46-51); MCIntegration is not part of the reference checkout, so nothing here has a counterpart in it.

An iteration is "draw ``n_sample`` points through a fixed map, evaluate, accumulate": the sampler writes component-major ``(K, T)``
columns, which the one-kernel Monte-Carlo route reads in place, and the accumulate call leaves the estimate, its second moment and the
training histogram on the device.  Only the histogram (``n_dim * n_grid`` doubles) and the two moments come to the host per iteration.

A discrete variable (``DiscreteMap``, ``vegas_integrate_binned``; fdg_vegas_sample_device_discrete, fdg_mc_accumulate_device_vegas_binned,
fdg_vegas_refine_discrete) picks one of ``n_bin`` external configurations per sample -- ``ExtKidx = MCIntegration.Discrete(1, Nk)`` of the
reference's test/ver4.jl:221-250 -- so that one run fills an observable ``[n_bin, R]`` and trains the variable's probabilities with the map.

Spherical momentum variables (``PolarVar``, ``ball``, the keyword ``polar``; fdg_vegas_sample_device_polar): a group of 2 or 3
consecutive variables is a modulus and a direction -- ``K = MCIntegration.FermiK(dim, kF, 0.2 kF, 10 kF)`` of the reference's
example/benchmark.jl:46 -- and the sampler writes the Cartesian components; the accumulate calls and the refinement are the same.

Matsubara frequencies (``MatsubaraProjection``, the keyword ``matsubara``; fdg_mc_accumulate_device_matsubara): every root is multiplied
by the phase of its own pair of external times before it is summed -- ``phase(varT, ver4.Tpair[...])`` of the reference's
test/ver4.jl:193 -- so the estimate is complex, one number per frequency and root; the map is trained on the unprojected roots as before.

Weight groups (``WeightGroups``, ``groups_from_dof``, the keyword ``groups``; fdg_vegas_sample_device_grouped,
fdg_mc_accumulate_device_grouped): roots that integrate different numbers of variables in one run -- MCIntegration's ``dof``, as in the
reference's test/hubbard.jl:81-85 and example/strong_coupling_expansion/naive.jl:195 -- each weighted by the jacobian of its own
variables, each variable's map trained by the roots that use it.

Observables (``Observables``, the keyword ``observables``; fdg_mc_accumulate_device_observables): what a caller reports is a sum of
roots -- the direct and exchange components of the reference's test/ver4.jl:184-216, a series summed over its orders -- and its error
bar needs the covariance of the roots, which share their samples.  The accumulate call sums the combinations and their products on
the device; the results gain ``obs_mean``, ``obs_stderr``, ``obs_chi2_dof`` and ``obs_cov``.

Adaptive stratified sampling (``Stratification``, ``strat_for``, the keyword ``strat``; fdg_vegas_sample_device_strat,
fdg_mc_accumulate_device_strat, fdg_strat_allocate): Lepage's VEGAS+ on top of the map.  The unit cube of the map's coordinates is cut
into hypercubes, each receives at least two samples and the rest go where the integrand's standard deviation is largest -- what a
separable map cannot do for a ridge along a diagonal (a propagator of ``k1 + k2`` or ``T[i] - T[j]``).  Together with spherical
momentum variables and weight groups: ``vegas_integrate_stratified`` (fdg_vegas_sample_device_strat_grouped,
fdg_[mc_]accumulate_device_strat_grouped, fdg_strat_allocate_cols).

Markov-chain sampling (``chain_integrate``, ``chain_estimate``, ``ChainResult``; fdg_chain_propose_device, fdg_[mc_]chain_step_device,
fdg_chain_reduce_device): a Metropolis chain whose proposals are fresh draws through the map for a subset of the variables, one
walker per lane -- what ``integrate(...; solver=:mcmc)`` of the reference's test/hubbard.jl:85 asks MCIntegration for -- for weights
that no separable map follows.  The stationary density ``|s| + gamma q`` carries the map's own density ``q``, whose known integral
normalises the result; the error bar comes from the spread across the independent walkers.  With ``matsubara`` the projection
runs inside the chain (fdg_[mc_]chain_step_device_matsubara): the weight is the modulus of the projected sum at one frequency, and
every root is measured at every frequency.  With weight groups (``chain_integrate_grouped``; fdg_[mc_]chain_step_device_grouped)
several orders of a series walk in one chain: every group carries the jacobian of its own variables and a reweight factor.
With spherical momentum variables (``chain_integrate_polar``, ``chain_moves_polar``; fdg_chain_propose_device_polar) the proposal
draws a group's modulus and direction and writes the Cartesian columns; the measure's factors ride in the group's own rows of the
per-variable factors, so every step serves as it is.  A group is redrawn whole or not at all.
With local moves (``chain_integrate_shift``, ``ChainShift``, ``chain_moves_shift``; fdg_chain_propose_device_local) a variable is
displaced in the map's uniform coordinate, ``y' = y + t h (mod 1)``, instead of being redrawn whole: the stationary density in ``y`` is
``a + gamma``, so the step's rule is the Metropolis rule of every proposal symmetric in ``y``, and every step serves as it is.
With observables (``chain_integrate_observables``, ``chain_estimate_observables``, ``ChainObservablesResult``;
fdg_chain_reduce_device_observables) the chain reports sums of roots, or of projected roots per frequency, with their covariance
over the walkers: one reduction behind the chain forms the cross moments between the roots, which share their walkers.
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import capi
from .compilers import mc_covariance, mc_estimate


def uniform_grid(lo, hi, n_grid: int) -> np.ndarray:
    """The flat map: edges ``lo + (hi - lo) * i / G`` for ``i = 0 .. G`` per variable, the last edge exactly ``hi``; ``[n_dim, G + 1]``."""
    lo = np.atleast_1d(np.asarray(lo, dtype=np.float64))
    hi = np.atleast_1d(np.asarray(hi, dtype=np.float64))
    G = int(n_grid)
    if lo.shape != hi.shape or lo.ndim != 1 or not (1 <= lo.shape[0] <= capi.FDG_VEGAS_DIM_MAX):
        raise ValueError(f"lo and hi must be vectors of 1 .. {capi.FDG_VEGAS_DIM_MAX} limits")
    if not (1 <= G <= capi.FDG_VEGAS_GRID_MAX):
        raise ValueError(f"n_grid must lie in [1, {capi.FDG_VEGAS_GRID_MAX}]")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
        raise ValueError("every variable needs finite limits lo < hi")
    g = lo[:, None] + (hi - lo)[:, None] * np.arange(G + 1, dtype=np.float64)[None, :] / G
    g[:, G] = hi
    if not (np.diff(g, axis=1) > 0).all():
        raise ValueError("n_grid cells do not resolve [lo, hi] in float64")
    return np.ascontiguousarray(g)


class VegasMap:
    """A map on the host (``.grid``, float64 ``[n_dim, n_grid + 1]``) and its copy on ``device`` (``.d_grid``, what the sampler reads)."""

    def __init__(self, grid: np.ndarray, device):
        import torch
        g = np.ascontiguousarray(grid, dtype=np.float64)
        if g.ndim != 2 or not (1 <= g.shape[0] <= capi.FDG_VEGAS_DIM_MAX) or not (2 <= g.shape[1] <= capi.FDG_VEGAS_GRID_MAX + 1):
            raise ValueError("grid must be [n_dim, n_grid + 1] within the map's limits")
        if not (np.diff(g, axis=1) > 0).all():
            raise ValueError("the edges of every variable must be strictly increasing")
        self.grid = g.copy()
        self.device = torch.device(device)
        self.d_grid = torch.from_numpy(self.grid).to(self.device)

    @property
    def n_dim(self) -> int:
        return self.grid.shape[0]

    @property
    def n_grid(self) -> int:
        return self.grid.shape[1] - 1

    def refine(self, hist, alpha: float = 0.5) -> "VegasMap":
        """Moves the edges by the training histogram ``hist [n_dim, n_grid]`` (a CUDA tensor or a host array) through
        ``fdg_vegas_refine`` and uploads them; a failed refinement leaves both copies as they were."""
        h = hist.detach().cpu().numpy() if hasattr(hist, "detach") else np.asarray(hist, dtype=np.float64)
        capi.vegas_refine(self.grid, h, alpha)
        self.d_grid.copy_(self.d_grid.new_tensor(self.grid))
        return self


@dataclass
class VegasResult:
    mean: np.ndarray                 # [R] inverse-variance combination of the iterations kept
    stderr: np.ndarray               # [R]
    chi2_dof: np.ndarray             # [R] consistency of the iterations kept (nan with fewer than two)
    iterations: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # (mean [R], stderr [R]) of every iteration
    map: Optional[VegasMap] = None   # the map after the last refinement
    histograms: List[np.ndarray] = field(default_factory=list)                       # the training histogram of every iteration
    obs_mean: Optional[np.ndarray] = None       # with ``observables``: [n_obs] combination of the iterations kept, as ``mean``
    obs_stderr: Optional[np.ndarray] = None     # [n_obs]
    obs_chi2_dof: Optional[np.ndarray] = None   # [n_obs]
    obs_cov: Optional[np.ndarray] = None        # [n_obs, n_obs] covariance of ``obs_mean`` (:func:`combine_covariance`)
    obs_iterations: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # (mean [n_obs], C [n_obs, n_obs]) of every iteration
    cube_counts: List[np.ndarray] = field(default_factory=list)      # with ``strat``: the samples per hypercube [H] of every iteration
    fobs_mean: Optional[np.ndarray] = None      # with ``freq_observables``: complex [n_freq, M], as ``mean`` under ``matsubara``
    fobs_stderr: Optional[np.ndarray] = None    # complex [n_freq, M]: the real parts' figures in .real, the imaginary parts' in .imag
    fobs_chi2_dof: Optional[np.ndarray] = None  # complex [n_freq, M], likewise
    fobs_cov: Optional[np.ndarray] = None       # real [n_freq, 2 M, 2 M]: the components (Re o_0 .., Im o_0 ..) (:func:`combine_covariance`)
    fobs_iterations: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # (mean [n_freq, 2 M], C [n_freq, 2 M, 2 M])


def combine(iterations: Sequence[Tuple[np.ndarray, np.ndarray]]):
    """Inverse-variance combination per root of ``(mean, stderr)`` pairs: ``(mean, stderr, chi2 / dof)``.  A root whose error is 0 in
    some iteration (a constant, or a root that does not exist) is averaged plainly and reports chi2/dof = nan."""
    m = np.array([np.ravel(a) for a, _ in iterations], dtype=np.float64)
    e = np.array([np.ravel(b) for _, b in iterations], dtype=np.float64)
    n = m.shape[0]
    ok = (e > 0).all(axis=0)
    wgt = np.where(ok, 1.0 / np.where(e > 0, e, 1.0) ** 2, 1.0)
    mean = (wgt * m).sum(axis=0) / wgt.sum(axis=0)
    err = np.where(ok, 1.0 / np.sqrt(wgt.sum(axis=0)), 0.0)
    chi2 = np.where(ok, (wgt * (m - mean) ** 2).sum(axis=0) / max(n - 1, 1), np.nan) if n > 1 else np.full(m.shape[1], np.nan)
    return mean, err, chi2


def combine_covariance(iterations: Sequence[Tuple[np.ndarray, np.ndarray]]):
    """:func:`combine` for observables with a covariance: ``iterations`` holds ``(mean [..., M], C [..., M, M])`` pairs
    (``mc_covariance``).  Every observable is combined on its own by :func:`combine` with ``stderr = sqrt(diag(C))``; the covariance of
    the combined means is the exact propagation through those fixed weights, ``sum_i a[i, m] a[i, m'] C_i[m, m']`` with ``a[i, m]``
    the normalised weights ``combine`` used for observable ``m`` in iteration ``i``.  With inverse-variance weights its diagonal is
    ``stderr**2``; where ``combine`` averages plainly (an error of 0 in some iteration) the diagonal is the variance of that plain
    average while ``stderr`` reports 0.  Returns ``(mean, stderr, chi2 / dof, cov)``."""
    m = np.array([a for a, _ in iterations], dtype=np.float64)
    c = np.array([b for _, b in iterations], dtype=np.float64)
    shape = m.shape[1:]
    M = shape[-1]
    e = np.sqrt(np.maximum(np.diagonal(c, axis1=-2, axis2=-1), 0.0))
    mean, err, chi2 = combine([(a.reshape(-1), b.reshape(-1)) for a, b in zip(m, e)])
    ok = (e > 0).all(axis=0)
    wgt = np.where(ok, 1.0 / np.where(e > 0, e, 1.0) ** 2, 1.0)
    a = wgt / wgt.sum(axis=0)
    cov = (a[..., :, None] * a[..., None, :] * c).sum(axis=0)
    return mean.reshape(shape), err.reshape(shape), chi2.reshape(shape), cov.reshape(shape + (M,))


@dataclass(frozen=True)
class PolarVar:
    """A group of polar variables: the VEGAS variables ``var, var + 1`` are ``(k, phi)`` when ``cols`` names two columns, and
    ``var, var + 1, var + 2`` are ``(k, theta, phi)`` when it names three; the sampler writes ``k cos(phi)``, ``k sin(phi)`` or
    ``k sin(theta) cos(phi)``, ``k sin(theta) sin(phi)``, ``k cos(theta)`` into the columns ``cols`` and multiplies the weight by
    ``k`` or ``k**2 sin(theta)``."""
    var: int
    cols: Tuple[int, ...]


def ball(k_max: float, dim: int = 3, k_min: float = 0.0):
    """``(lo, hi)`` of one group's variables for the ball (``k_min > 0``: the shell) ``k_min <= |K| <= k_max`` in ``dim`` = 2 or 3
    dimensions: ``k`` in ``[k_min, k_max]``, ``theta`` in ``[0, pi]`` (3D only), ``phi`` in ``[0, 2 pi]``."""
    if dim not in (2, 3):
        raise ValueError("dim must be 2 or 3")
    if not (0.0 <= k_min < k_max and math.isfinite(k_max)):
        raise ValueError("need 0 <= k_min < k_max, finite")
    angles = [math.pi, 2.0 * math.pi] if dim == 3 else [2.0 * math.pi]
    return [float(k_min)] + [0.0] * (dim - 1), [float(k_max)] + angles


def _check_polar(polar, col, vmap, n_col):
    """The groups as ``(var, cols)`` pairs, after the checks of the driver: every group inside the map and apart from the others, no
    column on a grouped variable, every column inside x, and the edges of the map within the domain of the sampler's sine and cosine."""
    groups, grouped = [], set()
    for p in polar:
        var, cols = int(p.var), tuple(int(c) for c in p.cols)
        if len(cols) not in (2, 3):
            raise ValueError("a polar group names 2 or 3 columns")
        mine = set(range(var, var + len(cols)))
        if var < 0 or var + len(cols) > vmap.n_dim:
            raise ValueError("a polar group reaches outside the map's variables")
        if mine & grouped:
            raise ValueError("two polar groups share a variable")
        grouped |= mine
        if not all(0 <= c < n_col for c in cols):
            raise ValueError(f"a polar group must name columns in [0, {n_col})")
        if any(col[d] is not None for d in mine):
            raise ValueError("the col entry of a grouped variable must be None: the group writes its own columns")
        g = vmap.grid
        angles = [(var + 1, math.pi, "theta"), (var + 2, 2.0 * math.pi, "phi")] if len(cols) == 3 else [(var + 1, 2.0 * math.pi, "phi")]
        if not g[var, 0] >= 0.0:
            raise ValueError("the modulus of a polar group needs lo >= 0")
        for d, top, what in angles:
            if not (g[d, 0] >= 0.0 and g[d, -1] <= top):
                raise ValueError(f"{what} of a polar group must stay within [0, {top}]")
        groups.append((var, cols))
    if len(groups) > capi.FDG_VEGAS_POLAR_MAX:
        raise ValueError(f"at most {capi.FDG_VEGAS_POLAR_MAX} polar groups")
    return groups


# ---- the set-up the drivers share: each helper is called where its checks stand in that driver's sequence of refusals ---------------- #
def _columns(func_or_handle, tables, col, polar, none_ok: bool):
    """``(handle, n_col_k, n_col, col, written)``: the columns of ``x`` -- ``n_col_k`` momentum components, then the times; with
    ``tables`` None (the leaf form) the graph's leaves --, ``col`` as ints (None kept where ``none_ok``: a grouped variable's entry)
    and the columns the sampler writes, which must be distinct and inside ``x``."""
    handle = getattr(func_or_handle, "handle", func_or_handle)
    if tables is None:
        n_col_k, n_col = 0, handle.table.n_leaf
    else:
        n_col_k = int(tables.n_loop) * int(tables.dim)
        n_col = n_col_k + int(tables.n_tau)
    col = [None if (c is None and none_ok) else int(c) for c in col]
    written = [c for c in col if c is not None] + [int(c) for p in (polar or ()) for c in p.cols]
    if len(set(written)) != len(written) or not all(0 <= c < n_col for c in written):
        raise ValueError(f"col must name distinct columns in [0, {n_col})")
    return handle, n_col_k, n_col, col, written


def _check_ext_col(dmap, n_col: int, written, that_col: str):
    """The discrete variable's columns lie inside ``x`` and apart from the sampler's; ``that_col``: the driver's own end of the message."""
    if not all(0 <= e < n_col for e in dmap.ext_col) or set(dmap.ext_col) & set(written):
        raise ValueError(f"dmap.ext_col must name columns in [0, {n_col}) {that_col}")


def _map_for(vmap, lo, hi, n_grid, device, col) -> "VegasMap":
    """``vmap``, or the flat map over ``[lo, hi]``; one variable per entry of ``col``."""
    if vmap is None:
        vmap = VegasMap(uniform_grid(lo, hi, n_grid), device)
    if vmap.n_dim != len(col):
        raise ValueError("one column per variable of the map")
    return vmap


def _polar_groups(polar, col, vmap, n_col):
    """:func:`_check_polar`, and no variable outside the groups without a column."""
    groups = _check_polar(polar, col, vmap, n_col)
    if any(c is None for d, c in enumerate(col) if not any(v <= d < v + len(cs) for v, cs in groups)):
        raise ValueError("only the variables of a polar group go without a column")
    return groups


def _check_weight_groups(wgroups, R: int, D: int, pgroups, limit: bool = True) -> int:
    """The checks of a :class:`WeightGroups` against ``R`` roots, ``D`` variables and the polar groups; returns the number of groups.
    ``limit`` False leaves FDG_WEIGHT_GROUP_MAX to the library (``vegas_integrate``, which never checked it on this side)."""
    NG = len(wgroups.var_sets)
    if len(wgroups.root_group) != R or not all(0 <= int(v) < NG for v in wgroups.root_group):
        raise ValueError("groups.root_group names one group of groups.var_sets per root")
    if limit and not 1 <= NG <= capi.FDG_WEIGHT_GROUP_MAX:
        raise ValueError(f"need 1 .. {capi.FDG_WEIGHT_GROUP_MAX} weight groups")
    if not all(0 <= int(d) < D for vs in wgroups.var_sets for d in vs):
        raise ValueError("groups.var_sets names variables of the map")
    for var, cs in pgroups or ():
        if any(0 < len(set(int(d) for d in vs) & set(range(var, var + len(cs)))) < len(cs) for vs in wgroups.var_sets):
            raise ValueError("a polar group belongs to a weight group whole or not at all")
    return NG


def _fixed(fixed, n_col: int) -> np.ndarray:
    fx = np.zeros(n_col) if fixed is None else np.asarray(fixed, dtype=np.float64)
    if fx.shape != (n_col,):
        raise ValueError(f"fixed must hold {n_col} column values")
    return fx


def _state(fx, B: int, device):
    """``x [n_col, B]`` on the device, sample stride 1: every column at its fixed value."""
    import torch
    return torch.from_numpy(fx).to(device)[:, None].repeat(1, B).contiguous()


class _Discrete(NamedTuple):
    """The discrete variable's arguments of the samplers, proposals and steps.  The defaults are what those calls take without one."""
    d_cdf: int = 0
    n_bin: int = 0
    bin_base: int = 0
    d_ext: int = 0
    ext_col: Optional[Sequence[int]] = None
    d_bin: int = 0
    d_binp: int = 0


def _discrete(dmap, none_bins: int, bins=None, binp=None) -> _Discrete:
    """The pack of ``dmap`` with the walkers' or samples' values in ``bins`` (and the proposals' in ``binp``); ``dmap`` None: the
    defaults with ``n_bin = none_bins`` (the direct sampler counts one bin then, the chain none)."""
    if dmap is None:
        return _Discrete(n_bin=none_bins)
    return _Discrete(dmap.d_cdf.data_ptr(), dmap.n_bin, 0, 0 if dmap.d_ext is None else dmap.d_ext.data_ptr(), dmap.ext_col,
                     bins.data_ptr(), 0 if binp is None else binp.data_ptr())


@dataclass(frozen=True)
class MatsubaraProjection:
    """The frequencies an integration projects its roots onto: ``freq`` the integers ``n`` of ``omega_n = (2n+1) pi / beta``
    (``fermionic``) or ``2n pi / beta``, ``root_tau_in`` / ``root_tau_out`` the 1-based labels of every root's pair of external times
    (``workloads.root_times``).  Root ``k`` enters as ``root_k * e^{+i omega_n (T[tau_out] - T[tau_in])}``
    (``capi.matsubara_phase``); for the other sign pass ``-n`` (fermions: ``-n - 1``)."""
    freq: Tuple[int, ...]
    fermionic: bool
    root_tau_in: Tuple[int, ...]
    root_tau_out: Tuple[int, ...]


@dataclass(frozen=True)
class WeightGroups:
    """Roots with their own integration variables: root ``k`` belongs to group ``root_group[k]``, and group ``g`` integrates the VEGAS
    variables ``var_sets[g]`` -- its roots are weighted by the jacobian of those variables only, and only they train those variables'
    maps.  A polar group of variables belongs to a set whole or not at all."""
    root_group: Tuple[int, ...]
    var_sets: Tuple[Tuple[int, ...], ...]


@dataclass(frozen=True)
class Observables:
    """Linear combinations of the roots that an integration reports: ``coef[m][k]`` the factor of root ``k`` in observable ``m``, at
    most ``capi.FDG_OBS_MAX`` rows of ``n_root`` finite numbers.  Every root enters with its own weight (its group's jacobian under
    ``groups``), unprojected; the complex observables of Matsubara-projected roots are :class:`FrequencyObservables`."""
    coef: Tuple[Tuple[float, ...], ...]


@dataclass(frozen=True)
class FrequencyObservables:
    """Linear combinations of the PROJECTED roots that an integration reports per frequency: ``coef[m][k]`` the real factor of root
    ``k`` in observable ``m``, at most ``capi.FDG_FREQ_OBS_MAX`` rows of ``n_root`` finite numbers.  Every root enters with its own
    weight (its group's jacobian under ``groups``) and the phase of its own pair of times (``matsubara``, which it needs)."""
    coef: Tuple[Tuple[float, ...], ...]


def complex_components(x) -> np.ndarray:
    """The complex ``[..., M]`` array of ``[..., 2 M]`` real components ``(Re_0 .. Re_{M-1}, Im_0 .. Im_{M-1})``: what the frequency
    observables' means, error bars and chi2/dof are reported as (the figures of the real parts in the real part)."""
    x = np.asarray(x, dtype=np.float64)
    M = x.shape[-1] // 2
    out = np.empty(x.shape[:-1] + (M,), dtype=np.complex128)
    out.real, out.imag = x[..., :M], x[..., M:]           # (not re + 1j * im: a nan of one part would spread to the other)
    return out


@dataclass(frozen=True)
class Stratification:
    """Adaptive stratified sampling on top of the map: ``strat[d]`` strata of variable ``d`` (:func:`strat_for`), ``H = prod strat``
    hypercubes of at most ``capi.FDG_STRAT_CUBE_MAX``; ``beta`` in ``[0, 1]`` damps the reallocation (0: every iteration uniform)."""
    strat: Tuple[int, ...]
    beta: float = 0.75


def strat_for(n_sample: int, n_dim: int, max_cubes: int = capi.FDG_STRAT_CUBE_MAX) -> Tuple[int, ...]:
    """Lepage's rule for the strata per variable: ``floor((n_sample / 4) ** (1 / n_dim))`` on every axis (at least 1; the root taken
    in integers), then, while there are more than ``max_cubes`` hypercubes, one stratum less on one axis at a time, from the last
    axis to the first and round again."""
    n, D = int(n_sample), int(n_dim)
    if n < 1 or D < 1 or max_cubes < 1:
        raise ValueError("need n_sample, n_dim and max_cubes >= 1")
    s = max(1, int((n / 4.0) ** (1.0 / D)))
    while 4 * (s + 1) ** D <= n:
        s += 1
    while s > 1 and 4 * s ** D > n:
        s -= 1
    out = [s] * D
    while math.prod(out) > max_cubes:
        for d in range(D - 1, -1, -1):
            if out[d] > 1 and math.prod(out) > max_cubes:
                out[d] -= 1
    return tuple(out)


def strat_variance(cube_sum, cube_sum2, counts, n_total: int) -> np.ndarray:
    """The variance of the stratified estimate per column of the per-hypercube moments ``[H, C]``:
    ``sum_h n_h var_h / N**2`` with ``var_h = max(0, (sum2_h - sum_h**2 / n_h) / (n_h - 1))``."""
    n = np.asarray(counts, dtype=np.float64)[:, None]
    var = np.maximum(0.0, (cube_sum2 - cube_sum * cube_sum / n) / (n - 1.0))
    return (n * var).sum(axis=0) / float(n_total) ** 2


def _iteration_seed(seed: int, it: int) -> int:
    """The Philox key of iteration ``it`` of a stratified run.  A sample's index places it in its hypercube, so the iterations cannot
    be told apart by ``sample_offset`` as in the plain driver: each takes a key of its own."""
    return (int(seed) + it * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def _integrate_strat(func_or_handle, tables, lo, hi, col, kF, beta, lam, *, n_iter, n_sample, n_grid, alpha, seed, n_discard, fixed, coef,
                     device, vmap, specialize_fused, n_total, shard_start, reduce, strat, polar=None, wgroups=None, alloc_cols=None):
    """:func:`vegas_integrate` with ``strat`` and :func:`vegas_integrate_stratified`.  Per iteration: allocate, sample, accumulate,
    refine the map, fdg_strat_allocate_cols.  Without ``polar`` and ``wgroups`` the device calls are the plain stratified ones."""
    import torch
    from .nodetable import FDG_NO_ROOT
    device = torch.device(device)
    handle, n_col_k, n_col, col, _ = _columns(func_or_handle, tables, col, polar, bool(polar))
    R = handle.table.n_root
    vmap = _map_for(vmap, lo, hi, n_grid, device, col)
    groups = _polar_groups(polar, col, vmap, n_col) if polar else None
    D, G = vmap.n_dim, vmap.n_grid
    NG = 1 if wgroups is None else _check_weight_groups(wgroups, R, D, groups)      # the columns behind the roots' in the per-hypercube moments
    sv = tuple(int(v) for v in strat.strat)
    if len(sv) != D or not all(v >= 1 for v in sv):
        raise ValueError("strat.strat holds one count >= 1 per variable of the map")
    H = math.prod(sv)
    B = int(n_sample)
    N = B if n_total is None else int(n_total)
    if not 0.0 <= strat.beta <= 1.0:
        raise ValueError("strat.beta must lie in [0, 1]")
    if H > capi.FDG_STRAT_CUBE_MAX or H * (R + NG) > 1 << 24 or N < 2 * H:
        raise ValueError(f"need at most {capi.FDG_STRAT_CUBE_MAX} hypercubes, H * (n_root + {'n_group' if wgroups is not None else '1'}) "
                         f"<= 2**24 and n_total >= 2 H")
    if B < 1 or n_iter < 1 or not (0 <= n_discard < n_iter) or not 0 <= int(shard_start) <= N - B:
        raise ValueError("need n_sample >= 1, 0 <= n_discard < n_iter and the shard inside n_total")
    if alloc_cols is None:
        # every column behind the roots' that has a root that exists behind it (without groups: the coef column)
        rs = np.asarray(handle.table.root_slot)
        have = {0 if wgroups is None else int(wgroups.root_group[k]) for k in range(R) if int(rs[k]) != FDG_NO_ROOT}
        alloc_cols = [R + g for g in range(NG) if g in have] or [R]
    alloc_cols = [int(c) for c in alloc_cols]
    if not alloc_cols or not all(0 <= c < R + NG for c in alloc_cols):
        raise ValueError(f"alloc_cols names at least one column in [0, {R + NG}) of the per-hypercube moments")
    if specialize_fused and tables is not None:
        handle.specialize_fused(tables)
    fx = _fixed(fixed, n_col)
    out = VegasResult(np.zeros(R), np.zeros(R), np.full(R, np.nan), map=vmap)
    start = capi.strat_allocate_cols(None, None, alloc_cols, None, H, N, strat.beta)
    with torch.cuda.device(device):
        st = torch.cuda.current_stream(device).cuda_stream
        x = _state(fx, B, device)
        src = (x.data_ptr(), 1, B, 0) if tables is None else (x.data_ptr(), 1, B, x.data_ptr() + 8 * n_col_k * B, 1, B, kF, beta, lam)
        jac = torch.empty(B if wgroups is None else (NG, B), dtype=torch.float64, device=device)
        cube = torch.empty(B, dtype=torch.int32, device=device)
        wdesc = None
        if wgroups is not None:
            wdesc, _wkeep = capi.make_weight_groups(wgroups.root_group, wgroups.var_sets, B)
        for it in range(int(n_iter)):
            key, off = _iteration_seed(seed, it), int(shard_start)
            d_start = torch.from_numpy(start).to(device)
            m = torch.zeros((2, 1, R), dtype=torch.float64, device=device)
            hist = torch.zeros((D, G), dtype=torch.float64, device=device)
            cs = torch.zeros((2, H, R + NG), dtype=torch.float64, device=device)
            if groups or wgroups is not None:
                capi.vegas_sample_device_strat_grouped(vmap.d_grid.data_ptr(), D, G, col, groups, None if wgroups is None else wgroups.var_sets,
                                                       B, sv, d_start.data_ptr(), key, off, x.data_ptr(), 1, B, jac.data_ptr(),
                                                       cube.data_ptr(), 0, B, st)
            else:
                capi.vegas_sample_device_strat(vmap.d_grid.data_ptr(), D, G, col, sv, d_start.data_ptr(), key, off, x.data_ptr(), 1, B,
                                               jac.data_ptr(), cube.data_ptr(), 0, B, st)
            handle._accumulate("strat" if wgroups is None else "strat_grouped", src, jac.data_ptr(), handle._coef(coef), key, off, D, G,
                               m[0].data_ptr(), m[1].data_ptr(), hist.data_ptr(), capi._strat_array(sv, D), cube.data_ptr(),
                               cs[0].data_ptr(), cs[1].data_ptr(), *(() if wgroups is None else (wdesc,)), B, st)
            if reduce is not None:
                for t in (m, hist, cs):
                    reduce(t)
            h_cs, counts = cs.cpu().numpy(), np.diff(start)
            mean = m[0, 0].cpu().numpy() / N
            err = np.sqrt(strat_variance(h_cs[0][:, :R], h_cs[1][:, :R], counts, N))
            out.iterations.append((mean, err))
            out.histograms.append(hist.cpu().numpy())
            out.cube_counts.append(counts)
            vmap.refine(out.histograms[-1], alpha)
            start = capi.strat_allocate_cols(h_cs[0], h_cs[1], alloc_cols, start, H, N, strat.beta)
    out.mean, out.stderr, out.chi2_dof = combine(out.iterations[int(n_discard):])
    return out


def vegas_integrate_stratified(func_or_handle, tables, lo, hi, col, strat: Stratification, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0,
                               *, n_iter: int = 10, n_sample: int = 100_000, n_grid: int = 64, alpha: float = 0.5, seed: int = 0,
                               n_discard: int = 0, fixed=None, coef=None, device="cuda", vmap: Optional[VegasMap] = None,
                               specialize_fused: bool = True, n_total: Optional[int] = None, shard_start: int = 0,
                               reduce: Optional[Callable] = None, polar: Optional[Sequence[PolarVar]] = None,
                               groups: Optional[WeightGroups] = None, alloc_cols: Optional[Sequence[int]] = None) -> VegasResult:
    """Adaptive stratified sampling (:class:`Stratification`) together with spherical momentum variables (``polar``) and weight
    groups (``groups``), which :func:`vegas_integrate` refuses beside ``strat``.  The arguments and the result are those of
    ``vegas_integrate(..., strat=strat)``; ``tables`` None is the leaf form.

    Per iteration: sample through fdg_vegas_sample_device_strat_grouped by the current allocation (the first is uniform) -- the
    strata cut the map's own coordinates, a polar group's ``(k, theta, phi)`` --, accumulate through
    fdg_[mc_]accumulate_device_strat_grouped (with ``polar`` alone: the _strat call on the one jacobian), ``reduce`` on the moments,
    the histogram and the per-hypercube moments ``[2, H, n_root + n_group]``, refine the map, fdg_strat_allocate_cols.  Every group's
    weight carries the hypercube's ``n_total / (H n_h)``, also that of a group which does not own every variable.  ``mean`` and
    ``stderr`` come per root from :func:`strat_variance` on the roots' columns; iteration ``it`` draws with the Philox key of
    ``vegas_integrate``'s stratified run.

    ``alloc_cols``: the columns of the per-hypercube moments whose variances, added up, steer the next allocation; by default the
    groups' columns ``n_root + g`` of every group with a root that exists (without ``groups``: column ``n_root``, the ``coef``
    combination).  With ``polar`` and ``groups`` None the device calls and the result are ``vegas_integrate(strat=...)``'s, bit for
    bit."""
    if strat is None:
        raise ValueError("vegas_integrate_stratified needs a Stratification")
    return _integrate_strat(func_or_handle, tables, lo, hi, col, kF, beta, lam, n_iter=n_iter, n_sample=n_sample, n_grid=n_grid, alpha=alpha,
                            seed=seed, n_discard=n_discard, fixed=fixed, coef=coef, device=device, vmap=vmap,
                            specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start, reduce=reduce, strat=strat,
                            polar=polar, wgroups=groups, alloc_cols=alloc_cols)


def groups_from_dof(dof, pools) -> WeightGroups:
    """:class:`WeightGroups` in MCIntegration's call shape.  ``pools[p]`` lists, in order, the VEGAS variables of each element of
    variable pool ``p`` (one ``K`` of a polar group: its three variables; one time: one variable); ``dof[i][p]`` says how many leading
    elements of pool ``p`` root ``i`` integrates.  Roots with equal sets of variables share a group; the groups are numbered in the
    order their first root appears."""
    sets, root_group = [], []
    for i, row in enumerate(dof):
        if len(row) != len(pools):
            raise ValueError(f"dof[{i}] must hold one count per pool")
        mine = []
        for n, pool in zip(row, pools):
            if not 0 <= int(n) <= len(pool):
                raise ValueError(f"dof[{i}] asks for {n} elements of a pool of {len(pool)}")
            mine += [int(d) for element in pool[:int(n)] for d in element]
        key = tuple(sorted(set(mine)))
        if key not in sets:
            sets.append(key)
        root_group.append(sets.index(key))
    if not 1 <= len(sets) <= capi.FDG_WEIGHT_GROUP_MAX:
        raise ValueError(f"need 1 .. {capi.FDG_WEIGHT_GROUP_MAX} distinct sets of variables")
    return WeightGroups(tuple(root_group), tuple(sets))


def _coef_table(table, what: str, R: int, limit: int) -> np.ndarray:
    """``table.coef`` (``what``: ``observables`` or ``freq_observables``) as float64 ``[n_obs, R]``: finite, ``1 <= n_obs <= limit``."""
    try:
        c = np.ascontiguousarray(table.coef, dtype=np.float64)
    except (TypeError, ValueError):                          # (rows of unequal lengths)
        c = np.zeros(0)
    if c.ndim != 2 or c.shape[1] != R or not (1 <= c.shape[0] <= limit) or not np.isfinite(c).all():
        raise ValueError(f"{what}.coef must be [n_obs, n_root = {R}], finite, with 1 <= n_obs <= {limit}")
    return c


def _integrate(func_or_handle, tables, lo, hi, col, kF, beta, lam, *, dmap, n_iter, n_sample, n_grid, alpha, floor, seed, n_discard, fixed, coef,
               device, vmap, specialize_fused, n_total, shard_start, reduce, polar=None, matsubara=None, wgroups=None, observables=None,
               freq_observables=None):
    """The driver behind :func:`vegas_integrate` (``dmap`` None: results ``[R]``) and :func:`vegas_integrate_binned` (``[n_bin, R]``);
    with ``matsubara`` the results are complex and carry a frequency axis in front of the roots."""
    if freq_observables is not None and matsubara is None:
        raise ValueError("freq_observables needs matsubara: the frequencies and the roots' time labels")
    import torch
    device = torch.device(device)
    n_tau = int(tables.n_tau)                              # (tables is required: this driver has no leaf form)
    handle, n_col_k, n_col, col, written = _columns(func_or_handle, tables, col, polar, bool(polar))
    R = handle.table.n_root
    if dmap is not None:
        _check_ext_col(dmap, n_col, written, "that col does not")
        if dmap.device != device:
            raise ValueError("dmap lives on another device")
    vmap = _map_for(vmap, lo, hi, n_grid, device, col)
    groups = _polar_groups(polar, col, vmap, n_col) if polar else None
    D, G, NB = vmap.n_dim, vmap.n_grid, 1 if dmap is None else dmap.n_bin
    if wgroups is not None:
        _check_weight_groups(wgroups, R, D, groups, limit=False)
    ocoef = None if observables is None else _coef_table(observables, "observables", R, capi.FDG_OBS_MAX)
    fcoef = None if freq_observables is None else _coef_table(freq_observables, "freq_observables", R, capi.FDG_FREQ_OBS_MAX)
    B = int(n_sample)
    N = B if n_total is None else int(n_total)
    if B < 1 or N < 2 or n_iter < 1 or not (0 <= n_discard < n_iter):
        raise ValueError("need n_sample >= 1, n_total >= 2 and 0 <= n_discard < n_iter")
    if specialize_fused:
        handle.specialize_fused(tables)
    fx = _fixed(fixed, n_col)
    shape = (R,) if dmap is None else (NB, R)
    if matsubara is not None:
        NF = len(matsubara.freq)
        if not (1 <= NF <= capi.FDG_MATSUBARA_FREQ_MAX and NB * NF <= capi.FDG_BIN_MAX):
            raise ValueError(f"need 1 .. {capi.FDG_MATSUBARA_FREQ_MAX} frequencies and n_bin * n_freq <= {capi.FDG_BIN_MAX}")
        if len(matsubara.root_tau_in) != R or len(matsubara.root_tau_out) != R:
            raise ValueError("matsubara.root_tau_in and root_tau_out hold one label per root")
        shape = shape[:-1] + (NF, R)
    if dmap is None:
        out = VegasResult(np.zeros(shape), np.zeros(shape), np.full(shape, np.nan), map=vmap)
    else:
        out = VegasBinnedResult(np.zeros(shape), np.zeros(shape), np.full(shape, np.nan), map=vmap, dmap=dmap)
    with torch.cuda.device(device):
        st = torch.cuda.current_stream(device).cuda_stream
        x = _state(fx, B, device)
        jac = torch.empty(B if wgroups is None else (len(wgroups.var_sets), B), dtype=torch.float64, device=device)
        wdesc = None
        if wgroups is not None:
            wdesc, _wkeep = capi.make_weight_groups(wgroups.root_group, wgroups.var_sets, B)
        src = (x.data_ptr(), 1, B, x.data_ptr() + 8 * n_col_k * B, 1, B, kF, beta, lam)
        bins = None if dmap is None else torch.empty(B, dtype=torch.int32, device=device)
        dv = _discrete(dmap, 1, bins)
        f64 = dict(dtype=torch.float64, device=device)
        for it in range(int(n_iter)):
            off = it * N + int(shard_start)
            # the moments, or (re, im, re^2, im^2) of the projected roots; the training histograms are the same with and without a projection
            m = torch.zeros((2, NB, R) if matsubara is None else (4, NB, NF, R), **f64)
            hist = torch.zeros((D, G), **f64)
            hist_bin = None if dmap is None else torch.zeros(NB, **f64)
            sample = (seed, off, x.data_ptr(), 1, B, jac.data_ptr(), dv.d_bin, 0, B, st)
            if wgroups is not None:
                capi.vegas_sample_device_grouped(vmap.d_grid.data_ptr(), D, G, col, dv.d_cdf, dv.n_bin, dv.bin_base, dv.d_ext, dv.ext_col, groups,
                                                 wgroups.var_sets, B, *sample)
            elif groups:
                capi.vegas_sample_device_polar(vmap.d_grid.data_ptr(), D, G, col, dv.d_cdf, dv.n_bin, dv.bin_base, dv.d_ext, dv.ext_col, groups,
                                               *sample)
            elif dmap is None:
                capi.vegas_sample_device(vmap.d_grid.data_ptr(), D, G, col, seed, off, x.data_ptr(), 1, B, jac.data_ptr(), 0, B, st)
            else:
                capi.vegas_sample_device_discrete(vmap.d_grid.data_ptr(), D, G, col, dv.d_cdf, dv.n_bin, dv.bin_base, dv.d_ext, dv.ext_col, *sample)
            desc = odesc = fdesc = None
            osums, fsums = [], []
            if matsubara is not None:
                desc, _keep = capi.make_matsubara(matsubara.freq, matsubara.fermionic, matsubara.root_tau_in, matsubara.root_tau_out, beta,
                                                  n_tau, *[m[i].data_ptr() for i in range(4)])
            if ocoef is not None:
                M = ocoef.shape[0]
                osums = [torch.zeros((NB, M), **f64), torch.zeros((NB, M, M), **f64)]
                odesc, _okeep = capi.make_observables(ocoef, osums[0].data_ptr(), osums[1].data_ptr())
            if fcoef is not None:
                P = 2 * fcoef.shape[0]
                fsums = [torch.zeros((NB, NF, P), **f64), torch.zeros((NB, NF, P, P), **f64)]
                fdesc, _fkeep = capi.make_freq_observables(fcoef, fsums[0].data_ptr(), fsums[1].data_ptr())
            # the narrowest entry that carries what was asked for.  Each of these takes the blocks of the ones below it, every one
            # optional in it (a null descriptor, d_bin 0), and leaves their bits as they are; with a projection the unprojected
            # moments are not taken (d_acc, d_acc2 0)
            if fcoef is not None:
                entry, descs = "freq_observables", (desc, wdesc, odesc, fdesc)
            elif ocoef is not None:
                entry, descs = "observables", (desc, wdesc, odesc)
            elif wgroups is not None:
                entry, descs = "grouped", (desc, wdesc)
            elif matsubara is not None:
                entry, descs = "matsubara", (desc,)
            else:
                entry, descs = "vegas" if dmap is None else "vegas_binned", ()
            head = (dv.d_bin, dv.bin_base, NB, jac.data_ptr())
            block = (handle._coef(coef), seed, off, D, G, 0 if matsubara is not None else m[0].data_ptr(),
                     0 if matsubara is not None else m[1].data_ptr(), hist.data_ptr(), 0 if dmap is None else hist_bin.data_ptr())
            if entry == "vegas":                             # the one entry without the discrete variable's arguments
                head, block = head[3:], block[:-1]
            handle._accumulate(entry, src, *head, *block, *descs, B, st)
            sums = [m, hist] if dmap is None else [m, hist, hist_bin]
            if reduce is not None:
                for t in sums + osums + fsums:
                    reduce(t)
            if osums:
                om, oc = mc_covariance(osums[0], osums[1], N)
                oshape = shape[:-1 if matsubara is None else -2] + (ocoef.shape[0],)
                out.obs_iterations.append((om.cpu().numpy().reshape(oshape), oc.cpu().numpy().reshape(oshape + oshape[-1:])))
            if fsums:
                fm, fc = mc_covariance(fsums[0], fsums[1], N)
                fshape = shape[:-1] + (2 * fcoef.shape[0],)
                out.fobs_iterations.append((fm.cpu().numpy().reshape(fshape), fc.cpu().numpy().reshape(fshape + fshape[-1:])))
            if matsubara is not None:
                (mr, er), (mi, ei) = mc_estimate(m[0], m[2], N), mc_estimate(m[1], m[3], N)
                mean, err = torch.complex(mr, mi), torch.complex(er, ei)
            else:
                mean, err = mc_estimate(m[0], m[1], N)
            out.iterations.append((mean.cpu().numpy().reshape(shape), err.cpu().numpy().reshape(shape)))
            hs = [t.cpu().numpy() for t in sums[1:]]
            out.histograms.append(hs[0])
            if dmap is not None:
                out.bin_histograms.append(hs[1])
            vmap.refine(hs[0], alpha)
            if dmap is not None:
                dmap.refine(hs[1], alpha, floor)
    kept = out.iterations[int(n_discard):]
    if matsubara is not None:                 # the real and the imaginary parts are two estimates: combined each on its own
        re = combine([(a.real, b.real) for a, b in kept])
        im = combine([(a.imag, b.imag) for a, b in kept])
        mean, err, chi2 = (r + 1j * i for r, i in zip(re, im))
    else:
        mean, err, chi2 = combine(kept)
    out.mean, out.stderr, out.chi2_dof = mean.reshape(shape), err.reshape(shape), chi2.reshape(shape)
    if ocoef is not None:
        out.obs_mean, out.obs_stderr, out.obs_chi2_dof, out.obs_cov = combine_covariance(out.obs_iterations[int(n_discard):])
    if fcoef is not None:
        fmean, ferr, fchi2, out.fobs_cov = combine_covariance(out.fobs_iterations[int(n_discard):])
        out.fobs_mean, out.fobs_stderr, out.fobs_chi2_dof = (complex_components(v) for v in (fmean, ferr, fchi2))
    return out


def vegas_integrate(func_or_handle, tables, lo, hi, col, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *, n_iter: int = 10,
                    n_sample: int = 100_000, n_grid: int = 64, alpha: float = 0.5, seed: int = 0, n_discard: int = 0, fixed=None,
                    coef=None, device="cuda", vmap: Optional[VegasMap] = None, specialize_fused: bool = True, n_total: Optional[int] = None,
                    shard_start: int = 0, reduce: Optional[Callable] = None, polar: Optional[Sequence[PolarVar]] = None,
                    matsubara: Optional[MatsubaraProjection] = None, groups: Optional[WeightGroups] = None,
                    observables: Optional[Observables] = None, strat: Optional[Stratification] = None,
                    freq_observables: Optional[FrequencyObservables] = None) -> VegasResult:
    """Integrates the roots of a graph over the box ``[lo, hi]`` of ``len(col)`` of its Monte-Carlo variables.

    ``func_or_handle``: a ``GraphFunc`` or ``capi.GraphHandle``; ``tables`` the ``fdg_leaf_tables`` struct of ``capi.make_leaf_tables``
    (passed to ``specialize_fused`` unless ``specialize_fused=False``).  The variables live in one component-major array of
    ``n_loop * dim + n_tau`` columns -- the momentum components, then the times -- and ``col[d]`` names the column variable ``d``
    integrates; the other columns keep ``fixed`` (a vector of that many values, zeros by default: external momenta, ``T[1] = 0``).
    Per iteration ``it``: sample with ``sample_offset = it * n_total + shard_start``, accumulate with weight = the map's jacobian,
    ``mc_estimate``, refine with ``alpha``.  Iterations ``>= n_discard`` enter the inverse-variance combination.

    Sharding: every rank passes its ``shard_range`` start and count as ``shard_start`` / ``n_sample``, the whole iteration as
    ``n_total``, and ``reduce`` = a function that sums a CUDA tensor over the ranks in place (``sharding.reduce_observable``); it is
    applied to the ``[2, 1, R]`` moments and to the histogram, so every rank refines the same map.

    ``polar``: a sequence of :class:`PolarVar`.  The variables of a group are a modulus and a direction (``lo`` / ``hi`` rows as
    :func:`ball` gives them), their ``col`` entries are None, and the group's own ``cols`` take the Cartesian components; the weight
    carries ``k`` or ``k**2 sin(theta)``.  The limits (of ``lo`` / ``hi`` or of a ``vmap`` passed in) must keep ``k >= 0``, ``theta``
    within ``[0, math.pi]`` and ``phi`` within ``[0, 2 * math.pi]``.  None or empty: the box, with the bits it always had.

    ``matsubara``: a :class:`MatsubaraProjection`.  Every root is multiplied by the phase of its own pair of times at every frequency
    before it is summed: ``mean`` is complex ``[n_freq, R]``, ``stderr`` and ``chi2_dof`` carry the figures of the real parts in their
    real parts and those of the imaginary parts in their imaginary parts (``mc_estimate`` and ``combine`` on each), and ``reduce`` is
    applied to the ``[4, 1, n_freq, R]`` sums.  The map is trained on the unprojected roots: its histograms are those of a run without.

    ``groups``: a :class:`WeightGroups` (:func:`groups_from_dof`).  Every root is weighted by the jacobian of its own group's variables
    -- the integral over the others is not taken, as with MCIntegration's ``dof`` -- and a variable's histogram sums, over the groups
    that own it, ``(w_g sum_k c_k r_k)**2`` of the group's roots; a variable of no group is not refined.  The sums, ``reduce`` and
    ``combine`` are as without.  None: the calls made and their bits are what they are without this keyword.

    ``observables``: an :class:`Observables`.  The one accumulate call of an iteration is then fdg_mc_accumulate_device_observables,
    which carries every other block and leaves their bits as they are; it also sums ``o_m = sum_k coef[m][k] w_g(k) root_k`` and the
    products ``o_a o_c`` (``reduce`` is applied to both).  ``mc_covariance`` gives every iteration's ``(mean, C)``
    (``obs_iterations``), and :func:`combine_covariance` the results ``obs_mean``, ``obs_stderr``, ``obs_chi2_dof`` ``[n_obs]`` and
    ``obs_cov`` ``[n_obs, n_obs]``.  Real observables of the unprojected roots only, also beside ``matsubara``.  None: the calls made
    and their bits are what they are without this keyword.

    ``freq_observables``: a :class:`FrequencyObservables`; needs ``matsubara``.  The one accumulate call of an iteration is then
    fdg_mc_accumulate_device_freq_observables, which carries every other block (the projection, ``groups``, ``observables``) and
    leaves their bits as they are; per (bin,) frequency it also sums the ``2 M`` real components ``Re o_m``, ``Im o_m`` of
    ``o_m = sum_k coef[m][k] w_g(k) root_k e^{i omega_n tau_k}`` and their products (``reduce`` is applied to both).  ``mc_covariance``
    gives every iteration's ``(mean, C)`` on the components (``fobs_iterations``) and :func:`combine_covariance` the results:
    ``fobs_mean`` complex ``[n_freq, M]``, ``fobs_stderr`` and ``fobs_chi2_dof`` complex as ``matsubara`` reports them,
    ``fobs_cov`` real ``[n_freq, 2 M, 2 M]``.  None: the calls made and their bits are what they are without this keyword.

    ``strat``: a :class:`Stratification` (:func:`strat_for`): adaptive stratified sampling on top of the map.  Per iteration: sample
    through fdg_vegas_sample_device_strat by the current allocation (the first is uniform), accumulate through
    fdg_mc_accumulate_device_strat, refine the map, fdg_strat_allocate from column ``n_root`` of the per-hypercube moments (the
    ``coef`` combination).  ``mean`` is ``acc / n_total`` and the reported variance per root ``sum_h n_h var_h(t_k) / n_total**2``;
    the iterations combine through :func:`combine`, ``cube_counts`` keeps every iteration's samples per hypercube.  A sample's
    index places it in its hypercube, so ``sample_offset`` is ``shard_start`` in every iteration and iteration ``it`` draws with the
    Philox key ``seed + it * 0x9E3779B97F4A7C15`` (mod 2**64).  ``reduce`` is applied to the moments, the histogram and the
    per-hypercube moments ``[2, H, n_root + 1]``.  ``tables`` may then be None: the leaf form, where the columns of ``x`` are the
    graph's leaves themselves (fdg_accumulate_device_strat), ``col[d]`` the leaf that variable ``d`` fills and ``fixed`` the values
    of the others.  Together with ``polar``, ``matsubara``, ``groups``, ``observables`` or ``freq_observables`` (and with a discrete variable) it raises
    ValueError: ``polar`` and ``groups`` go through :func:`vegas_integrate_stratified`, the others are not built yet.  None: the calls made and their bits are what they are without this keyword."""
    shared = dict(n_iter=n_iter, n_sample=n_sample, n_grid=n_grid, alpha=alpha, seed=seed, n_discard=n_discard, fixed=fixed, coef=coef,
                  device=device, vmap=vmap, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start, reduce=reduce)
    if strat is not None:
        if polar or matsubara is not None or groups is not None or observables is not None or freq_observables is not None:
            raise ValueError("strat cannot be combined with polar, matsubara, groups, observables or freq_observables here "
                             "(polar and groups: vegas_integrate_stratified)")
        return _integrate_strat(func_or_handle, tables, lo, hi, col, kF, beta, lam, strat=strat, **shared)
    return _integrate(func_or_handle, tables, lo, hi, col, kF, beta, lam, dmap=None, floor=0.0, polar=polar, matsubara=matsubara, wgroups=groups,
                      observables=observables, freq_observables=freq_observables, **shared)


def uniform_cdf(n_bin: int) -> np.ndarray:
    """The flat discrete variable: ``cdf[j] = j / n_bin`` for ``j = 0 .. n_bin``, the last entry exactly 1; ``[n_bin + 1]``."""
    n = int(n_bin)
    if not (1 <= n <= capi.FDG_BIN_MAX):
        raise ValueError(f"n_bin must lie in [1, {capi.FDG_BIN_MAX}]")
    c = np.arange(n + 1, dtype=np.float64) / n
    c[n] = 1.0
    return c


class DiscreteMap:
    """A discrete variable on the host (``.cdf``, float64 ``[n_bin + 1]``: 0 .. 1, strictly increasing) and on ``device`` (``.d_cdf``),
    with the table of what its values mean: ``ext [n_bin, n_ext]`` (``.ext`` / ``.d_ext``), row ``j`` going to the columns ``ext_col`` of
    a sample that drew value ``j``."""

    def __init__(self, cdf: np.ndarray, ext=None, ext_col: Sequence[int] = (), device="cuda"):
        import torch
        c = np.ascontiguousarray(cdf, dtype=np.float64)
        if c.ndim != 1 or not (2 <= c.shape[0] <= capi.FDG_BIN_MAX + 1):
            raise ValueError(f"cdf must be [n_bin + 1] with n_bin in [1, {capi.FDG_BIN_MAX}]")
        if c[0] != 0.0 or c[-1] != 1.0 or not (np.diff(c) > 0).all():
            raise ValueError("cdf must run from 0 to 1 exactly, strictly increasing")
        self.cdf = c.copy()
        self.ext_col = [int(e) for e in ext_col]
        n_ext = len(self.ext_col)
        if n_ext > capi.FDG_VEGAS_EXT_MAX or len(set(self.ext_col)) != n_ext or any(e < 0 for e in self.ext_col):
            raise ValueError(f"ext_col must name at most {capi.FDG_VEGAS_EXT_MAX} distinct columns")
        if (ext is None) != (n_ext == 0):
            raise ValueError("ext and ext_col go together")
        self.ext = None
        if ext is not None:
            e = np.ascontiguousarray(ext, dtype=np.float64)
            if e.shape != (self.n_bin, n_ext):
                raise ValueError(f"ext must be [{self.n_bin}, {n_ext}]: one row per value, one column per ext_col")
            self.ext = e.copy()
        self.device = torch.device(device)
        self.d_cdf = torch.from_numpy(self.cdf).to(self.device)
        self.d_ext = None if self.ext is None else torch.from_numpy(self.ext).to(self.device)

    @property
    def n_bin(self) -> int:
        return self.cdf.shape[0] - 1

    @property
    def prob(self) -> np.ndarray:
        """``p_j = cdf[j + 1] - cdf[j]``: what the sampler divides the weight by"""
        return self.cdf[1:] - self.cdf[:-1]

    def refine(self, hist_bin, alpha: float = 0.5, floor: float = 0.05) -> "DiscreteMap":
        """Moves the probabilities by the training histogram ``hist_bin [n_bin]`` (a CUDA tensor or a host array) through
        ``fdg_vegas_refine_discrete`` and uploads them; a failed refinement leaves both copies as they were."""
        h = hist_bin.detach().cpu().numpy() if hasattr(hist_bin, "detach") else np.asarray(hist_bin, dtype=np.float64)
        capi.vegas_refine_discrete(self.cdf, h, alpha, floor)
        self.d_cdf.copy_(self.d_cdf.new_tensor(self.cdf))
        return self


@dataclass
class VegasBinnedResult:
    mean: np.ndarray                 # [n_bin, R] inverse-variance combination of the iterations kept, per (bin, root)
    stderr: np.ndarray               # [n_bin, R]
    chi2_dof: np.ndarray             # [n_bin, R]
    iterations: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # (mean, stderr) [n_bin, R] of every iteration
    map: Optional[VegasMap] = None
    dmap: Optional[DiscreteMap] = None
    histograms: List[np.ndarray] = field(default_factory=list)                       # [n_dim, n_grid] of every iteration
    bin_histograms: List[np.ndarray] = field(default_factory=list)                   # [n_bin] of every iteration
    obs_mean: Optional[np.ndarray] = None       # with ``observables``: [n_bin, n_obs], as ``mean``
    obs_stderr: Optional[np.ndarray] = None     # [n_bin, n_obs]
    obs_chi2_dof: Optional[np.ndarray] = None   # [n_bin, n_obs]
    obs_cov: Optional[np.ndarray] = None        # [n_bin, n_obs, n_obs] (:func:`combine_covariance`)
    obs_iterations: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # (mean [n_bin, n_obs], C [n_bin, n_obs, n_obs])
    fobs_mean: Optional[np.ndarray] = None      # with ``freq_observables``: complex [n_bin, n_freq, M]
    fobs_stderr: Optional[np.ndarray] = None    # complex [n_bin, n_freq, M]: the real parts' figures in .real, the imaginary parts' in .imag
    fobs_chi2_dof: Optional[np.ndarray] = None  # complex [n_bin, n_freq, M], likewise
    fobs_cov: Optional[np.ndarray] = None       # real [n_bin, n_freq, 2 M, 2 M]
    fobs_iterations: List[Tuple[np.ndarray, np.ndarray]] = field(default_factory=list)   # (mean [n_bin, n_freq, 2 M], C [.., 2 M, 2 M])


def vegas_integrate_binned(func_or_handle, tables, lo, hi, col, dmap: DiscreteMap, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *,
                           n_iter: int = 10, n_sample: int = 100_000, n_grid: int = 64, alpha: float = 0.5, floor: float = 0.05, seed: int = 0,
                           n_discard: int = 0, fixed=None, coef=None, device="cuda", vmap: Optional[VegasMap] = None,
                           specialize_fused: bool = True, n_total: Optional[int] = None, shard_start: int = 0,
                           reduce: Optional[Callable] = None, polar: Optional[Sequence[PolarVar]] = None,
                           matsubara: Optional[MatsubaraProjection] = None,
                           groups: Optional[WeightGroups] = None, observables: Optional[Observables] = None,
                           strat: Optional[Stratification] = None,
                           freq_observables: Optional[FrequencyObservables] = None) -> VegasBinnedResult:
    """:func:`vegas_integrate` with a discrete variable: every sample draws a value ``j`` of ``dmap`` next to its continuous variables,
    the columns ``dmap.ext_col`` take row ``j`` of ``dmap.ext`` (external momenta), and the estimate is per value: arrays ``[n_bin, R]``,
    bin ``j`` the integral over the continuous variables at configuration ``j`` (the weight carries ``1 / p_j``, and ``mc_estimate``
    takes the whole batch as ``N``).  Per iteration: sample, accumulate (binned moments and both training histograms in one pass),
    ``mc_estimate``, refine the map with ``alpha`` and the probabilities with ``alpha`` and ``floor``.  ``combine`` is per (bin, root).
    Sharding as in :func:`vegas_integrate`; ``reduce`` is applied to the moments ``[2, n_bin, R]`` and to both histograms, so every rank
    refines the same maps.  ``polar``, ``matsubara`` and ``groups`` as in :func:`vegas_integrate` (complex ``[n_bin, n_freq, R]``; the
    discrete variable is shared by every group); ``observables`` too: ``obs_mean`` ``[n_bin, n_obs]``, ``obs_cov`` ``[n_bin, n_obs, n_obs]``;
    ``freq_observables`` too: ``fobs_mean`` complex ``[n_bin, n_freq, M]``, ``fobs_cov`` ``[n_bin, n_freq, 2 M, 2 M]``.
    ``strat`` is not built for a discrete variable yet: anything but None raises ValueError."""
    if strat is not None:
        raise ValueError("strat cannot be combined with a discrete variable (dmap)")
    return _integrate(func_or_handle, tables, lo, hi, col, kF, beta, lam, dmap=dmap, floor=floor, n_iter=n_iter, n_sample=n_sample, n_grid=n_grid,
                      alpha=alpha, seed=seed, n_discard=n_discard, fixed=fixed, coef=coef, device=device, vmap=vmap,
                      specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start, reduce=reduce, polar=polar,
                      matsubara=matsubara, wgroups=groups, observables=observables, freq_observables=freq_observables)


# ---- Markov-chain sampling on the VEGAS map (include/fdg.h: fdg_chain_propose_device, fdg_[mc_]chain_step_device, fdg_chain_reduce_device) ---- #
@dataclass
class ChainResult:
    mean: np.ndarray                 # [R] S_k / S_R: the integral of every root; with ``matsubara`` complex [n_freq, R]
    stderr: np.ndarray               # [R] from the spread across the walkers (:func:`chain_estimate`); with ``matsubara`` complex
                                     # [n_freq, R]: the error of the real part in the real part, of the imaginary part in the imaginary
    acceptance: float                # mean over the walkers of n_accept / n_step
    gamma: float                     # the weight of the map's own density in the stationary density
    map: Optional[VegasMap] = None   # the map the chain drew its proposals through
    S: Optional[np.ndarray] = None   # [R + 1] sum over the walkers of their sums A_c(b); A_R is the normalisation.  With ``matsubara``
                                     # S, Q, X are raw over the 2 n_freq R columns 2 (f R + k) (real part), + 1 (imaginary part)
    Q: Optional[np.ndarray] = None   # [R + 1] sum over the walkers of A_c(b)**2
    X: Optional[np.ndarray] = None   # [R] sum over the walkers of A_k(b) A_R(b)
    shift_width: Optional[np.ndarray] = None   # [D] the half widths of the shifts of the measured steps (:func:`chain_integrate_shift`)
    reweight: Optional[np.ndarray] = None   # [n_group] the factor of every weight group (:func:`chain_integrate_grouped`)


@dataclass
class ChainObservablesResult(ChainResult):
    """What :func:`chain_integrate_observables` returns: a :class:`ChainResult` (whose own last field stays ``reweight``) with the
    observables behind it, in the shapes and conventions of VegasResult's; with ``dmap`` every array has a leading n_bin axis."""
    obs_mean: Optional[np.ndarray] = None    # with ``observables``: [n_obs] the combinations of the roots
    obs_cov: Optional[np.ndarray] = None     # [n_obs, n_obs] their covariance over the walkers (:func:`chain_estimate_observables`)
    obs_stderr: Optional[np.ndarray] = None  # [n_obs] sqrt of its diagonal
    fobs_mean: Optional[np.ndarray] = None   # with ``freq_observables``: complex [n_freq, M]
    fobs_stderr: Optional[np.ndarray] = None  # complex [n_freq, M]: the real parts' figures in .real, the imaginary parts' in .imag
    fobs_cov: Optional[np.ndarray] = None    # real [n_freq, 2 M, 2 M]: the components (Re o_0 .., Im o_0 ..)
    obs_sums: Optional[np.ndarray] = None    # [V] the raw sums (S, P packed) of fdg_chain_reduce_device_observables, additive over shards
    fobs_sums: Optional[np.ndarray] = None   # [n_freq, V] those of every frequency's block, over the 2 M components
    walker_sums: object = None               # with ``keep_sums``: the walkers' sums [n_columns, n_walker] of this shard, on the device


def chain_estimate(S, Q, X, n_walker: int):
    """``(mean, stderr)`` per root from the reduced sums of a chain run (fdg_chain_reduce_device): with ``B = n_walker`` independent
    walkers whose sums are ``A_c(b)``, ``m_k = S_k / S_R``, ``V_cd = B / (B - 1) (sum_b A_c A_d - S_c S_d / B)`` for the pairs the sums
    provide, and ``var(m_k) = (V_kk - 2 m_k V_kR + m_k**2 V_RR) / S_R**2``: the delta method for a ratio over independent walkers.
    ``B = 1`` has no spread to measure: every stderr is nan.  ``S_R = 0`` (nothing was measured) raises ValueError; a variance that
    rounding leaves below zero is reported as 0."""
    S, Q, X = (np.asarray(v, dtype=np.float64) for v in (S, Q, X))
    R, B = X.shape[0], int(n_walker)
    if S.shape != (R + 1,) or Q.shape != (R + 1,) or B < 1:
        raise ValueError("need S, Q of n_root + 1 sums, X of n_root and n_walker >= 1")
    if not S[R] > 0.0:
        raise ValueError("S_R, the sum of the normalisation, is not positive: no step was measured")
    mean = S[:R] / S[R]
    if B == 1:
        return mean, np.full(R, np.nan)
    f = B / (B - 1.0)
    Vkk = f * (Q[:R] - S[:R] * S[:R] / B)
    VkR = f * (X - S[:R] * S[R] / B)
    VRR = f * (Q[R] - S[R] * S[R] / B)
    var = (Vkk - 2.0 * mean * VkR + mean * mean * VRR) / (S[R] * S[R])
    return mean, np.sqrt(np.maximum(var, 0.0))


def chain_estimate_observables(S, P, n_walker: int):
    """``(mean [M], cov [M, M])`` of ``M`` observables from the sums of fdg_chain_reduce_device_observables: ``S [M + 1]`` with the
    normalisation last, ``P`` the sums of products, packed upper triangle ``[(M + 1) (M + 2) / 2]`` row-major as the device writes
    it, or the full symmetric ``[M + 1, M + 1]``.  With ``B = n_walker`` independent walkers ``m_p = S_p / S_M``, ``V_pq = B / (B - 1)
    (P_pq - S_p S_q / B)`` and ``cov(m_p, m_q) = (V_pq - m_q V_pM - m_p V_qM + m_p m_q V_MM) / S_M**2``: the delta method for ratios
    that share their walkers and their denominator.  The diagonal for a unit row is :func:`chain_estimate`'s variance.  ``B = 1``
    gives nan covariances; ``S_M`` not positive raises ValueError; a diagonal that rounding leaves below zero is reported as 0."""
    S, P = np.asarray(S, dtype=np.float64), np.asarray(P, dtype=np.float64)
    M, B = S.shape[0] - 1 if S.ndim == 1 else -1, int(n_walker)
    if M < 1 or B < 1:
        raise ValueError("need S of n_obs + 1 >= 2 sums and n_walker >= 1")
    if P.shape == ((M + 1) * (M + 2) // 2,):
        full = np.zeros((M + 1, M + 1))
        full[np.triu_indices(M + 1)] = P
        P = full + np.triu(full, 1).T
    elif P.shape != (M + 1, M + 1):
        raise ValueError("P must be the packed upper triangle [(M + 1) (M + 2) / 2] or [M + 1, M + 1]")
    if not S[M] > 0.0:
        raise ValueError("S_M, the sum of the normalisation, is not positive: no step was measured")
    mean = S[:M] / S[M]
    if B == 1:
        return mean, np.full((M, M), np.nan)
    V = (B / (B - 1.0)) * (P - np.outer(S, S) / B)
    t = mean[None, :] * V[:M, M][:, None]                   # [p, q] = m_q V_pM
    cov = (V[:M, :M] - (t + t.T) + np.outer(mean, mean) * V[M, M]) / (S[M] * S[M])
    d = np.arange(M)
    cov[d, d] = np.maximum(cov[d, d], 0.0)
    return mean, cov


def chain_complex(v, n_freq: int, n_root: int) -> np.ndarray:
    """The complex ``[n_freq, R]`` array of the ``2 n_freq R`` figures that the projected chain keeps per column ``2 (f R + k)`` (real
    part) and ``2 (f R + k) + 1`` (imaginary part): means, or error bars with each part's own error in that part."""
    v = np.asarray(v, dtype=np.float64).reshape(int(n_freq), int(n_root), 2)
    out = np.empty(v.shape[:2], dtype=np.complex128)
    out.real, out.imag = v[..., 0], v[..., 1]               # (not re + 1j * im: a nan of one part would spread to the other)
    return out


def chain_moves(n_dim: int) -> List[int]:
    """The default moves of :func:`chain_integrate`: the mask of all variables, then one mask per variable."""
    D = int(n_dim)
    return [(1 << D) - 1] + [1 << d for d in range(D)]


def chain_moves_polar(n_dim: int, polar) -> List[int]:
    """The default moves of :func:`chain_integrate_polar`: the mask of all ``n_dim`` variables (the discrete one counted, where there
    is one), then one mask per unit in the order of the units' first variables: a polar group (``polar``: :class:`PolarVar` or
    ``(var, cols)`` pairs) with all its variables, a variable of no group, the discrete variable."""
    D = int(n_dim)
    first = {}
    for p in polar:
        var, cols = (p.var, p.cols) if isinstance(p, PolarVar) else p
        first[int(var)] = len(cols)
    out, d = [(1 << D) - 1], 0
    while d < D:
        n = first.get(d, 1)
        out.append(((1 << n) - 1) << d)
        d += n
    return out


@dataclass
class ChainShift:
    """The local moves of :func:`chain_integrate_shift`: a variable is displaced in the map's uniform coordinate, ``y' = y + t h
    (mod 1)`` with ``t`` uniform in ``[-1, 1)``.  ``width``: the half width ``h`` in ``(0, 0.5]``, one number or one per variable.
    ``moves``: pairs ``(redraw_mask, shift_mask)``, one per step in turn (None: :func:`chain_moves_shift`).  ``tune``: adapt the widths
    towards the acceptance ``target`` during the discarded steps."""
    width: object = 0.1
    moves: Optional[Sequence[Tuple[int, int]]] = None
    tune: bool = False
    target: float = 0.44


def chain_moves_shift(n_dim: int, polar=(), discrete: bool = False) -> List[Tuple[int, int]]:
    """The default moves of :func:`chain_integrate_shift`, pairs ``(redraw_mask, shift_mask)`` over ``n_dim`` continuous variables:
    everything redrawn (the discrete variable, bit ``n_dim``, too), then one move per unit in the order of the units' first variables:
    a variable of no group shifted, a polar group (``polar``: :class:`PolarVar` or ``(var, cols)`` pairs) redrawn whole, the discrete
    variable redrawn.  The one whole redraw stays because a cycle of shifts alone thermalises slowly from the map's placement."""
    D = int(n_dim)
    first = {}
    for p in polar:
        var, cols = (p.var, p.cols) if isinstance(p, PolarVar) else p
        first[int(var)] = len(cols)
    out, d = [((1 << (D + bool(discrete))) - 1, 0)], 0
    while d < D:
        n = first.get(d, 0)
        out.append(((((1 << n) - 1) << d), 0) if n else (0, 1 << d))
        d += max(n, 1)
    if discrete:
        out.append((1 << D, 0))
    return out


def chain_tune_width(h: float, n_accepted, n_total: int, target: float) -> float:
    """The width of a one-variable shift after a tuned step: ``r`` = the step's acceptances over the walkers,
    ``h <- clip(h r / target, h / 2, 2 h)``, then into ``[2**-20, 0.5]``."""
    r = float(n_accepted) / int(n_total)
    return min(max(min(max(h * r / target, h / 2.0), 2.0 * h), 2.0 ** -20), 0.5)


_CHAIN_EXCLUDED = ("polar", "groups", "dmap", "observables", "freq_observables", "strat")
_CHAIN_TRAIN_KEY = 0x632BE59BD9B4E019       # added to ``seed`` for the map's training: the chain's counters are used once


def _refuse_excluded(driver: str, excluded) -> None:
    """The keywords a chain driver has no parameter for: a name outside ``_CHAIN_EXCLUDED`` is unknown to ``driver``, a value of one
    inside it is refused (an empty ``polar`` is none)."""
    for name, value in excluded.items():
        if name not in _CHAIN_EXCLUDED:
            raise TypeError(f"{driver}() got an unexpected keyword argument '{name}'")
        if value is not None and not (name == "polar" and not value):
            raise ValueError(f"{name} cannot be combined with the chain yet")


def _check_kinds(polar, dmap, groups, reweight):
    """The kinds of the optional keywords the later chain drivers share, behind each driver's own checks; returns ``polar`` as a list."""
    if polar is not None:
        polar = list(polar)
        if not all(isinstance(p, PolarVar) for p in polar):
            raise ValueError("polar must be a sequence of PolarVar")
    if dmap is not None and not isinstance(dmap, DiscreteMap):
        raise ValueError("dmap must be a DiscreteMap")
    if groups is not None and not isinstance(groups, WeightGroups):
        raise ValueError("groups must be a WeightGroups")
    if groups is None and reweight is not None:
        raise ValueError("reweight goes with groups")
    return polar


def chain_integrate(func_or_handle, tables, lo, hi, col, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *, n_walker: int,
                    n_step: int, n_therm: int, moves: Optional[Sequence[int]] = None, gamma_rel: float = 1.0, gamma: Optional[float] = None,
                    n_warm: int = 5, n_warm_sample: Optional[int] = None, n_grid: int = 64, alpha: float = 0.5, seed: int = 0, fixed=None,
                    coef=None, vmap: Optional[VegasMap] = None, specialize_fused: bool = True, n_total: Optional[int] = None,
                    shard_start: int = 0, reduce: Optional[Callable] = None, device="cuda",
                    matsubara: Optional[MatsubaraProjection] = None, weight_freq: int = 0, **excluded) -> ChainResult:
    """Integrates the roots of a graph over the box ``[lo, hi]`` with a Metropolis chain whose proposals are fresh draws through the
    VEGAS map for a subset of the variables (MCIntegration's ``:vegasmc``; no counterpart in the reference: the caller's side of
    test/hubbard.jl:85).  ``n_walker`` independent walkers, one per lane; the stationary density is ``|s| + gamma q`` with ``s`` the
    ``coef`` combination of the roots and ``q`` the map's own density, whose known integral 1 normalises the result (include/fdg.h).

    The arguments up to ``lam``, ``fixed``, ``coef``, ``vmap``, ``specialize_fused`` and ``device`` are :func:`vegas_integrate`'s;
    ``tables`` None is the leaf form (the columns of ``x`` are the graph's leaves).  Procedure:

    1. the map is trained by ``n_warm`` plain ``vegas_integrate`` iterations of ``n_warm_sample`` (default ``n_walker``) samples, on
       a Philox key of its own; skipped with ``n_warm = 0`` (then ``vmap``, or the uniform map, is used as it is).  The leaf form
       trains through the stratified driver with one stratum per variable, which is the plain step;
    2. FDG_CHAIN_INIT places the walkers with all variables drawn (``sample_offset = shard_start``);
    3. ``gamma = gamma_rel * mean(a)`` unless ``gamma`` is given: the mean over the walkers (all of them: ``reduce`` is applied to
       the sum) of ``a = |jac s|`` is the map's estimate of the integral of ``|s|``;
    4. ``n_step`` steps; step ``t`` redraws the variables of ``moves[t % len(moves)]`` (bit ``d`` = variable ``d``; default
       :func:`chain_moves`) with ``sample_offset = (t + 1) * n_total + shard_start`` and ``seed``, and measures from step
       ``n_therm`` on;
    5. fdg_chain_reduce_device, ``reduce`` on the ``3 R + 2`` sums, :func:`chain_estimate` with ``n_total`` walkers.

    Sharding is :func:`vegas_integrate`'s: a rank passes its range as ``shard_start`` / ``n_walker`` and the whole as ``n_total``;
    a walker's chain does not depend on the split.

    ``matsubara`` (a :class:`MatsubaraProjection`) projects the roots onto its frequencies INSIDE the chain
    (fdg_[mc_]chain_step_device_matsubara): the walkers' weight is ``a = |jac sum_k c_k r_k e^{i omega tau_k}|`` at the frequency
    ``freq[weight_freq]``, and every root is measured at every frequency, so ``mean`` and ``stderr`` are complex ``[n_freq, R]``
    (the errors of the two parts kept apart, as ``vegas_integrate(matsubara=...)`` reports them) and ``S``, ``Q``, ``X`` the raw sums
    over the ``2 n_freq R`` columns.  The projection's 1-based time label ``i`` names column ``t0 + i - 1`` of ``x``: ``t0 = n_loop *
    dim`` in the Monte-Carlo form, and ``t0 = 0`` in the leaf form, where a "time" is a leaf column (of use to tests).  The warm-up
    still trains the map on the unprojected ``s``, and ``gamma = gamma_rel * mean(a)`` is taken of the projected ``a``.

    Out of scope here, refused with ValueError: ``polar``, ``groups``, a discrete variable (``dmap``), ``observables``,
    ``freq_observables`` (both are :func:`chain_integrate_observables`'s) and ``strat`` together with the chain.  Not built either: training the map from the chain's own samples,
    reweighting between orders; local (shift) proposals are :func:`chain_integrate_shift`'s.  The target these lead to is ``Sigma(i omega_0)`` of the Hubbard atom in
    the reference's test/hubbard.jl: its single-order case is what ``matsubara`` reaches; several orders at once need ``groups``,
    which :func:`chain_integrate_grouped` takes (with the reweighting between orders)."""
    _refuse_excluded("chain_integrate", excluded)
    return _chain(func_or_handle, tables, lo, hi, col, kF, beta, lam, n_walker=n_walker, n_step=n_step, n_therm=n_therm, moves=moves,
                  gamma_rel=gamma_rel, gamma=gamma, n_warm=n_warm, n_warm_sample=n_warm_sample, n_grid=n_grid, alpha=alpha, seed=seed,
                  fixed=fixed, coef=coef, vmap=vmap, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start,
                  reduce=reduce, device=device, matsubara=matsubara, weight_freq=weight_freq)


def chain_integrate_grouped(func_or_handle, tables, lo, hi, col, groups: WeightGroups, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *,
                            n_walker: int, n_step: int, n_therm: int, moves: Optional[Sequence[int]] = None, gamma_rel: float = 1.0,
                            gamma: Optional[float] = None, n_warm: int = 5, n_warm_sample: Optional[int] = None, n_grid: int = 64,
                            alpha: float = 0.5, seed: int = 0, fixed=None, coef=None, vmap: Optional[VegasMap] = None,
                            specialize_fused: bool = True, n_total: Optional[int] = None, shard_start: int = 0,
                            reduce: Optional[Callable] = None, device="cuda", reweight=None,
                            matsubara: Optional[MatsubaraProjection] = None, weight_freq: int = 0, **excluded) -> ChainResult:
    """:func:`chain_integrate` with weight groups (``groups``: a :class:`WeightGroups`, :func:`groups_from_dof`), which that function
    refuses: several orders of a series in one run, every order with its own variables, MCIntegration's ``:vegasmc`` with several
    integrands (fdg_[mc_]chain_step_device_grouped; include/fdg.h).  The walkers' weight is ``a = sum_g rho_g |jac_g s_g|`` with
    ``jac_g`` the jacobian of the variables of group ``g`` only, ``s_g`` the ``coef`` combination of the group's roots and ``rho_g``
    the reweight factor that balances the orders; root ``k`` is measured with the jacobian of its own group.  With ``matsubara`` the
    group's sum is projected at ``freq[weight_freq]`` as in :func:`chain_integrate`.  Every other argument and the result are that
    function's; ``ChainResult.reweight`` holds the factors used.  Procedure:

    1. the map is trained by the grouped direct sampler: ``vegas_integrate(groups=...)`` in the Monte-Carlo form,
       ``vegas_integrate_stratified(..., Stratification((1,) * D), groups=...)`` in the leaf form; skipped with ``n_warm = 0``;
    2. unless ``reweight`` is given, FDG_CHAIN_INIT places the walkers without factors, and ``rho_g = 1 / mean_b |jac_g s_g|`` is
       taken from the placed ``fac`` and ``root`` (all walkers: ``reduce`` is applied to the sums), so that every group carries the
       same share of the density.  This is the UNPROJECTED ``s_g``, also under ``matsubara``.  A group with a root that exists whose
       mean is 0 or not finite raises ValueError asking for ``reweight``; a group without such a root gets the factor 1;
    3. FDG_CHAIN_INIT places the walkers on the same counters with ``rho``; ``gamma = gamma_rel * mean(a)``;
    4. the steps, the reduction and :func:`chain_estimate` as in :func:`chain_integrate`.

    ``reweight``: one finite factor > 0 per group.  Refused with ValueError: ``polar``, ``dmap``, ``observables``,
    ``freq_observables`` (:func:`chain_integrate_observables` takes both) and ``strat``."""
    _refuse_excluded("chain_integrate_grouped", excluded)
    if not isinstance(groups, WeightGroups):
        raise ValueError("groups must be a WeightGroups")
    return _chain(func_or_handle, tables, lo, hi, col, kF, beta, lam, n_walker=n_walker, n_step=n_step, n_therm=n_therm, moves=moves,
                  gamma_rel=gamma_rel, gamma=gamma, n_warm=n_warm, n_warm_sample=n_warm_sample, n_grid=n_grid, alpha=alpha, seed=seed,
                  fixed=fixed, coef=coef, vmap=vmap, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start,
                  reduce=reduce, device=device, matsubara=matsubara, weight_freq=weight_freq, wgroups=groups, reweight=reweight)


def chain_integrate_binned(func_or_handle, tables, lo, hi, col, dmap: DiscreteMap, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *,
                           n_walker: int, n_step: int, n_therm: int, moves: Optional[Sequence[int]] = None, gamma_rel: float = 1.0,
                           gamma: Optional[float] = None, n_warm: int = 5, n_warm_sample: Optional[int] = None, n_grid: int = 64,
                           alpha: float = 0.5, floor: float = 0.05, seed: int = 0, fixed=None, coef=None, vmap: Optional[VegasMap] = None,
                           specialize_fused: bool = True, n_total: Optional[int] = None, shard_start: int = 0,
                           reduce: Optional[Callable] = None, device="cuda", groups: Optional[WeightGroups] = None, reweight=None,
                           matsubara: Optional[MatsubaraProjection] = None, weight_freq: int = 0, **excluded) -> ChainResult:
    """:func:`chain_integrate` with a discrete variable (``dmap``: a :class:`DiscreteMap` of at most ``FDG_CHAIN_BIN_MAX`` values),
    which that function refuses: the walkers move over ``(x, j)``, the columns ``dmap.ext_col`` take row ``j`` of ``dmap.ext``
    (external momenta), and every root is measured per value (fdg_chain_propose_device_discrete, fdg_[mc_]chain_step_device_binned;
    include/fdg.h).  ``mean`` and ``stderr`` are ``[n_bin, R]``, with ``matsubara`` complex ``[n_bin, n_freq, R]``: entry ``j`` is the
    integral over the continuous variables at configuration ``j`` (the weight carries ``1 / p_j``, as in
    :func:`vegas_integrate_binned`), with its own error bar; ``S``, ``Q``, ``X`` are raw over the ``n_bin R`` (``2 n_bin n_freq R``)
    columns.  This is the sampler's side of the reference's test/ver4.jl: ``ExtKidx = Discrete(1, Nk)`` and an observable per value.

    A move is an int whose bit ``d < D`` names variable ``d`` and whose bit ``D`` names the discrete variable; the default is
    ``chain_moves(D + 1)``.  ``groups`` (with ``reweight``), ``matsubara`` and ``weight_freq`` as in :func:`chain_integrate_grouped`
    and :func:`chain_integrate`; the discrete variable is shared by every group, and ``rho_g`` is taken of ``|jac_g s_g|`` with the
    factor ``1 / p_j`` in ``jac_g``.  ``gamma``, ``sample_offset`` and sharding as there.  The warm-up of the Monte-Carlo form is
    ``n_warm`` iterations of ``vegas_integrate_binned(..., groups=groups)``, which train the map and ``dmap`` (in place, with
    ``alpha`` and ``floor``); the leaf form has no such driver, so there ``n_warm > 0`` raises ValueError and ``vmap`` / ``dmap``
    are used as given.

    Refused with ValueError: ``polar``, ``observables``, ``freq_observables`` (:func:`chain_integrate_observables` takes both) and
    ``strat``; more than ``FDG_VEGAS_DIM_MAX - 1``
    continuous variables (the discrete variable's Philox column would be the accept rule's)."""
    _refuse_excluded("chain_integrate_binned", excluded)
    if not isinstance(dmap, DiscreteMap):
        raise ValueError("dmap must be a DiscreteMap")
    _check_kinds(None, dmap, groups, reweight)
    return _chain(func_or_handle, tables, lo, hi, col, kF, beta, lam, n_walker=n_walker, n_step=n_step, n_therm=n_therm, moves=moves,
                  gamma_rel=gamma_rel, gamma=gamma, n_warm=n_warm, n_warm_sample=n_warm_sample, n_grid=n_grid, alpha=alpha, seed=seed,
                  fixed=fixed, coef=coef, vmap=vmap, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start,
                  reduce=reduce, device=device, matsubara=matsubara, weight_freq=weight_freq, wgroups=groups, reweight=reweight, dmap=dmap,
                  floor=floor)


def chain_integrate_polar(func_or_handle, tables, lo, hi, col, polar: Sequence[PolarVar], kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *,
                          n_walker: int, n_step: int, n_therm: int, moves: Optional[Sequence[int]] = None, gamma_rel: float = 1.0,
                          gamma: Optional[float] = None, n_warm: int = 5, n_warm_sample: Optional[int] = None, n_grid: int = 64,
                          alpha: float = 0.5, floor: float = 0.05, seed: int = 0, fixed=None, coef=None, vmap: Optional[VegasMap] = None,
                          specialize_fused: bool = True, n_total: Optional[int] = None, shard_start: int = 0,
                          reduce: Optional[Callable] = None, device="cuda", groups: Optional[WeightGroups] = None, reweight=None,
                          dmap: Optional[DiscreteMap] = None, matsubara: Optional[MatsubaraProjection] = None, weight_freq: int = 0,
                          **excluded) -> ChainResult:
    """The chain with spherical momentum variables (``polar``: a sequence of :class:`PolarVar`, as in :func:`vegas_integrate`), which
    the other chain drivers refuse: the loop momenta are a modulus and a direction over a ball (:func:`ball`), MCIntegration's
    ``FermiK``, the way every caller of the chain in the reference draws them (test/hubbard.jl:85, test/ver4.jl:77-92;
    fdg_chain_propose_device_polar, include/fdg.h).  The ``col`` entry of a grouped variable is None; the group writes its own columns.

    The factors of the polar measure -- ``k**2`` and ``sin(theta)``, or ``k`` -- are kept per variable in the rows of ``fac`` the chain
    already carries, so the step is the one of :func:`chain_integrate`, :func:`chain_integrate_grouped` (``groups``, ``reweight``) or
    :func:`chain_integrate_binned` (``dmap``), with ``matsubara`` and ``weight_freq`` as there; the result has that driver's shapes.
    A polar group belongs to a weight group whole or not at all.

    A move redraws a polar group whole or not at all: the state holds the Cartesian columns, not ``(k, theta, phi)``, which moving the
    modulus or the direction alone would need.  A move naming part of a group raises ValueError; the default is
    :func:`chain_moves_polar`: everything, then one move per unit (a polar group, a variable of no group, the discrete variable).

    The warm-up is the direct sampler's with the same groups: ``vegas_integrate(polar=..., groups=...)`` in the Monte-Carlo form,
    ``vegas_integrate_binned(polar=..., groups=...)`` with ``dmap``, ``vegas_integrate_stratified(..., Stratification((1,) * D),
    polar=..., groups=...)`` in the leaf form; the leaf form with ``dmap`` has none (``n_warm > 0`` raises ValueError).

    Refused with ValueError: ``observables``, ``freq_observables`` (:func:`chain_integrate_observables` takes both) and ``strat``.  Not
    built: moving the modulus or the direction of a group alone."""
    _refuse_excluded("chain_integrate_polar", excluded)
    if polar is None:
        raise ValueError("polar must be a sequence of PolarVar")
    polar = _check_kinds(polar, dmap, groups, reweight)
    return _chain(func_or_handle, tables, lo, hi, col, kF, beta, lam, n_walker=n_walker, n_step=n_step, n_therm=n_therm, moves=moves,
                  gamma_rel=gamma_rel, gamma=gamma, n_warm=n_warm, n_warm_sample=n_warm_sample, n_grid=n_grid, alpha=alpha, seed=seed,
                  fixed=fixed, coef=coef, vmap=vmap, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start,
                  reduce=reduce, device=device, matsubara=matsubara, weight_freq=weight_freq, wgroups=groups, reweight=reweight, dmap=dmap,
                  floor=floor, polar=polar)


def chain_integrate_shift(func_or_handle, tables, lo, hi, col, shift: ChainShift, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *,
                          n_walker: int, n_step: int, n_therm: int, gamma_rel: float = 1.0, gamma: Optional[float] = None, n_warm: int = 5,
                          n_warm_sample: Optional[int] = None, n_grid: int = 64, alpha: float = 0.5, floor: float = 0.05, seed: int = 0,
                          fixed=None, coef=None, vmap: Optional[VegasMap] = None, specialize_fused: bool = True,
                          n_total: Optional[int] = None, shard_start: int = 0, reduce: Optional[Callable] = None, device="cuda",
                          groups: Optional[WeightGroups] = None, reweight=None, dmap: Optional[DiscreteMap] = None,
                          polar: Optional[Sequence[PolarVar]] = None, matsubara: Optional[MatsubaraProjection] = None, weight_freq: int = 0,
                          **excluded) -> ChainResult:
    """The chain with LOCAL moves (``shift``: a :class:`ChainShift`), which the other chain drivers lack: a variable is displaced by a
    small step instead of being redrawn whole -- the way ``integrate(...; solver=:mcmc)`` of the reference's test/hubbard.jl:85 walks
    (fdg_chain_propose_device_local, include/fdg.h).  Diagram weights depend on differences of times and momenta; a separable map
    cannot adapt to such a ridge, and a whole redraw of a variable then lands off it most of the time.

    With ``x = map(y)`` the stationary density in the map's uniform coordinate ``y`` is exactly ``a + gamma``, so the step's rule
    ``u (a + gamma) < a' + gamma`` is the Metropolis rule of every proposal that is symmetric in ``y``.  A redraw is the uniform one;
    the shift ``y' = y + t h (mod 1)``, ``t`` uniform in ``[-1, 1)``, is another.  So the step entries are those of
    :func:`chain_integrate_polar` -- ``groups`` (with ``reweight``), ``dmap``, ``polar``, ``matsubara`` and ``weight_freq`` as there,
    with the same warm-up, placement, ``gamma``, sharding and result -- and only the proposal call differs.  FDG_CHAIN_INIT redraws
    everything, as in every driver.

    A move is a pair ``(redraw_mask, shift_mask)``: the variables of the first are redrawn through the map, those of the second
    shifted by their own ``shift.width``, the rest kept.  The default, :func:`chain_moves_shift`, is one whole redraw, then one move
    per unit: a shift of a variable of no group, a redraw of a polar group, a redraw of the discrete variable.

    ``shift.tune``: during the first ``n_therm`` steps only, after a step whose move shifts exactly one variable ``d`` and does nothing
    else, ``r`` = the step's acceptances over all walkers (``reduce`` is applied to the count, so every rank holds the same widths)
    and ``h_d <- clip(h_d r / target, h_d / 2, 2 h_d)``, then into ``[2**-20, 0.5]``.  From step ``n_therm`` on the widths are
    frozen, so the measured chain is stationary; ``ChainResult.shift_width`` holds them.  This is host arithmetic on integer counts:
    deterministic and independent of the split into shards.

    Refused with ValueError: a move whose two masks overlap; a shift of a variable of a polar group or of the discrete variable (the
    state holds Cartesian columns and no ``(k, theta, phi)``; inverting that is out of scope, as are local moves of the discrete
    variable); a width outside ``(0, 0.5]``; ``observables``, ``freq_observables`` (:func:`chain_integrate_observables` takes both,
    with ``shift``) and ``strat``.  Not built: training the map from
    the chain.  Whether shifts lower the error on a given workload has not been measured."""
    _refuse_excluded("chain_integrate_shift", excluded)
    if not isinstance(shift, ChainShift):
        raise ValueError("shift must be a ChainShift")
    polar = _check_kinds(polar, dmap, groups, reweight)
    return _chain(func_or_handle, tables, lo, hi, col, kF, beta, lam, n_walker=n_walker, n_step=n_step, n_therm=n_therm, moves=None,
                  gamma_rel=gamma_rel, gamma=gamma, n_warm=n_warm, n_warm_sample=n_warm_sample, n_grid=n_grid, alpha=alpha, seed=seed,
                  fixed=fixed, coef=coef, vmap=vmap, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start,
                  reduce=reduce, device=device, matsubara=matsubara, weight_freq=weight_freq, wgroups=groups, reweight=reweight, dmap=dmap,
                  floor=floor, polar=polar or None, shift=shift)


def chain_integrate_observables(func_or_handle, tables, lo, hi, col, kF: float = 0.0, beta: float = 1.0, lam: float = 0.0, *,
                                n_walker: int, n_step: int, n_therm: int, observables: Optional[Observables] = None,
                                freq_observables: Optional[FrequencyObservables] = None, shift: Optional[ChainShift] = None,
                                moves: Optional[Sequence[int]] = None, gamma_rel: float = 1.0, gamma: Optional[float] = None,
                                n_warm: int = 5, n_warm_sample: Optional[int] = None, n_grid: int = 64, alpha: float = 0.5,
                                floor: float = 0.05, seed: int = 0, fixed=None, coef=None, vmap: Optional[VegasMap] = None,
                                specialize_fused: bool = True, n_total: Optional[int] = None, shard_start: int = 0,
                                reduce: Optional[Callable] = None, device="cuda", groups: Optional[WeightGroups] = None, reweight=None,
                                dmap: Optional[DiscreteMap] = None, polar: Optional[Sequence[PolarVar]] = None,
                                matsubara: Optional[MatsubaraProjection] = None, weight_freq: int = 0, keep_sums: bool = False,
                                **excluded) -> ChainObservablesResult:
    """The chain with OBSERVABLES, which the other chain drivers refuse: linear combinations of the roots with their covariance over
    the walkers -- what every caller of the chain in the reference reports (test/ver4.jl:184-216: a direct and an exchange sum;
    Sigma(i omega_n) of test/hubbard.jl: the sum over all orders).  All roots share their walkers, so the error of a sum is not the
    quadrature of the roots' errors (fdg_chain_reduce_device_observables, include/fdg.h).

    The chain is that of :func:`chain_integrate_shift` with the same keywords -- ``groups`` (with ``reweight``), ``dmap``, ``polar``,
    ``matsubara``, ``weight_freq`` -- except that ``shift`` is optional: without it the moves are redraws (``moves``, default as in
    the driver that takes the same keywords); with it ``moves`` must be None.  An observable is linear in the walkers' sums, so no
    step changes: ``mean``, ``stderr``, ``S``, ``Q``, ``X``, ``acceptance``, ``gamma`` and the widths are bit for bit those of the
    existing driver on the same arguments.  After its reduction the new entry runs once per block of the walkers' sums:

    ``observables`` (an :class:`Observables`, rows of ``n_root`` factors): per value of the discrete variable the window of its ``R``
    columns.  ``obs_mean [n_obs]``, ``obs_cov [n_obs, n_obs]``, ``obs_stderr``; with ``dmap`` a leading ``n_bin`` axis.  Refused with
    ``matsubara``: the chain's sums are then projected, and the unprojected combination does not exist.

    ``freq_observables`` (a :class:`FrequencyObservables`, needs ``matsubara``): per (value, frequency) the window of its ``2 R``
    interleaved columns, with ``2 M`` rows in the component order ``(Re o_0 .., Im o_0 ..)``.  ``fobs_mean`` and ``fobs_stderr`` complex
    ``[n_freq, M]`` (:func:`complex_components`), ``fobs_cov`` real ``[n_freq, 2 M, 2 M]``; with ``dmap`` a leading ``n_bin`` axis.

    At least one of the two must be given.  ``reduce`` is applied to the arrays of raw sums (``obs_sums``, ``fobs_sums``), which are
    additive over shards, as it is to the sums of the roots.  ``keep_sums``: ``walker_sums`` holds this shard's sums on the device.
    Covariances between blocks -- between values of the discrete variable, or between frequencies -- are not formed.  Refused with
    ValueError: ``strat``; everything :func:`chain_integrate_shift` refuses."""
    _refuse_excluded("chain_integrate_observables", excluded)
    if observables is None and freq_observables is None:
        raise ValueError("chain_integrate_observables needs observables or freq_observables")
    if observables is not None and not isinstance(observables, Observables):
        raise ValueError("observables must be an Observables")
    if freq_observables is not None and not isinstance(freq_observables, FrequencyObservables):
        raise ValueError("freq_observables must be a FrequencyObservables")
    if freq_observables is not None and matsubara is None:
        raise ValueError("freq_observables needs matsubara: the projection whose frequencies they are reported at")
    if observables is not None and matsubara is not None:
        raise ValueError("observables cannot be combined with matsubara in the chain: its sums are then projected, and the unprojected "
                         "combination does not exist")
    if shift is not None and not isinstance(shift, ChainShift):
        raise ValueError("shift must be a ChainShift")
    if shift is not None and moves is not None:
        raise ValueError("with shift the moves are shift.moves: moves must be None")
    polar = _check_kinds(polar, dmap, groups, reweight)
    return _chain(func_or_handle, tables, lo, hi, col, kF, beta, lam, n_walker=n_walker, n_step=n_step, n_therm=n_therm, moves=moves,
                  gamma_rel=gamma_rel, gamma=gamma, n_warm=n_warm, n_warm_sample=n_warm_sample, n_grid=n_grid, alpha=alpha, seed=seed,
                  fixed=fixed, coef=coef, vmap=vmap, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start,
                  reduce=reduce, device=device, matsubara=matsubara, weight_freq=weight_freq, wgroups=groups, reweight=reweight, dmap=dmap,
                  floor=floor, polar=polar or None, shift=shift, observables=observables, freq_observables=freq_observables,
                  keep_sums=bool(keep_sums))


def _chain_observable_rows(observables, freq_observables, R: int):
    """The rows of the two kinds of observables as the new reduction takes them, checked: ``(ocoef [n_obs, R] or None, frows [2 M, 2 R]
    or None)``; the frequency rows hold the real parts' factors at the window positions ``2 k`` and the imaginary parts' at ``2 k + 1``,
    in the component order ``(Re o_0 .., Im o_0 ..)``."""
    ocoef = frows = None
    if observables is not None:
        ocoef = _coef_table(observables, "observables", R, capi.FDG_OBS_MAX)
        if R > capi.FDG_CHAIN_OBS_COL_MAX:
            raise ValueError(f"the chain's observables take at most {capi.FDG_CHAIN_OBS_COL_MAX} roots")
    if freq_observables is not None:
        fcoef = _coef_table(freq_observables, "freq_observables", R, capi.FDG_FREQ_OBS_MAX)
        if 2 * R > capi.FDG_CHAIN_OBS_COL_MAX:
            raise ValueError(f"the chain's frequency observables take at most {capi.FDG_CHAIN_OBS_COL_MAX // 2} roots")
        M = fcoef.shape[0]
        frows = np.zeros((2 * M, 2 * R))
        frows[:M, 0::2], frows[M:, 1::2] = fcoef, fcoef
    return ocoef, frows


class _ChainPlan(namedtuple("_ChainPlan", "handle entry desc keep col n_col fx R F n_bin C B N n_step n_therm n_warm shard_start vmap D G DV "
                            "pgroups moves lmoves width ocoef frows NG rho mc coef gamma gamma_rel wgroups dmap shift device")):
    """What :func:`_chain_plan` decides of a chain run, and the arguments it checked that the later stages read as given.

    ``handle``; ``entry``: the step entry, "", "_matsubara", "_grouped" or "_binned"; ``desc``, ``keep``: the projection's descriptor
    (None without ``matsubara``) and what keeps its arrays alive; ``col``: as ints, None at a polar group's variables; ``n_col``,
    ``fx [n_col]``: the columns of ``x`` and their fixed values; ``R`` roots, ``F`` frequencies (0 without ``matsubara``), ``n_bin``
    values of the discrete variable (0 without ``dmap``); ``C``: the columns of the walkers' sums before the normalisation's; ``B``
    walkers of this shard, of ``N`` in all, from ``shard_start``; ``n_step``, ``n_therm``, ``n_warm`` as ints; ``vmap`` with its
    ``D`` variables and ``G`` cells; ``DV``: the variables a move can name, bit ``D`` the discrete one; ``pgroups``: the polar groups
    as ``(var, cols)`` pairs (None without ``polar``); ``moves``: the redraw mask of every move; ``lmoves``, ``width``: the moves'
    shift masks and the ``D`` half widths (None without ``shift``; the walk tunes ``width`` in place); ``ocoef``, ``frows``:
    :func:`_chain_observable_rows`; ``NG`` weight groups (0 without ``wgroups``) and ``rho``, ``reweight`` as given.
    As given: ``mc`` = ``(kF, beta, lam)`` (None: the leaf form), ``coef``, ``gamma``, ``gamma_rel``, ``wgroups``, ``dmap``,
    ``shift``, ``device`` (a ``torch.device``)."""
    __slots__ = ()


def _chain_plan(func_or_handle, tables, lo, hi, col, kF, beta, lam, *, n_walker, n_step, n_therm, n_warm, gamma_rel, n_grid, shard_start,
                weight_freq, device, moves=None, gamma=None, fixed=None, coef=None, vmap=None, n_total=None, matsubara=None, wgroups=None,
                reweight=None, dmap=None, polar=None, shift=None, observables=None, freq_observables=None) -> _ChainPlan:
    """The first stage of :func:`_chain`: every check of the arguments, in the order of the drivers' refusals, and every quantity the
    later stages derive from them.  Host work only: it runs with ``device="cpu"`` on a machine without a GPU."""
    import torch
    device = torch.device(device)
    handle, n_col_k, n_col, col, written = _columns(func_or_handle, tables, col, polar, polar is not None)
    R = handle.table.n_root
    ocoef, frows = _chain_observable_rows(observables, freq_observables, R)
    F, desc, keep = 0, None, None
    if matsubara is not None:
        if not isinstance(matsubara, MatsubaraProjection):
            raise ValueError("matsubara must be a MatsubaraProjection")
        F = len(matsubara.freq)
        t0, n_time = n_col_k, n_col - n_col_k                # (the leaf form: every column counts as a time)
        if not 1 <= F <= capi.FDG_MATSUBARA_FREQ_MAX:
            raise ValueError(f"matsubara needs 1 .. {capi.FDG_MATSUBARA_FREQ_MAX} frequencies")
        if not 0 <= int(weight_freq) < F:
            raise ValueError("weight_freq must be an index into matsubara.freq")
        if len(matsubara.root_tau_in) != R or len(matsubara.root_tau_out) != R:
            raise ValueError(f"matsubara must name the two times of each of the {R} roots")
        if not (math.isfinite(beta) and beta > 0.0):
            raise ValueError("beta must be finite and > 0")
        from .nodetable import FDG_NO_ROOT
        live = [int(v) != FDG_NO_ROOT for v in handle.table.root_slot]
        cin, cout = [], []
        for k in range(R):
            i, o = int(matsubara.root_tau_in[k]), int(matsubara.root_tau_out[k])
            if live[k] and not (1 <= i <= n_time and 1 <= o <= n_time):
                raise ValueError(f"matsubara: a time label of root {k} lies outside [1, {n_time}]")
            cin.append(t0 + i - 1 if live[k] else 0)
            cout.append(t0 + o - 1 if live[k] else 0)
        desc, keep = capi.make_chain_matsubara(matsubara.freq, matsubara.fermionic, int(weight_freq), cin, cout, beta)
    n_bin = 0
    if dmap is not None:
        if not isinstance(dmap, DiscreteMap):
            raise ValueError("dmap must be a DiscreteMap")
        n_bin = dmap.n_bin
        if n_bin > capi.FDG_CHAIN_BIN_MAX:
            raise ValueError(f"the chain takes at most {capi.FDG_CHAIN_BIN_MAX} values of the discrete variable")
        _check_ext_col(dmap, n_col, written, "that col does not name")
        if len(col) >= capi.FDG_VEGAS_DIM_MAX:
            raise ValueError(f"a discrete variable leaves room for {capi.FDG_VEGAS_DIM_MAX - 1} continuous ones")
        if tables is None and int(n_warm) > 0:
            raise ValueError("the leaf form has no warm-up with a discrete variable: pass n_warm=0 (vmap and dmap are used as given)")
    C = max(n_bin, 1) * (2 * F * R if F else R)            # the columns of the walkers' sums before the normalisation's
    B, n_step, n_therm, n_warm = int(n_walker), int(n_step), int(n_therm), int(n_warm)
    N = B if n_total is None else int(n_total)
    if B < 1 or n_step < 1 or not 0 <= n_therm < n_step or n_warm < 0 or not 0 <= int(shard_start) <= N - B:
        raise ValueError("need n_walker >= 1, 0 <= n_therm < n_step, n_warm >= 0 and the shard inside n_total")
    if gamma is not None and not (math.isfinite(gamma) and gamma > 0.0):
        raise ValueError("gamma must be finite and > 0")
    if gamma is None and not (math.isfinite(gamma_rel) and gamma_rel > 0.0):
        raise ValueError("gamma_rel must be finite and > 0")
    vmap = _map_for(vmap, lo, hi, n_grid, device, col)
    D, G = vmap.n_dim, vmap.n_grid
    DV = D + 1 if dmap is not None else D                   # the variables a move can name: bit D is the discrete one
    pgroups = None
    if polar is not None:
        pgroups = _polar_groups(polar, col, vmap, n_col)
        pbits = [((1 << len(cs)) - 1) << v for v, cs in pgroups]
        if moves is None and shift is None:
            moves = chain_moves_polar(DV, pgroups)
    lmoves = width = None                                   # the shift masks of the moves and the widths, with ``shift`` only
    if shift is not None:
        width = np.array(shift.width, dtype=np.float64)
        width = np.full(D, float(width)) if width.ndim == 0 else width
        if width.shape != (D,) or not (np.isfinite(width) & (width > 0.0) & (width <= 0.5)).all():
            raise ValueError("shift.width holds one half width in (0, 0.5], or one per variable of the map")
        if shift.tune and not (math.isfinite(shift.target) and 0.0 < shift.target < 1.0):
            raise ValueError("shift.target must lie in (0, 1)")
        pairs = chain_moves_shift(D, pgroups or (), dmap is not None) if shift.moves is None else [(int(r), int(s)) for r, s in shift.moves]
        for r, s in pairs:
            if not 0 <= s < (1 << DV):
                raise ValueError("moves holds pairs of masks over the variables of the map")
            if r & s:
                raise ValueError("a move redraws or shifts a variable, not both: its two masks overlap")
            if s >> D:
                raise ValueError("the discrete variable can only be redrawn, not shifted")
            if polar is not None and any(s & bits for bits in pbits):
                raise ValueError("a variable of a polar group can only be redrawn with its group: the state does not hold (k, theta, phi)")
        moves, lmoves = [r for r, _ in pairs], [s for _, s in pairs]
    moves = chain_moves(DV) if moves is None else [int(m) for m in moves]
    if not moves or not all(0 <= m < (1 << DV) for m in moves):
        raise ValueError("moves holds masks over the variables of the map" + (" and the discrete variable" if dmap is not None else ""))
    if polar is not None and any((m & bits) not in (0, bits) for m in moves for bits in pbits):
        raise ValueError("a move redraws a polar group whole or not at all: the state does not hold (k, theta, phi)")
    fx = _fixed(fixed, n_col)
    NG, rho = 0, None
    if wgroups is not None:
        NG = _check_weight_groups(wgroups, R, D, pgroups)
        if coef is not None and np.shape(coef) != (R,):
            raise ValueError(f"coef must hold n_root = {R} factors")
        if reweight is not None:
            rho = np.array(reweight, dtype=np.float64)
            if rho.shape != (NG,) or not (np.isfinite(rho) & (rho > 0.0)).all():
                raise ValueError("reweight must hold one finite factor > 0 per group")
    entry = "_binned" if dmap is not None else "_grouped" if wgroups is not None else "_matsubara" if desc is not None else ""
    return _ChainPlan(handle=handle, entry=entry, desc=desc, keep=keep, col=col, n_col=n_col, fx=fx, R=R, F=F, n_bin=n_bin, C=C, B=B, N=N,
                      n_step=n_step, n_therm=n_therm, n_warm=n_warm, shard_start=int(shard_start), vmap=vmap, D=D, G=G, DV=DV,
                      pgroups=pgroups, moves=moves, lmoves=lmoves, width=width, ocoef=ocoef, frows=frows, NG=NG, rho=rho,
                      mc=None if tables is None else (kF, beta, lam), coef=coef, gamma=gamma, gamma_rel=gamma_rel, wgroups=wgroups,
                      dmap=dmap, shift=shift, device=device)


def _chain_warm(p: _ChainPlan, func_or_handle, tables, lo, hi, kF, beta, lam, *, n_warm_sample, alpha, floor, seed, fixed, polar,
                specialize_fused, n_total, shard_start, reduce) -> None:
    """The map's training: ``p.n_warm`` iterations of the direct driver that takes the chain's keywords, on a Philox key of its own;
    without a warm-up, the fused kernel's specialisation that such a driver would have asked for."""
    if p.n_warm:
        kw = dict(n_iter=p.n_warm, n_grid=p.G, alpha=alpha, seed=(int(seed) + _CHAIN_TRAIN_KEY) & 0xFFFFFFFFFFFFFFFF, fixed=fixed,
                  coef=p.coef, device=p.device, vmap=p.vmap, specialize_fused=specialize_fused, reduce=reduce)
        if n_warm_sample is None:
            kw.update(n_sample=p.B, n_total=n_total, shard_start=shard_start)
        else:
            kw.update(n_sample=int(n_warm_sample))
        if polar is not None:
            kw["polar"] = polar
        if p.dmap is not None:
            vegas_integrate_binned(func_or_handle, tables, lo, hi, p.col, p.dmap, kF, beta, lam, floor=floor, groups=p.wgroups, **kw)
        elif (p.wgroups is not None or polar is not None) and tables is None:
            vegas_integrate_stratified(func_or_handle, tables, lo, hi, p.col, Stratification((1,) * p.D), kF, beta, lam, groups=p.wgroups, **kw)
        else:
            if p.wgroups is not None:
                kw["groups"] = p.wgroups
            elif tables is None:
                kw["strat"] = Stratification((1,) * p.D)
            vegas_integrate(func_or_handle, tables, lo, hi, p.col, kF, beta, lam, **kw)
    elif specialize_fused and tables is not None:
        p.handle.specialize_fused(tables)


class _ChainWalkers(namedtuple("_ChainWalkers", "step total n_acc gamma rho keep")):
    """The placed walkers, what :func:`_chain_place` hands to the walk and to the results: ``step(mask, sample_offset, gamma, flags,
    shift_mask=0)`` makes one proposal and one step of every walker; ``total [C + 1, B]`` the walkers' sums and ``n_acc [B]`` their
    acceptances, on the device; ``gamma``; ``rho``: the reweight factors in use; ``keep``: what ``step`` holds
    only addresses of -- the arrays of the groups' descriptor and the walkers' values of the discrete variable."""
    __slots__ = ()


def _chain_place(p: _ChainPlan, st, *, seed, reduce) -> _ChainWalkers:
    """Allocates the walkers' state, places them with FDG_CHAIN_INIT (twice where the reweight factors come from the first placement)
    and takes ``gamma`` from the placed weights unless it was given.  ``step`` is the one place that issues a proposal and a step."""
    import torch
    handle, vmap, dmap, wgroups, coef, rho, gamma = p.handle, p.vmap, p.dmap, p.wgroups, p.coef, p.rho, p.gamma
    R, B, N, D, DV = p.R, p.B, p.N, p.D, p.DV
    all_mask = (1 << D) - 1
    f64 = dict(dtype=torch.float64, device=p.device)
    x = _state(p.fx, B, p.device)
    xp = torch.empty_like(x)
    fac, facp = torch.ones((DV, B), **f64), torch.empty((DV, B), **f64)          # (row D: the discrete variable's 1 / p_j)
    bins = binp = None
    if dmap is not None:
        bins, binp = (torch.zeros(B, dtype=torch.int32, device=p.device) for _ in range(2))
    dv = _discrete(dmap, 0, bins, binp)
    root, a = torch.zeros((R, B), **f64), torch.zeros(B, **f64)
    total = torch.zeros((p.C + 1, B), **f64)
    n_acc = torch.zeros(B, dtype=torch.int32, device=p.device)

    def step(mask, off, g, flags, lmask=0):
        grid = (vmap.d_grid.data_ptr(), D, p.G, p.col, p.n_col)
        walk = (seed, off, x.data_ptr(), B, fac.data_ptr(), xp.data_ptr(), B, facp.data_ptr())
        disc = (bool((mask >> D) & 1), dv.d_cdf, dv.n_bin, dv.d_ext, dv.ext_col, dv.d_bin, dv.d_binp)
        if p.shift is not None:
            capi.chain_propose_device_local(*grid, mask & all_mask, lmask, p.width, *walk, *disc, p.pgroups or (), B, st)
        elif p.pgroups is not None:
            capi.chain_propose_device_polar(*grid, mask & all_mask, *walk, *disc, p.pgroups, B, st)
        elif dmap is None:
            capi.chain_propose_device(*grid, mask, *walk, B, st)
        else:
            capi.chain_propose_device_discrete(*grid, mask & all_mask, *walk, *disc, B, st)
        handle._chain_step(p.entry, p.mc, xp.data_ptr(), B, facp.data_ptr(), p.n_col, D, coef, g, seed, off, flags, x.data_ptr(), B,
                           fac.data_ptr(), root.data_ptr(), a.data_ptr(), total.data_ptr(), n_acc.data_ptr(), B, st, p.desc, gdesc,
                           None if dmap is None else (dv.n_bin, dv.d_binp, dv.d_bin))

    gdesc = gkeep = None
    if wgroups is not None:
        gdesc, gkeep = capi.make_chain_groups(wgroups.root_group, wgroups.var_sets, rho)
    place = (1 << DV) - 1                                                            # every variable, the discrete one too
    step(place, p.shard_start, 1.0, capi.FDG_CHAIN_INIT)                             # (gamma enters no result of the placement)
    if wgroups is not None and rho is None:
        # rho_g = 1 / mean_b |jac_g s_g| of the placement, then the placement again on the same counters with rho
        from .nodetable import FDG_NO_ROOT
        members = [[k for k in range(R) if int(handle.table.root_slot[k]) != FDG_NO_ROOT and int(wgroups.root_group[k]) == g]
                   for g in range(p.NG)]
        sg = torch.zeros(p.NG, **f64)
        for g, ks in enumerate(members):
            if ks:
                c = torch.ones(len(ks), **f64) if coef is None else torch.as_tensor(np.asarray(coef, dtype=np.float64)[ks], **f64)
                jg = fac[sorted(set(int(d) for d in wgroups.var_sets[g]))].prod(0)       # (an empty set: 1)
                if dmap is not None:
                    jg = jg * fac[D]
                sg[g] = (jg * (c[:, None] * root[ks]).sum(0)).abs().sum()
        if reduce is not None:
            reduce(sg)
        mean_g = sg.cpu().numpy() / N
        rho = np.ones(p.NG)
        for g, ks in enumerate(members):
            if ks:
                if not (math.isfinite(mean_g[g]) and mean_g[g] > 0.0 and math.isfinite(1.0 / mean_g[g])):
                    raise ValueError(f"the map's estimate of the integral of |s_g| of group {g} is not positive and finite: pass reweight")
                rho[g] = 1.0 / mean_g[g]
        gdesc, gkeep = capi.make_chain_groups(wgroups.root_group, wgroups.var_sets, rho)
        step(place, p.shard_start, 1.0, capi.FDG_CHAIN_INIT)
    if gamma is None:
        sa = a.sum().reshape(1)
        if reduce is not None:
            reduce(sa)
        gamma = float(p.gamma_rel) * float(sa.item()) / N
        if not (math.isfinite(gamma) and gamma > 0.0):
            raise ValueError("the map's estimate of the integral of |s| is not positive: pass gamma")
    n_acc.zero_()
    return _ChainWalkers(step, total, n_acc, float(gamma), rho, (gkeep, bins, binp))      # (``step`` holds ``dv``'s addresses, not the tensors)


def _chain_walk(p: _ChainPlan, w: _ChainWalkers, *, reduce) -> None:
    """The ``n_step`` steps, measuring from ``n_therm`` on; with ``shift.tune`` the widths ``p.width`` move in the discarded steps."""
    import torch
    shift, moves, lmoves, N = p.shift, p.moves, p.lmoves, p.N

    def accepted():                                       # the acceptances of all walkers so far: an integer, exact in fp64
        s = w.n_acc.sum(dtype=torch.float64).reshape(1)
        if reduce is not None:
            reduce(s)
        return float(s.item())

    for t in range(p.n_step):
        i = t % len(moves)
        lm = 0 if lmoves is None else lmoves[i]
        # tuning, in the discarded steps only: after a move that shifts exactly one variable and does nothing else
        tuned = shift is not None and shift.tune and t < p.n_therm and moves[i] == 0 and lm != 0 and lm & (lm - 1) == 0
        before = accepted() if tuned else 0.0
        w.step(moves[i], (t + 1) * N + p.shard_start, w.gamma, capi.FDG_CHAIN_MEASURE if t >= p.n_therm else 0, lm)
        if tuned:
            d = lm.bit_length() - 1
            p.width[d] = chain_tune_width(float(p.width[d]), accepted() - before, N, float(shift.target))


def _observable_estimates(sums: np.ndarray, M: int, N: int):
    """:func:`chain_estimate_observables` on every block of raw sums ``[blocks, V]`` of ``M`` rows: ``(mean [blocks, M],
    cov [blocks, M, M], stderr [blocks, M])``."""
    est = [chain_estimate_observables(v[:M + 1], v[M + 1:], N) for v in sums]
    return np.stack([m for m, _ in est]), np.stack([c for _, c in est]), np.sqrt(np.stack([np.diag(c) for _, c in est]))


def _chain_results(p: _ChainPlan, w: _ChainWalkers, st, *, reduce, keep_sums) -> ChainResult:
    """The reduction of the walkers' sums, one observables call per block of them behind it on its stream, and the estimates."""
    import torch
    R, F, C, B, N = p.R, p.F, p.C, p.B, p.N
    f64 = dict(dtype=torch.float64, device=p.device)
    out = torch.zeros(3 * C + 2, **f64)
    capi.chain_reduce_device(w.total.data_ptr(), C, B, out.data_ptr(), st)
    acc_sum = w.n_acc.sum(dtype=torch.float64).reshape(1)
    if reduce is not None:
        reduce(out)
        reduce(acc_sum)

    def block_sums(rows, n_block):                         # the raw sums of ``rows`` over each of the windows of their width
        M, width = rows.shape
        sums = torch.zeros((n_block, (M + 1) + (M + 1) * (M + 2) // 2), **f64)
        for j in range(n_block):
            capi.chain_reduce_observables_device(w.total.data_ptr(), B, j * width, width, C, rows, sums[j].data_ptr(), work.data_ptr(), st)
        if reduce is not None:
            reduce(sums)
        return sums

    NB = max(p.n_bin, 1)
    rows = [c for c in (p.ocoef, p.frows) if c is not None]
    if rows:
        work = torch.empty(max(capi.chain_reduce_observables_work_bytes(*c.shape) for c in rows), dtype=torch.uint8, device=p.device)
    osum = None if p.ocoef is None else block_sums(p.ocoef, NB)
    fsum = None if p.frows is None else block_sums(p.frows, NB * F)
    h = out.cpu().numpy()
    osum, fsum = (None if v is None else v.cpu().numpy() for v in (osum, fsum))
    S, Q, X = h[:C + 1].copy(), h[C + 1:2 * C + 2].copy(), h[2 * C + 2:].copy()
    mean, err = chain_estimate(S, Q, X, N)                # (a root that does not exist has sums of 0: mean 0, stderr 0)
    if F:
        mean, err = chain_complex(mean, NB * F, R), chain_complex(err, NB * F, R)
    if p.dmap is not None:
        mean, err = (v.reshape((p.n_bin, F, R) if F else (p.n_bin, R)) for v in (mean, err))
    res = (ChainResult if osum is None and fsum is None else ChainObservablesResult)(
        mean, err, float(acc_sum.item()) / (N * p.n_step), w.gamma, p.vmap, S, Q, X, shift_width=None if p.width is None else p.width.copy(),
        reweight=w.rho)
    if keep_sums:
        res.walker_sums = w.total
    lead = (p.n_bin,) if p.dmap is not None else ()
    if osum is not None:
        Mo = p.ocoef.shape[0]
        m, c, e = _observable_estimates(osum, Mo, N)
        res.obs_mean, res.obs_cov, res.obs_stderr = m.reshape(lead + (Mo,)), c.reshape(lead + (Mo, Mo)), e.reshape(lead + (Mo,))
        res.obs_sums = osum.reshape(lead + osum.shape[1:])
    if fsum is not None:
        Mf = p.frows.shape[0]
        m, c, e = _observable_estimates(fsum, Mf, N)
        res.fobs_mean, res.fobs_stderr = (complex_components(v).reshape(lead + (F, Mf // 2)) for v in (m, e))
        res.fobs_cov = c.reshape(lead + (F, Mf, Mf))
        res.fobs_sums = fsum.reshape(lead + (F,) + fsum.shape[1:])
    return res


def _chain(func_or_handle, tables, lo, hi, col, kF, beta, lam, *, n_warm_sample, alpha, seed, fixed, specialize_fused, n_total, shard_start, reduce,
           floor=0.05, polar=None, keep_sums=False, **plan) -> ChainResult:
    """The body of :func:`chain_integrate`, with ``wgroups`` of :func:`chain_integrate_grouped`, with ``dmap`` of
    :func:`chain_integrate_binned`, with ``polar`` of :func:`chain_integrate_polar`, with ``shift`` of
    :func:`chain_integrate_shift` (the moves are then its pairs, and ``moves`` is None), and with ``observables`` /
    ``freq_observables`` of :func:`chain_integrate_observables` (calls behind the reduction; without them none is made).
    Five stages: the plan, the warm-up, the placement, the walk, the results.  ``plan``: the keywords that only :func:`_chain_plan`
    reads, which names them; the ones spelled out here are read by a later stage too."""
    import torch
    p = _chain_plan(func_or_handle, tables, lo, hi, col, kF, beta, lam, fixed=fixed, n_total=n_total, shard_start=shard_start, polar=polar, **plan)
    _chain_warm(p, func_or_handle, tables, lo, hi, kF, beta, lam, n_warm_sample=n_warm_sample, alpha=alpha, floor=floor, seed=seed, fixed=fixed,
                polar=polar, specialize_fused=specialize_fused, n_total=n_total, shard_start=shard_start, reduce=reduce)
    with torch.cuda.device(p.device):
        st = torch.cuda.current_stream(p.device).cuda_stream
        w = _chain_place(p, st, seed=seed, reduce=reduce)
        _chain_walk(p, w, reduce=reduce)
        return _chain_results(p, w, st, reduce=reduce, keep_sums=keep_sums)
