// Markov-chain sampling on the VEGAS map (include/fdg.h: fdg_chain_propose_device, fdg_chain_step_device, fdg_mc_chain_step_device,
// fdg_chain_reduce_device).  One walker per lane, every access with sample stride 1.  A step is: propose (redraw the
// variables of a mask through the map, copy the rest), evaluate the proposals chunk by chunk into the handle's root scratch by the
// route of fdg_eval_device / fdg_mc_eval_device, then fdg_chain_select per chunk: fold, accept rule, selection, measurement.  No
// kernel here holds a per-lane array: the select kernel walks the root columns twice (fold, then select), the variables' factors
// likewise, so n_root = 180 and n_dim = 64 cost loads, not registers.  Nothing here touches the kernels of fdg_binned.hip: the
// proposal calls the sampler's own statements of one variable, of the discrete pick and of the polar point (fdg_sampler.h), so the bits are its.
//
// All step entries run the one select kernel fdg_chain_select<MZ, BIN>.  It gives every group of roots the jacobian of its own
// variables and a reweight factor: a' = sum_g rho_g |jac_g s_g| (fdg_[mc_]chain_step_device_grouped).  It walks the
// groups outside and a group's roots inside: the lists of the roots are uploaded sorted by (group, root), so a group is one contiguous
// range, and the groups' ranges, masks and factors are a kernel argument by value (ChainGroups).  jac_g is one pass over the group's
// variables, made anew for every group: a product per group in a register, not an array of them.  A call without groups is one
// group of every live root and every variable without a factor, built on the host: a' = |jac' s'|, the same bits.
//
// With MZ (fdg_[mc_]chain_step_device_matsubara, or a grouped call with a projection) a group's roots are folded with
// the phase of the weight frequency (s_g = sum_k c_k r_k e^{i w tau_k}) and every root is measured at every frequency.  Roots
// outside, frequencies inside, x = tau / beta once per root; the phase is fdg_matsubara.h's, so a numpy restatement gives the same
// bits.
//
// With BIN (fdg_chain_propose_device_discrete, fdg_[mc_]chain_step_device_binned) the walker carries one discrete
// variable behind the continuous ones: its value in bin / binp, its factor 1 / p_j in row n_dim of fac / facp.  Every group's jacobian
// takes that factor as its last product, and a walker measures into the columns of its own bin through a row address of its own:
// no loop over the bins, nothing multiplied by zero, every word still one lane's.
//
// Local moves (fdg_chain_propose_device_local) are a matter of the proposal alone: in the map's uniform coordinate y the
// stationary density is a + gamma, so the select kernel's rule is the Metropolis rule of every proposal that is symmetric in y, and
// a shift y' = y + t h (mod 1) is one.  The proposal kernel has an instance that shifts; no step, select or reduce kernel changes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

#define FDG_RUNTIME_TU 1
#include "fdg_internal.h"
#include "fdg_matsubara.h"
#include "fdg_sampler.h"

using namespace fdg;

namespace {

// The groups of a step (a kernel argument, by value): the live roots of group g are the entries start[g] .. start[g + 1] - 1
// of the sorted lists, mask[g] its variables, rho[g] its reweight factor (read only where the call has one).
struct ChainGroups {
  uint32_t n;
  uint32_t start[FDG_WEIGHT_GROUP_MAX + 1];
  uint64_t mask[FDG_WEIGHT_GROUP_MAX];
  double rho[FDG_WEIGHT_GROUP_MAX];
};

// The discrete variable of a proposal (a kernel argument, by value; only the instances with one take it): move = redraw it, cdf and
// the table ext [n_bin][n_ext] with its columns as the VEGAS sampler takes them, bin / binp its value in the state / the proposal.
struct ChainDiscArgs {
  uint32_t move;
  const double *cdf;
  uint32_t n_bin;
  const double *ext;
  uint32_t n_ext;
  SamplerExtCols ecol;
  const int32_t *bin;
  int32_t *binp;
};

// The shifted variables of a proposal (a kernel argument, by value; only the instances with one take it): mask = the variables moved by
// a shift in the map's coordinate, hG[d] = width[d] * n_grid the half width of variable d's shift in cells.
struct ChainLocalArgs {
  uint64_t mask;
  double hG[FDG_VEGAS_DIM_MAX];
};

// xp, facp = the proposal of every walker, one lane per walker: the variables of `mask` redrawn through the map (vegas_draw, the
// sampler's statements: the counter is the walker's global index), everything else copied from x, fac.  A redrawn variable's column is
// first copied and then overwritten by the same lane, in program order.
// POLAR: groups of variables read as (k, phi) or (k, theta, phi).  The ungrouped variables first; then group by group,
// in the order of the array.  A group moves whole or not at all (the host has refused a mask that names part of one: the bit of its
// first variable decides): moved, its two or three values are drawn on their own counters, stay in registers, and give the group's
// columns and the measure's factors, each factor in the row of its own variable
//     3D:  facp[var] = ((G wd_k) k) k,  facp[var + 1] = (G wd_theta) sin(theta),  facp[var + 2] = G wd_phi
//     2D:  facp[var] = (G wd_k) k,      facp[var + 1] = G wd_phi
// so that the select kernel's left fold over a mask is the jacobian of the polar measure with no change to it; kept, its rows of fac
// are copied (its columns were copied with all the others).  No per-lane array, no LDS: everything indexed by g is wave-uniform.
// DISC: the discrete variable behind the D continuous ones, fac and facp have the row D.  move: its value j by
// discrete_pick, row j of ext to the columns ecol and 1 / p_j to row D of facp; otherwise the value and its factor are copied (the
// columns ecol were copied with all the others).
// LOCAL: a variable of no group whose bit is set in loc.mask, and not in mask, is SHIFTED in the map's coordinate
// (vegas_shift: the inverse of the map at the state's value, y' = y + t h mod 1, the map again), on the Philox column a redraw of it
// would use.  loc.hG[d] = width[d] * G is read only for those variables; d is wave-uniform, so it is a scalar load of the argument.
// The discrete variable and the polar groups are only ever redrawn: the state holds Cartesian columns and no (k, theta, phi).
template <bool POLAR, bool DISC, bool LOCAL>
__global__ void __launch_bounds__(256)
fdg_chain_propose(const double *__restrict__ grid, uint32_t D, uint32_t G, SamplerCols col, uint32_t n_col, uint64_t mask, uint64_t seed,
                  uint64_t off, const double *__restrict__ x, long xc, const double *__restrict__ fac, double *__restrict__ xp, long xpc,
                  double *__restrict__ facp, long n, ArgIf<POLAR, SamplerPolar> pol, ArgIf<DISC, ChainDiscArgs> da,
                  ArgIf<LOCAL, ChainLocalArgs> loc) {
  const long b = blockIdx.x * 256L + threadIdx.x;
  if (b >= n) return;
  const uint64_t sample = off + (uint64_t)b;
  for (uint32_t c = 0; c < n_col; ++c) xp[(long)c * xpc + b] = x[(long)c * xc + b];
  for (uint32_t d = 0; d < D; ++d) {
    if constexpr (POLAR) {
      if ((pol.grouped >> d) & 1u) continue;
    }
    const size_t at = (size_t)d * (size_t)n + (size_t)b;
    if ((mask >> d) & 1u) {
      uint32_t c;
      double f;
      const double v = vegas_draw(grid, d, G, sample, seed, 0, 1, c, f);
      xp[(long)col.c[d] * xpc + b] = v;
      facp[at] = f;
    } else {
      if constexpr (LOCAL) {
        if ((loc.mask >> d) & 1u) {
          double f;
          const double v = vegas_shift(grid, d, G, sample, seed, loc.hG[d], x[(long)col.c[d] * xc + b], f);
          xp[(long)col.c[d] * xpc + b] = v;
          facp[at] = f;
          continue;
        }
      }
      facp[at] = fac[at];
    }
  }
  if constexpr (POLAR) {
    for (uint32_t g = 0; g < pol.n; ++g) {
      const uint32_t var = pol.var[g];
      const bool three = pol.dim[g] == 3;
      const size_t at = (size_t)var * (size_t)n + (size_t)b;
      if (!((mask >> var) & 1u)) {
        facp[at] = fac[at];
        facp[at + (size_t)n] = fac[at + (size_t)n];
        if (three) facp[at + 2u * (size_t)n] = fac[at + 2u * (size_t)n];
        continue;
      }
      uint32_t c;
      double fk, fa, fp = 0.0;
      const double k = vegas_draw(grid, var, G, sample, seed, 0, 1, c, fk);
      const double va = vegas_draw(grid, var + 1u, G, sample, seed, 0, 1, c, fa);      // theta, or phi in two dimensions
      const double vp = three ? vegas_draw(grid, var + 2u, G, sample, seed, 0, 1, c, fp) : va;
      double c0, c1, c2, st;
      polar_point(three, k, va, vp, c0, c1, c2, st);
      xp[(long)pol.col[g][0] * xpc + b] = c0;
      xp[(long)pol.col[g][1] * xpc + b] = c1;
      if (three) xp[(long)pol.col[g][2] * xpc + b] = c2;
      double f0 = fk * k;
      if (three) f0 = f0 * k;
      facp[at] = f0;
      facp[at + (size_t)n] = three ? fa * st : fa;
      if (three) facp[at + 2u * (size_t)n] = fp;
    }
  }
  if constexpr (DISC) {
    const size_t at = (size_t)D * (size_t)n + (size_t)b;
    if (da.move) {
      double p;
      const uint32_t j = discrete_pick(da.cdf, da.n_bin, sample, D, seed, p);
      da.binp[b] = (int32_t)j;
      for (uint32_t e = 0; e < da.n_ext; ++e) xp[(long)da.ecol.c[e] * xpc + b] = da.ext[(size_t)j * da.n_ext + e];
      facp[at] = 1.0 / p;
    } else {
      da.binp[b] = da.bin[b];
      facp[at] = fac[at];
    }
  }
}

// The jacobian of one group for walker b: the left fold of f[d][b] over ascending d with bit d in mask; an empty mask gives 1.0.
__device__ __forceinline__ double chain_group_jac(const double *__restrict__ f, uint64_t mask, uint32_t D, long nw, long b) {
  double j = 1.0;
  bool first = true;
  for (uint32_t d = 0; d < D; ++d) {
    if (!((mask >> d) & 1u)) continue;
    const double v = f[(size_t)d * (size_t)nw + (size_t)b];
    j = first ? v : j * v;
    first = false;
  }
  return j;
}

// One chunk of n walkers whose proposals' roots lie column-major in `roots` (leading dimension ld).  Every array pointer is already
// moved to the chunk's first walker; nw = n_walker is the column stride of fac, root and sum; off = sample_offset + the chunk's start.
// kidx are the roots that exist, cf their factors (null: 1), both sorted by (group, root); a group without a live root is skipped
// altogether.  Without MZ sum is [R + 1][nw], column k root k's, the last one d, and the arguments of the projection are not read.
// With MZ cin[j], cout[j] are the columns of xp / x that hold the two times of live root j, mult[f] the multiplier of frequency f
// (matsubara_multiplier, formed on the host), wf the frequency of the weight, and sum is [2 F R + 1][nw]: column 2 (f R + k) the real
// part of root k at frequency f, the next one the imaginary part, the last one d.  Everything indexed by g, j or f is wave-uniform;
// the only per-lane values that live across a group are ap and bad.
// With BIN fac and facp have the row D (the discrete variable's factor: the last product of every jac_g), binp / bin hold the value of
// the proposal / the state, and sum is [n_bin R + 1][nw] or [2 n_bin F R + 1][nw]: the walker's columns are those of its bin j, root k
// at j R + k, or at 2 ((j F + f) R + k).  A bin outside [0, n_bin), which the proposal never writes, measures nothing.
template <bool MZ, bool BIN>
__global__ void __launch_bounds__(256)
fdg_chain_select(const double *__restrict__ roots, long ld, long n, const uint32_t *__restrict__ kidx, const double *__restrict__ cf,
                 ChainGroups cg, uint32_t has_rho, const uint32_t *__restrict__ cin, const uint32_t *__restrict__ cout,
                 const double *__restrict__ mult, uint32_t F, uint32_t wf, double beta, const double *__restrict__ xp, long xpc,
                 const double *__restrict__ facp, uint32_t n_col, uint32_t D, long nw, double gamma, uint64_t seed, uint64_t off,
                 uint32_t flags, double *__restrict__ x, long xc, double *__restrict__ fac, double *__restrict__ root,
                 double *__restrict__ a, double *__restrict__ sum, uint32_t R, int32_t *__restrict__ n_accept, uint32_t n_bin,
                 const int32_t *__restrict__ binp, int32_t *__restrict__ bin) {
  const long b = blockIdx.x * 256L + threadIdx.x;
  if (b >= n) return;
  const bool init = (flags & FDG_CHAIN_INIT) != 0, meas = (flags & FDG_CHAIN_MEASURE) != 0;
  // the fold, group by group: jac_g', s_g' (or re_g', im_g' at the weight frequency), a_g', and a' = the fold of rho_g a_g'
  double mw = 0.0;
  if (MZ) mw = mult[wf];
  double asum = 0.0;
  bool bad = false, first_group = true;
  double fdp = 1.0;
  if (BIN) fdp = facp[(size_t)D * (size_t)nw + (size_t)b];
  for (uint32_t g = 0; g < cg.n; ++g) {
    const uint32_t j0 = cg.start[g], j1 = cg.start[g + 1];
    if (j0 == j1) continue;
    double jg = chain_group_jac(facp, cg.mask[g], D, nw, b);
    if (BIN) jg = jg * fdp;
    double ag;
    if (MZ) {
      double re = 0.0, im = 0.0;
      for (uint32_t j = j0; j < j1; ++j) {
        const double r = roots[(size_t)kidx[j] * (size_t)ld + (size_t)b];
        bad = bad || !std::isfinite(r);
        const double tau = xp[(long)cout[j] * xpc + b] - xp[(long)cin[j] * xpc + b];
        const double xt = tau / beta;
        double sn, cs;
        matsubara_phase_of(xt, mw, sn, cs);
        const double term = cf ? cf[j] * r : r;
        const double pr = term * cs, pi = term * sn;
        re = j != j0 ? re + pr : pr;
        im = j != j0 ? im + pi : pi;
      }
      const double tre = jg * re, tim = jg * im;
      bad = bad || !std::isfinite(tre) || !std::isfinite(tim);
      const double q0 = tre * tre, q1 = tim * tim;
      const double q = q0 + q1;
      bad = bad || !std::isfinite(q);
      ag = sqrt(q);
    } else {
      double s = 0.0;
      for (uint32_t j = j0; j < j1; ++j) {
        const double r = roots[(size_t)kidx[j] * (size_t)ld + (size_t)b];
        bad = bad || !std::isfinite(r);
        const double term = cf ? cf[j] * r : r;
        s = j != j0 ? s + term : term;
      }
      const double tg = jg * s;
      bad = bad || !std::isfinite(tg);
      ag = fabs(tg);
    }
    const double wa = has_rho ? cg.rho[g] * ag : ag;
    asum = first_group ? wa : asum + wa;
    first_group = false;
  }
  bad = bad || !std::isfinite(asum);
  const double ap = bad ? 0.0 : asum;
  // the accept rule
  const double a0 = init ? 0.0 : a[b];
  bool acc = true;
  if (!init) {
    const double u = fdg_philox_u53(off + (uint64_t)b, FDG_VEGAS_DIM_MAX, seed);
    acc = u * (a0 + gamma) < (ap + gamma);
  }
  // the selection
  if (acc) {
    for (uint32_t c = 0; c < n_col; ++c) x[(long)c * xc + b] = xp[(long)c * xpc + b];
    for (uint32_t d = 0; d < D; ++d) {
      const size_t at = (size_t)d * (size_t)nw + (size_t)b;
      fac[at] = facp[at];
    }
    if (BIN) {
      const size_t at = (size_t)D * (size_t)nw + (size_t)b;
      fac[at] = facp[at];
      bin[b] = binp[b];
    }
    a[b] = ap;
    if (n_accept) n_accept[b] = n_accept[b] + 1;
  }
  if (!acc && !meas) return;
  // the second walk over the groups and their roots: select, and measure on the state after the selection (whose factors and times
  // are the proposal's after an acceptance: the same bits, read where they were not just written)
  const double dd = 1.0 / ((acc ? ap : a0) + gamma);
  const double *fs = acc ? facp : fac;
  const double *tp = acc ? xp : x;
  const long tpc = acc ? xpc : xc;
  uint32_t jb = 0;
  double fds = 1.0;
  bool jin = true;
  if (BIN && meas) {
    jb = (uint32_t)(acc ? binp[b] : bin[b]);
    jin = jb < n_bin;
    fds = fs[(size_t)D * (size_t)nw + (size_t)b];
  }
  for (uint32_t g = 0; g < cg.n; ++g) {
    const uint32_t j0 = cg.start[g], j1 = cg.start[g + 1];
    if (j0 == j1) continue;
    double jac = 0.0;
    if (meas) jac = chain_group_jac(fs, cg.mask[g], D, nw, b);
    if (BIN && meas) jac = jac * fds;
    for (uint32_t j = j0; j < j1; ++j) {
      const uint32_t k = kidx[j];
      const size_t at = (size_t)k * (size_t)nw + (size_t)b;
      double r;
      if (acc) {
        const double rp = roots[(size_t)k * (size_t)ld + (size_t)b];
        r = bad ? 0.0 : rp;
        root[at] = r;
      } else {
        r = root[at];
      }
      if (meas && (!BIN || jin)) {
        const double jr = jac * r;
        const double w = jr * dd;
        if (MZ) {
          const double tau = tp[(long)cout[j] * tpc + b] - tp[(long)cin[j] * tpc + b];
          const double xt = tau / beta;
          for (uint32_t f = 0; f < F; ++f) {
            double sn, cs;
            matsubara_phase_of(xt, mult[f], sn, cs);
            const size_t o = (size_t)(2u * ((BIN ? jb * F + f : f) * R + k)) * (size_t)nw + (size_t)b;
            sum[o] = sum[o] + w * cs;
            sum[o + (size_t)nw] = sum[o + (size_t)nw] + w * sn;
          }
        } else if (BIN) {
          const size_t o = ((size_t)jb * R + k) * (size_t)nw + (size_t)b;
          sum[o] = sum[o] + w;
        } else {
          sum[at] = sum[at] + w;
        }
      }
    }
  }
  if (meas && (!BIN || jin)) {
    const size_t at = (size_t)((BIN ? n_bin : 1u) * (MZ ? 2u * F * R : R)) * (size_t)nw + (size_t)b;
    sum[at] = sum[at] + dd;
  }
}

// out[c] += the sum over the walkers of column c's term (include/fdg.h: S, Q, X); one workgroup per output.
__global__ void __launch_bounds__(256)
fdg_chain_reduce(const double *__restrict__ sum, uint32_t R, long n, double *__restrict__ out) {
  __shared__ double sh[256];
  const uint32_t c = blockIdx.x;
  const double *p, *q;                                     // the term of walker b is p[b] * q[b], or p[b] where q is null
  if (c <= R) { p = sum + (size_t)c * (size_t)n; q = nullptr; }
  else if (c <= 2u * R + 1u) { p = q = sum + (size_t)(c - R - 1u) * (size_t)n; }
  else { p = sum + (size_t)(c - 2u * R - 2u) * (size_t)n; q = sum + (size_t)R * (size_t)n; }
  double t = 0.0;
  for (long b = threadIdx.x; b < n; b += 256) {
    const double v = p[b];
    t = t + (q ? v * q[b] : v);
  }
  sh[threadIdx.x] = t;
  __syncthreads();
  for (uint32_t h = 128; h; h >>= 1) {
    if (threadIdx.x < h) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = out[c] + sh[0];
}

constexpr size_t page_up(size_t bytes) { return (bytes + 4095) & ~(size_t)4095; }

struct ChainCall {
  const double *d_xp;
  int64_t xpc;
  const double *d_facp;
  uint32_t n_col, n_dim;
  const double *coef;
  double gamma;
  uint64_t seed, offset;
  unsigned flags;
  double *d_x;
  int64_t xc;
  double *d_fac, *d_root, *d_a, *d_sum;
  int32_t *d_n_accept;
  int64_t B;
  void *stream;
  uint32_t n_bin = 0;                                      // the binned step: the discrete variable's values, 0 for every other entry
  const int32_t *d_binp = nullptr;
  int32_t *d_bin = nullptr;
};

// The checks of both step calls that need no lock.
int check_chain(const fdg_graph *g, const ChainCall &c) {
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  if (c.B < 0) { set_error("n_walker < 0"); return FDG_E_INVALID; }
  if (c.flags & ~(FDG_CHAIN_INIT | FDG_CHAIN_MEASURE)) { set_error("unknown flags"); return FDG_E_INVALID; }
  const bool meas = (c.flags & FDG_CHAIN_MEASURE) != 0;
  if (!c.d_xp || !c.d_facp || !c.d_x || !c.d_fac || !c.d_root || !c.d_a || (meas && !c.d_sum)) { set_error("null device buffer"); return FDG_E_INVALID; }
  const void *arr[7] = {c.d_x, c.d_fac, c.d_root, c.d_a, c.d_sum, c.d_xp, c.d_facp};
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < i; ++j)
      if (arr[i] && arr[i] == arr[j]) { set_error("two of the state, proposal and sum arrays are the same buffer"); return FDG_E_INVALID; }
  if ((const void *)c.d_n_accept && std::find(arr, arr + 7, (const void *)c.d_n_accept) != arr + 7) {
    set_error("d_n_accept is the same buffer as another array"); return FDG_E_INVALID;
  }
  if (!(std::isfinite(c.gamma) && c.gamma > 0.0)) { set_error("gamma must be finite and > 0"); return FDG_E_INVALID; }
  if (c.n_dim == 0) { set_error("n_dim == 0"); return FDG_E_INVALID; }
  if (c.n_dim > FDG_VEGAS_DIM_MAX) { set_error("n_dim > FDG_VEGAS_DIM_MAX"); return FDG_E_UNSUPPORTED; }
  if (c.xc < c.B || c.xpc < c.B) { set_error("a column stride < n_walker"); return FDG_E_INVALID; }
  if (c.coef)
    for (uint32_t k = 0; k < g->prog.R; ++k)
      if (!std::isfinite(c.coef[k])) { set_error("a coefficient is not finite"); return FDG_E_INVALID; }
  return FDG_OK;
}

// The checks of the projected step calls on their descriptor, after check_chain.
int check_chain_mz(const fdg_graph *g, const ChainCall &c, const fdg_chain_matsubara *mz) {
  if (!mz) { set_error("null Matsubara descriptor"); return FDG_E_INVALID; }
  if (!mz->freq || !mz->root_col_in || !mz->root_col_out) { set_error("null array in the Matsubara descriptor"); return FDG_E_INVALID; }
  if (mz->n_freq == 0) { set_error("n_freq == 0"); return FDG_E_INVALID; }
  if (mz->n_freq > FDG_MATSUBARA_FREQ_MAX) { set_error("n_freq > FDG_MATSUBARA_FREQ_MAX"); return FDG_E_UNSUPPORTED; }
  if (mz->weight_freq >= mz->n_freq) { set_error("weight_freq >= n_freq"); return FDG_E_INVALID; }
  if (!(std::isfinite(mz->beta) && mz->beta > 0.0)) { set_error("beta must be finite and > 0"); return FDG_E_INVALID; }
  for (uint32_t k = 0; k < g->prog.R; ++k)
    if (g->prog.root_slot[k] != FDG_NO_ROOT && (mz->root_col_in[k] >= c.n_col || mz->root_col_out[k] >= c.n_col)) {
      set_error("a time column of an existing root >= n_col"); return FDG_E_INVALID;
    }
  return FDG_OK;
}

// The checks of the grouped step calls on their descriptor, after check_chain (and check_chain_mz where there is a projection).
int check_chain_groups(const fdg_graph *g, const ChainCall &c, const fdg_chain_groups *cg) {
  if (!cg) { set_error("null groups descriptor"); return FDG_E_INVALID; }
  if (!cg->root_group || !cg->var_mask) { set_error("null array in the groups descriptor"); return FDG_E_INVALID; }
  if (cg->n_group == 0) { set_error("n_group == 0"); return FDG_E_INVALID; }
  if (cg->n_group > FDG_WEIGHT_GROUP_MAX) { set_error("n_group > FDG_WEIGHT_GROUP_MAX"); return FDG_E_UNSUPPORTED; }
  for (uint32_t k = 0; k < g->prog.R; ++k)
    if (g->prog.root_slot[k] != FDG_NO_ROOT && cg->root_group[k] >= cg->n_group) {
      set_error("root_group of an existing root >= n_group"); return FDG_E_INVALID;
    }
  for (uint32_t q = 0; q < cg->n_group; ++q) {
    if (c.n_dim < 64 && (cg->var_mask[q] >> c.n_dim)) { set_error("var_mask names a variable >= n_dim"); return FDG_E_INVALID; }
    if (cg->reweight && !(std::isfinite(cg->reweight[q]) && cg->reweight[q] > 0.0)) {
      set_error("a reweight factor is not finite or <= 0"); return FDG_E_INVALID;
    }
  }
  return FDG_OK;
}

// The checks of the binned step calls on the discrete variable's arguments, after all the others.
int check_chain_binned(const ChainCall &c) {
  if (c.n_bin == 0) { set_error("n_bin == 0"); return FDG_E_INVALID; }
  if (c.n_bin > FDG_CHAIN_BIN_MAX) { set_error("n_bin > FDG_CHAIN_BIN_MAX"); return FDG_E_UNSUPPORTED; }
  if (!c.d_binp || !c.d_bin) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (c.d_binp == c.d_bin) { set_error("d_bin and d_binp are the same buffer"); return FDG_E_INVALID; }
  const void *arr[8] = {c.d_x, c.d_fac, c.d_root, c.d_a, c.d_sum, c.d_xp, c.d_facp, c.d_n_accept};
  for (int i = 0; i < 8; ++i)
    if (arr[i] && (arr[i] == (const void *)c.d_binp || arr[i] == (const void *)c.d_bin)) {
      set_error("d_bin or d_binp is the same buffer as another array"); return FDG_E_INVALID;
    }
  return FDG_OK;
}

struct ChainMc { double kF, beta, lambda; };               // the parameters of the Monte-Carlo form's leaves

// The work of all step calls (caller holds g->mu, stream bound), chunk by chunk: the roots of the proposals column-major into the
// root scratch, by fdg_run_locked or, with mc, fdg_mc_run_locked, then fdg_chain_select.  The chunk is the accumulate calls'
// (FDG_ROOT_SCRATCH_MB); no result depends on it.
// mz: the projected step; its multipliers and time columns lie behind the plain step's uploads.
// cg: the grouped step; the lists are then sorted by (group, root).  Without cg the roots are one group of every variable.
int run_chain(fdg_graph *g, const ChainCall &c, const ChainMc *mc, const fdg_chain_matsubara *mz, const fdg_chain_groups *cg) {
  const uint32_t R = g->prog.R;
  const hipStream_t st = (hipStream_t)c.stream;
  long Bc = std::max<long>(64, (long)((g->cfg.root_scratch_mb << 20) / (8ull * std::max<uint32_t>(R, 1u))) & ~63l);
  Bc = std::min<long>(Bc, (long)((c.B + 63) & ~(int64_t)63));
  const size_t root_bytes = page_up((size_t)Bc * std::max<uint32_t>(R, 1u) * sizeof(double));
  const size_t plain_bytes = page_up((size_t)std::max<uint32_t>(R, 1u) * 12u);
  const size_t mz_bytes = mz ? page_up((size_t)FDG_MATSUBARA_FREQ_MAX * sizeof(double) + (size_t)std::max<uint32_t>(R, 1u) * 8u) : 0;
  int rc = ensure_root_scratch(g, root_bytes + plain_bytes + mz_bytes);
  if (rc) return rc;
  double *roots = (double *)g->d_ws2;
  // the roots that exist, ascending, and their factors: one small upload per call (pageable memory: staged before the call returns)
  double *d_coef = (double *)((char *)g->d_ws2 + root_bytes);
  uint32_t *d_kidx = (uint32_t *)(d_coef + std::max<uint32_t>(R, 1u));
  std::vector<double> hc;
  std::vector<uint32_t> hk;
  for (uint32_t k = 0; k < R; ++k)
    if (g->prog.root_slot[k] != FDG_NO_ROOT) hk.push_back(k);
  ChainGroups grp{};
  if (cg) {
    std::stable_sort(hk.begin(), hk.end(), [&](uint32_t p, uint32_t q) { return cg->root_group[p] < cg->root_group[q]; });
    grp.n = cg->n_group;
    for (uint32_t k : hk) ++grp.start[cg->root_group[k] + 1u];
    for (uint32_t q = 0; q < cg->n_group; ++q) {
      grp.start[q + 1u] += grp.start[q];
      grp.mask[q] = cg->var_mask[q];
      grp.rho[q] = cg->reweight ? cg->reweight[q] : 1.0;
    }
  } else {
    grp.n = 1;
    grp.start[1] = (uint32_t)hk.size();
    grp.mask[0] = c.n_dim < 64 ? (1ull << c.n_dim) - 1ull : ~0ull;
  }
  for (uint32_t k : hk) hc.push_back(c.coef ? c.coef[k] : 1.0);
  const uint32_t n_live = (uint32_t)hk.size();
  if (n_live) {
    HIP_TRY(hipMemcpyAsync(d_coef, hc.data(), n_live * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_kidx, hk.data(), n_live * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  // the projected step: the multiplier of every frequency, then the two time columns of every root that exists; without a
  // projection the kernel reads none of them
  double *d_mult = nullptr;
  uint32_t *d_cin = nullptr, *d_cout = nullptr;
  if (mz) {
    d_mult = (double *)((char *)g->d_ws2 + root_bytes + plain_bytes);
    d_cin = (uint32_t *)(d_mult + FDG_MATSUBARA_FREQ_MAX);
    d_cout = d_cin + std::max<uint32_t>(R, 1u);
    std::vector<double> hm(mz->n_freq);
    std::vector<uint32_t> hin, hout;
    for (uint32_t f = 0; f < mz->n_freq; ++f) hm[f] = matsubara_multiplier(mz->freq[f], mz->fermionic);
    for (uint32_t k : hk) { hin.push_back(mz->root_col_in[k]); hout.push_back(mz->root_col_out[k]); }
    HIP_TRY(hipMemcpyAsync(d_mult, hm.data(), hm.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (n_live) {
      HIP_TRY(hipMemcpyAsync(d_cin, hin.data(), n_live * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_cout, hout.data(), n_live * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
  }
  const auto select = c.n_bin ? (mz ? fdg_chain_select<true, true> : fdg_chain_select<false, true>)
                              : (mz ? fdg_chain_select<true, false> : fdg_chain_select<false, false>);
  for (long c0 = 0; c0 < (long)c.B; c0 += Bc) {
    const long n = std::min<long>(Bc, (long)c.B - c0);
    if (n_live) {
      const double *xp = c.d_xp + c0;
      if (mc) {
        const double *T = xp + (int64_t)(g->lt_hdr[2] * g->lt_hdr[3]) * c.xpc;
        rc = fdg_mc_run_locked(g, 0, xp, 1, c.xpc, T, 1, c.xpc, mc->kF, mc->beta, mc->lambda, roots, 1, Bc, nullptr, nullptr, n, st);
      } else {
        rc = fdg_run_locked(g, 0, xp, 1, c.xpc, roots, 1, Bc, nullptr, nullptr, n, st, 0, 0);
      }
      if (rc) return rc;
    }
    hipLaunchKernelGGL(select, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, roots,
                       Bc, n, d_kidx, c.coef ? d_coef : nullptr, grp, cg && cg->reweight ? 1u : 0u, d_cin, d_cout, d_mult,
                       mz ? mz->n_freq : 0u, mz ? mz->weight_freq : 0u, mz ? mz->beta : 1.0, c.d_xp + c0, (long)c.xpc, c.d_facp + c0,
                       c.n_col, c.n_dim, (long)c.B, c.gamma, c.seed, c.offset + (uint64_t)c0, (uint32_t)c.flags, c.d_x + c0, (long)c.xc,
                       c.d_fac + c0, c.d_root + c0, c.d_a + c0, c.d_sum ? c.d_sum + c0 : nullptr, R,
                       c.d_n_accept ? c.d_n_accept + c0 : nullptr, c.n_bin, c.n_bin ? c.d_binp + c0 : nullptr,
                       c.n_bin ? c.d_bin + c0 : nullptr);
    HIP_TRY(hipGetLastError());
  }
  return FDG_OK;
}

// Which of the four pairs of entries a call came through: what its descriptors may be.
// no descriptor; mz required; cg required, mz optional; both optional (with the discrete variable's arguments in the call)
enum ChainEntry { CHAIN_PLAIN, CHAIN_MATSUBARA, CHAIN_GROUPED, CHAIN_BINNED };

// The body of the eight step entries: the leaf form, or with mc the Monte-Carlo form.  The checks run in this order in every entry,
// so a call that is wrong in two ways is refused with the same message through each of them.
int chain_step(fdg_graph *g, const ChainCall &c, const ChainMc *mc, ChainEntry entry, const fdg_chain_matsubara *mz,
               const fdg_chain_groups *cg) {
  int rc = check_chain(g, c);
  if (rc) return rc;
  if (!mc && c.n_col != g->prog.L) { set_error("n_col is not the graph's number of leaves"); return FDG_E_INVALID; }
  if (mz || entry == CHAIN_MATSUBARA) {
    rc = check_chain_mz(g, c, mz);
    if (rc) return rc;
  }
  if (entry == CHAIN_GROUPED || (entry == CHAIN_BINNED && cg)) {
    rc = check_chain_groups(g, c, cg);
    if (rc) return rc;
  }
  if (entry == CHAIN_BINNED) {
    rc = check_chain_binned(c);
    if (rc) return rc;
  }
  std::lock_guard<std::mutex> lk(g->mu);
  fdg::KnobScope knob_scope(&g->knobs);
  if (mc) {
    if (g->mc_route == 0) { set_error("fdg_graph_specialize_fused has not been called on this handle"); return FDG_E_INVALID; }
    if (c.n_col != g->lt_hdr[2] * g->lt_hdr[3] + g->lt_hdr[4]) { set_error("n_col is not the tables' n_loop * dim + n_tau"); return FDG_E_INVALID; }
  }
  if (c.B == 0) return FDG_OK;
  rc = ensure_device(g);
  if (rc) return rc;
  rc = fdg_bind_stream_ws(g, c.stream);
  if (rc) return rc;
  return run_chain(g, c, mc, mz, cg);
}

// The discrete variable of a propose call as the host takes it; d_cdf null (fdg_chain_propose_device, or the polar entry without
// one): none, and the rest is ignored.  required (fdg_chain_propose_device_discrete): d_cdf null is refused.
struct ChainProposeDiscrete {
  bool required;
  int move;
  const double *d_cdf;
  uint32_t n_bin;
  const double *d_ext;
  uint32_t n_ext;
  const uint32_t *ext_col;
  const int32_t *d_bin;
  int32_t *d_binp;
};

// Every fdg_chain_propose_device* entry: the checks in one order, then the instance of the proposal that reads what the call carries.
// takes_polar (the _polar entry): every written column is to be named once.
int chain_propose(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col, uint64_t mask, uint64_t seed,
                  uint64_t sample_offset, const double *d_x, int64_t x_col_stride, const double *d_fac, double *d_xp, int64_t xp_col_stride,
                  double *d_facp, int64_t B, void *stream, const ChainProposeDiscrete &dv, bool takes_polar, const fdg_vegas_polar *polar,
                  uint32_t n_polar, uint64_t local_mask = 0, const double *width = nullptr) {
  // The groups first, for pol.grouped: the col entry of a grouped variable is not read, and 0 stands in for it in the checks below.
  // A refusal of theirs is returned at its own rank, behind those checks; nothing sets a message in between unless it refuses.
  SamplerPolar pol;
  const int rc_polar = parse_polar(polar, n_polar, n_dim, n_col, pol);
  if (B < 0) { set_error("n_walker < 0"); return FDG_E_INVALID; }
  if (!d_grid || !d_x || !d_fac || !d_xp || !d_facp) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (n_dim == 0 || n_grid == 0) { set_error("n_dim == 0 or n_grid == 0"); return FDG_E_INVALID; }
  if (n_dim > FDG_VEGAS_DIM_MAX) { set_error("n_dim > FDG_VEGAS_DIM_MAX"); return FDG_E_UNSUPPORTED; }
  if (n_grid > FDG_VEGAS_GRID_MAX) { set_error("n_grid > FDG_VEGAS_GRID_MAX"); return FDG_E_UNSUPPORTED; }
  if (d_x == d_xp || d_fac == d_facp) { set_error("the state and the proposal are the same buffer"); return FDG_E_INVALID; }
  if (n_dim < 64 && (mask >> n_dim)) { set_error("mask names a variable >= n_dim"); return FDG_E_INVALID; }
  if (x_col_stride < B || xp_col_stride < B) { set_error("a column stride < n_walker"); return FDG_E_INVALID; }
  const SamplerCols cols = sampler_cols(col, n_dim, pol.grouped);
  for (uint32_t d = 0; d < n_dim; ++d)
    if (cols.c[d] >= n_col) { set_error("col names a column >= n_col"); return FDG_E_INVALID; }
  const bool discrete = dv.required || dv.d_cdf;
  ChainDiscArgs da = {};
  if (discrete) {
    if (n_dim == FDG_VEGAS_DIM_MAX) { set_error("n_dim == FDG_VEGAS_DIM_MAX: the discrete variable's counter is the accept rule's"); return FDG_E_UNSUPPORTED; }
    if (!dv.d_cdf || !dv.d_bin || !dv.d_binp) { set_error("null device buffer"); return FDG_E_INVALID; }
    if (dv.d_bin == dv.d_binp) { set_error("d_bin and d_binp are the same buffer"); return FDG_E_INVALID; }
    da = ChainDiscArgs{dv.move ? 1u : 0u, dv.d_cdf, dv.n_bin, dv.d_ext, dv.n_ext, {}, dv.d_bin, dv.d_binp};
    int rc = check_discrete_table(dv.n_bin, FDG_CHAIN_BIN_MAX, "FDG_CHAIN_BIN_MAX", dv.d_ext, dv.n_ext, dv.ext_col, da.ecol);
    if (!rc) rc = check_ext_cols(da.ecol, dv.n_ext, cols, n_dim, pol.grouped, n_col);
    if (rc) return rc;
  }
  if (rc_polar) return rc_polar;
  if (takes_polar) {
    const int rc = check_cols_once(cols, n_dim, pol, da.ecol, da.n_ext);
    if (rc) return rc;
  }
  for (uint32_t g = 0; g < pol.n; ++g) {
    const uint64_t bits = ((1ull << pol.dim[g]) - 1ull) << pol.var[g], has = mask & bits;
    if (has && has != bits) { set_error("mask names some but not all variables of a polar group"); return FDG_E_INVALID; }
  }
  // the shifted variables (fdg_chain_propose_device_local), behind everything the other entries refuse
  ChainLocalArgs loc = {};
  if (local_mask) {
    if (n_dim < 64 && (local_mask >> n_dim)) { set_error("local_mask names a variable >= n_dim"); return FDG_E_INVALID; }
    if (mask & local_mask) { set_error("mask and local_mask name the same variable: it is redrawn or shifted, not both"); return FDG_E_INVALID; }
    if (local_mask & pol.grouped) {
      set_error("local_mask names a variable of a polar group: the state does not hold (k, theta, phi)"); return FDG_E_UNSUPPORTED;
    }
    if (!width) { set_error("local_mask != 0 needs width"); return FDG_E_INVALID; }
    loc.mask = local_mask;
    for (uint32_t d = 0; d < n_dim; ++d) {
      if (!((local_mask >> d) & 1u)) continue;
      if (!(std::isfinite(width[d]) && width[d] > 0.0 && width[d] <= 0.5)) { set_error("a width of a shifted variable is not in (0, 0.5]"); return FDG_E_INVALID; }
      loc.hG[d] = width[d] * (double)n_grid;
    }
  }
  if (B == 0) return FDG_OK;
  with_flag(pol.n != 0, [&](auto p) {
    with_flag(discrete, [&](auto d) {
      with_flag(local_mask != 0, [&](auto l) {
        constexpr bool P = decltype(p)::value, Dc = decltype(d)::value, Lc = decltype(l)::value;
        hipLaunchKernelGGL((fdg_chain_propose<P, Dc, Lc>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_grid, n_dim,
                           n_grid, cols, n_col, mask, seed, sample_offset, d_x, (long)x_col_stride, d_fac, d_xp, (long)xp_col_stride, d_facp,
                           (long)B, arg_if<P>(pol), arg_if<Dc>(da), arg_if<Lc>(loc));
      });
    });
  });
  HIP_TRY(hipGetLastError());
  return FDG_OK;
}

}  // namespace

extern "C" {

int fdg_chain_step_device(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col, uint32_t n_dim,
                          const double *coef, double gamma, uint64_t seed, uint64_t sample_offset, unsigned flags, double *d_x,
                          int64_t x_col_stride, double *d_fac, double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept, int64_t B,
                          void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream};
  return chain_step(g, c, nullptr, CHAIN_PLAIN, nullptr, nullptr);
}

int fdg_mc_chain_step_device(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                             const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma, uint64_t seed,
                             uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride, double *d_fac, double *d_root,
                             double *d_a, double *d_sum, int32_t *d_n_accept, int64_t B, void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream};
  const ChainMc mc{kF, beta, lambda};
  return chain_step(g, c, &mc, CHAIN_PLAIN, nullptr, nullptr);
}

int fdg_chain_step_device_matsubara(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col,
                                    uint32_t n_dim, const double *coef, double gamma, uint64_t seed, uint64_t sample_offset, unsigned flags,
                                    double *d_x, int64_t x_col_stride, double *d_fac, double *d_root, double *d_a, double *d_sum,
                                    int32_t *d_n_accept, const fdg_chain_matsubara *mz, int64_t B, void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream};
  return chain_step(g, c, nullptr, CHAIN_MATSUBARA, mz, nullptr);
}

int fdg_mc_chain_step_device_matsubara(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                                       const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma,
                                       uint64_t seed, uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride,
                                       double *d_fac, double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept,
                                       const fdg_chain_matsubara *mz, int64_t B, void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream};
  const ChainMc mc{kF, beta, lambda};
  return chain_step(g, c, &mc, CHAIN_MATSUBARA, mz, nullptr);
}

int fdg_chain_step_device_grouped(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col,
                                  uint32_t n_dim, const double *coef, double gamma, uint64_t seed, uint64_t sample_offset, unsigned flags,
                                  double *d_x, int64_t x_col_stride, double *d_fac, double *d_root, double *d_a, double *d_sum,
                                  int32_t *d_n_accept, const fdg_chain_matsubara *mz, const fdg_chain_groups *cg, int64_t B,
                                  void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream};
  return chain_step(g, c, nullptr, CHAIN_GROUPED, mz, cg);
}

int fdg_mc_chain_step_device_grouped(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                                     const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma, uint64_t seed,
                                     uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride, double *d_fac,
                                     double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept, const fdg_chain_matsubara *mz,
                                     const fdg_chain_groups *cg, int64_t B, void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream};
  const ChainMc mc{kF, beta, lambda};
  return chain_step(g, c, &mc, CHAIN_GROUPED, mz, cg);
}

int fdg_chain_propose_device(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col, uint64_t mask,
                             uint64_t seed, uint64_t sample_offset, const double *d_x, int64_t x_col_stride, const double *d_fac,
                             double *d_xp, int64_t xp_col_stride, double *d_facp, int64_t B, void *stream) {
  return chain_propose(d_grid, n_dim, n_grid, col, n_col, mask, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp, xp_col_stride, d_facp, B,
                       stream, ChainProposeDiscrete{}, false, nullptr, 0);
}

int fdg_chain_propose_device_discrete(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col,
                                      uint64_t mask, uint64_t seed, uint64_t sample_offset, const double *d_x, int64_t x_col_stride,
                                      const double *d_fac, double *d_xp, int64_t xp_col_stride, double *d_facp, int move_discrete,
                                      const double *d_cdf, uint32_t n_bin, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                      const int32_t *d_bin, int32_t *d_binp, int64_t B, void *stream) {
  return chain_propose(d_grid, n_dim, n_grid, col, n_col, mask, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp, xp_col_stride, d_facp, B,
                       stream, ChainProposeDiscrete{true, move_discrete, d_cdf, n_bin, d_ext, n_ext, ext_col, d_bin, d_binp}, false, nullptr, 0);
}

int fdg_chain_propose_device_polar(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col, uint64_t mask,
                                   uint64_t seed, uint64_t sample_offset, const double *d_x, int64_t x_col_stride, const double *d_fac,
                                   double *d_xp, int64_t xp_col_stride, double *d_facp, int move_discrete, const double *d_cdf,
                                   uint32_t n_bin, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col, const int32_t *d_bin,
                                   int32_t *d_binp, const fdg_vegas_polar *polar, uint32_t n_polar, int64_t B, void *stream) {
  return chain_propose(d_grid, n_dim, n_grid, col, n_col, mask, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp, xp_col_stride, d_facp, B,
                       stream, ChainProposeDiscrete{false, move_discrete, d_cdf, n_bin, d_ext, n_ext, ext_col, d_bin, d_binp}, true, polar,
                       n_polar);
}

int fdg_chain_propose_device_local(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint32_t n_col, uint64_t mask,
                                   uint64_t local_mask, const double *width, uint64_t seed, uint64_t sample_offset, const double *d_x,
                                   int64_t x_col_stride, const double *d_fac, double *d_xp, int64_t xp_col_stride, double *d_facp,
                                   int move_discrete, const double *d_cdf, uint32_t n_bin, const double *d_ext, uint32_t n_ext,
                                   const uint32_t *ext_col, const int32_t *d_bin, int32_t *d_binp, const fdg_vegas_polar *polar, uint32_t n_polar,
                                   int64_t B, void *stream) {
  return chain_propose(d_grid, n_dim, n_grid, col, n_col, mask, seed, sample_offset, d_x, x_col_stride, d_fac, d_xp, xp_col_stride, d_facp, B,
                       stream, ChainProposeDiscrete{false, move_discrete, d_cdf, n_bin, d_ext, n_ext, ext_col, d_bin, d_binp}, true, polar,
                       n_polar, local_mask, width);
}

int fdg_chain_step_device_binned(fdg_graph *g,const double *d_xp, int64_t xp_col_stride, const double *d_facp, uint32_t n_col,
                                 uint32_t n_dim, const double *coef, double gamma, uint64_t seed, uint64_t sample_offset, unsigned flags,
                                 double *d_x, int64_t x_col_stride, double *d_fac, double *d_root, double *d_a, double *d_sum,
                                 int32_t *d_n_accept, const fdg_chain_matsubara *mz, const fdg_chain_groups *cg, uint32_t n_bin,
                                 const int32_t *d_binp, int32_t *d_bin, int64_t B, void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream, n_bin, d_binp, d_bin};
  return chain_step(g, c, nullptr, CHAIN_BINNED, mz, cg);
}

int fdg_mc_chain_step_device_binned(fdg_graph *g, const double *d_xp, int64_t xp_col_stride, double kF, double beta, double lambda,
                                    const double *d_facp, uint32_t n_col, uint32_t n_dim, const double *coef, double gamma, uint64_t seed,
                                    uint64_t sample_offset, unsigned flags, double *d_x, int64_t x_col_stride, double *d_fac,
                                    double *d_root, double *d_a, double *d_sum, int32_t *d_n_accept, const fdg_chain_matsubara *mz,
                                    const fdg_chain_groups *cg, uint32_t n_bin, const int32_t *d_binp, int32_t *d_bin, int64_t B,
                                    void *stream) {
  const ChainCall c{d_xp, xp_col_stride, d_facp, n_col, n_dim, coef, gamma, seed, sample_offset, flags, d_x, x_col_stride, d_fac,
                    d_root, d_a, d_sum, d_n_accept, B, stream, n_bin, d_binp, d_bin};
  const ChainMc mc{kF, beta, lambda};
  return chain_step(g, c, &mc, CHAIN_BINNED, mz, cg);
}

int fdg_chain_reduce_device(const double *d_sum, uint32_t n_root, int64_t B, double *d_out, void *stream) {
  if (B < 0) { set_error("n_walker < 0"); return FDG_E_INVALID; }
  if (!d_sum || !d_out) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (d_sum == d_out) { set_error("d_sum and d_out are the same buffer"); return FDG_E_INVALID; }
  if (B == 0) return FDG_OK;
  hipLaunchKernelGGL(fdg_chain_reduce, dim3(3u * n_root + 2u), dim3(256), 0, (hipStream_t)stream, d_sum, n_root, (long)B, d_out);
  HIP_TRY(hipGetLastError());
  return FDG_OK;
}

}  // extern "C"
