// What the VEGAS samplers (fdg_binned.hip) and the chain's proposals (fdg_chain.hip) share, written once: the by-value kernel arguments,
// the device statements of one variable (drawn, inverted, shifted), of the discrete pick, of the hypercube search and of the polar point, and the host checks of
// the polar groups, the discrete variable's table and the column lists.  Every device function is one fixed sequence of rounded fp64
// operations (the build has no FMA contraction): a kernel that calls one has the bits of every other that does.
// Include after fdg_internal.h with FDG_RUNTIME_TU defined.
#pragma once

#include <algorithm>
#include <type_traits>
#include <vector>

#include "fdg_internal.h"
#include "fdg_sincos.h"

namespace {

// ---- kernel arguments, by value ----
struct SamplerCols { uint32_t c[FDG_VEGAS_DIM_MAX]; };     // the column of x each variable is written to
struct SamplerExtCols { uint32_t c[FDG_VEGAS_EXT_MAX]; };  // the columns of x the rows of the discrete variable's table go to

// The groups of polar variables: group g takes the variables var[g] .. var[g] + dim[g] - 1 and writes the Cartesian components to the
// columns col[g][0 .. dim[g]).  grouped: bit d set = variable d belongs to a group.
struct SamplerPolar {
  uint64_t grouped;
  uint32_t n;
  uint32_t var[FDG_VEGAS_POLAR_MAX], dim[FDG_VEGAS_POLAR_MAX];
  uint32_t col[FDG_VEGAS_POLAR_MAX][3];
};

// The strata of the stratified calls: n[d] strata of variable d, div[d] = n[0] * .. * n[d - 1] (the digit of hypercube h in variable d
// is h / div[d] % n[d]; 1 and 1 past n_dim), H their product.
struct VegasStrat { uint32_t n[FDG_VEGAS_DIM_MAX], div[FDG_VEGAS_DIM_MAX], H; };

// A kernel instance takes only the arguments it reads: ArgIf<ON, T> is T in the instances that read it and an empty struct in the
// others; arg_if<ON>(v) is the value to launch with.  with_flag(v, f): f(std::bool_constant<v>) for a run-time v, the way from what
// a call carries to the instance.
struct SamplerNoArg {};
template <bool ON, class T> using ArgIf = std::conditional_t<ON, T, SamplerNoArg>;
template <bool ON, class T> ArgIf<ON, T> arg_if(const T &v) {
  if constexpr (ON) return v;
  else return {};
}
template <class F> auto with_flag(bool v, F f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// ---- device statements ----
// The cell of variable d that sample `sample` (a global index: the Philox counter) falls in, and y = u * G; every operation one rounded
// fp64 operation.  The samplers and the training pass both call this: the pass reads no cell array.
__device__ __forceinline__ uint32_t vegas_cell(uint64_t sample, uint32_t d, uint64_t seed, uint32_t G, double &y) {
  const double u = fdg_philox_u53(sample, d, seed);
  y = u * (double)G;
  return min((uint32_t)(int)y, G - 1u);
}

// vegas_cell inside stratum s of ns: v = (s + u) / ns in the place of u.  (0 + u) / 1 = u exactly: one stratum is vegas_cell.
__device__ __forceinline__ uint32_t vegas_cell_strat(uint64_t sample, uint32_t d, uint64_t seed, uint32_t G, uint32_t s, uint32_t ns, double &y) {
  const double u = fdg_philox_u53(sample, d, seed);
  const double v = ((double)s + u) / (double)ns;
  y = v * (double)G;
  return min((uint32_t)(int)y, G - 1u);
}

// Variable d of `sample` through the map: its value, returned, its cell c and its factor f = G * wd of the jacobian.  STRAT: drawn
// inside stratum s of ns (not read otherwise).
template <bool STRAT = false>
__device__ __forceinline__ double vegas_draw(const double *__restrict__ grid, uint32_t d, uint32_t G, uint64_t sample, uint64_t seed, uint32_t s,
                                             uint32_t ns, uint32_t &c, double &f) {
  double y;
  if constexpr (STRAT) c = vegas_cell_strat(sample, d, seed, G, s, ns, y);
  else c = vegas_cell(sample, d, seed, G, y);
  const double *e = grid + (size_t)d * (G + 1u) + c;
  const double lo = e[0], wd = e[1] - lo, fr = y - (double)c;
  f = (double)G * wd;
  return lo + fr * wd;
}

// The inverse of the map for variable d: the coordinate yy in cells, 0 <= yy <= G, of the value xv.  c = the number of interior edges
// e[1 .. G - 1] that are <= xv (a binary search per lane like discrete_pick's: a row is at most a few KiB and stays in cache; G = 1
// searches nothing), then fr = (xv - e[c]) / (e[c + 1] - e[c]) clamped into [0, 1] (0 for a cell without width and for a nan), and
// yy = c + fr.  A value outside the row is clamped, never faulted on: every index lies in [0, G].
__device__ __forceinline__ double vegas_invert(const double *__restrict__ grid, uint32_t d, uint32_t G, double xv) {
  const double *e = grid + (size_t)d * (G + 1u);
  uint32_t lo = 0, hi = G - 1u;                           // c in [lo, hi]: e[1 .. lo] <= xv < e[hi + 1 ..]
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (e[mid + 1u] <= xv) lo = mid + 1u; else hi = mid;
  }
  const double l = e[lo], wd = e[lo + 1u] - l;
  double fr = (xv - l) / wd;
  if (wd == 0.0 || !(fr >= 0.0)) fr = 0.0;
  if (fr > 1.0) fr = 1.0;
  return (double)lo + fr;
}

// Variable d of `sample` moved from the value xv by a shift in the map's coordinate: y' = y + t h (mod 1) with t = 2 u - 1 uniform in
// [-1, 1), u the Philox column d (the one a redraw of d would use: a variable is redrawn or shifted in one step, never both) and
// hG = h * G the half width in cells, formed on the host.  One wrap suffices because h <= 0.5.  The new value is returned and f = G * wd
// of its cell: the tail of vegas_draw.  The proposal is symmetric in y, so the chain's accept rule needs no factor for it.
__device__ __forceinline__ double vegas_shift(const double *__restrict__ grid, uint32_t d, uint32_t G, uint64_t sample, uint64_t seed, double hG,
                                              double xv, double &f) {
  const double yy = vegas_invert(grid, d, G, xv);
  const double u = fdg_philox_u53(sample, d, seed);
  const double t = (u + u) - 1.0;
  const double s = t * hG;
  double y1 = yy + s;
  if (y1 < 0.0) y1 = y1 + (double)G;
  if (y1 >= (double)G) y1 = y1 - (double)G;
  const uint32_t c = min((uint32_t)(int)y1, G - 1u);
  const double *e = grid + (size_t)d * (G + 1u) + c;
  const double lo = e[0], wd = e[1] - lo, fr = y1 - (double)c;
  f = (double)G * wd;
  return lo + fr * wd;
}

// The discrete variable of `sample` behind D continuous ones: its uniform is the Philox column D, its value j, returned, the number
// of interior edges of cdf that are <= u (a binary search per lane: the cdf is at most 128 KiB and stays in L2), p its probability.
__device__ __forceinline__ uint32_t discrete_pick(const double *__restrict__ cdf, uint32_t n_bin, uint64_t sample, uint32_t D, uint64_t seed,
                                                  double &p) {
  const double u = fdg_philox_u53(sample, D, seed);
  uint32_t lo = 0, hi = n_bin - 1u;                       // j in [lo, hi]: cdf[1 .. lo] <= u < cdf[hi + 1 ..]
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (cdf[mid + 1u] <= u) lo = mid + 1u; else hi = mid;
  }
  p = cdf[lo + 1u] - cdf[lo];
  return lo;
}

// The hypercube h of sample i, returned, and its number of samples n_h: a binary search in the prefix sums start[0 .. H] (at most 20
// steps; the table is at most 8 MiB and stays in L2).
__device__ __forceinline__ uint32_t strat_cube(const int64_t *__restrict__ start, uint32_t H, int64_t i, int64_t &n_h) {
  uint32_t lo = 0, hi = H - 1u;                           // h in [lo, hi]: start[lo] <= i
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (start[mid] <= i) lo = mid; else hi = mid - 1u;
  }
  n_h = start[lo + 1u] - start[lo];
  return lo;
}

// The Cartesian components of a polar point: (k, phi) -> c0, c1, or (k, theta, phi) -> c0, c1, c2 and st = sin(theta) (in two
// dimensions theta is not read, c2 not written and st = 0).  The folds of the measure, k or k k st, stay with the callers.
__device__ __forceinline__ void polar_point(bool three, double k, double theta, double phi, double &c0, double &c1, double &c2, double &st) {
  double sp, cp;
  fdg_sincos_impl(phi, sp, cp);
  if (three) {
    double ct;
    fdg_sincos_impl(theta, st, ct);
    const double ks = k * st;
    c0 = ks * cp;
    c1 = ks * sp;
    c2 = k * ct;
  } else {
    c0 = k * cp;
    c1 = k * sp;
    st = 0.0;
  }
}

// ---- host checks; each sets the message of the first refusal and returns its code ----
// The column of every variable: col[d], d itself without a list, 0 where bit d of `skip` is set (a variable of a polar group: its
// entry is not read).
inline SamplerCols sampler_cols(const uint32_t *col, uint32_t n_dim, uint64_t skip = 0) {
  SamplerCols cols;
  for (uint32_t d = 0; d < FDG_VEGAS_DIM_MAX; ++d) cols.c[d] = d < n_dim && !((skip >> d) & 1u) ? (col ? col[d] : d) : 0u;
  return cols;
}

// The polar groups of a call into pol: at most FDG_VEGAS_POLAR_MAX of them, each of 2 or 3 variables inside n_dim, no variable in two,
// and (n_col >= 0) every column below n_col.  pol.grouped holds the variables of every well-formed group even when the call is
// refused: the checks that rank before these need it, since the col entry of a grouped variable is not read.
inline int parse_polar(const fdg_vegas_polar *polar, uint32_t n_polar, uint32_t n_dim, int64_t n_col, SamplerPolar &pol) {
  int rc = FDG_OK;
  auto refuse = [&](const char *why, int code) {
    if (rc == FDG_OK) fdg::set_error(why), rc = code;
  };
  pol = {};
  pol.n = n_polar;
  if (n_polar > FDG_VEGAS_POLAR_MAX) refuse("n_polar > FDG_VEGAS_POLAR_MAX", FDG_E_UNSUPPORTED);
  if (n_polar && !polar) refuse("n_polar > 0 needs polar", FDG_E_INVALID);
  if (!polar) return rc;
  const uint32_t n = std::min<uint32_t>(n_polar, FDG_VEGAS_POLAR_MAX);
  const uint32_t end = std::min<uint32_t>(n_dim, FDG_VEGAS_DIM_MAX);   // (a larger n_dim is refused by the caller, whatever this finds)
  for (uint32_t g = 0; g < n; ++g) {
    const fdg_vegas_polar &p = polar[g];
    if (p.dim != 2 && p.dim != 3) { refuse("a polar group has 2 or 3 variables", FDG_E_INVALID); continue; }
    if (p.var >= end || p.var + p.dim > end) { refuse("a polar group reaches past n_dim", FDG_E_INVALID); continue; }
    const uint64_t bits = ((1ull << p.dim) - 1ull) << p.var;
    if (pol.grouped & bits) refuse("two polar groups share a variable", FDG_E_INVALID);
    pol.grouped |= bits;
    pol.var[g] = p.var;
    pol.dim[g] = p.dim;
    for (uint32_t i = 0; i < p.dim; ++i) pol.col[g][i] = p.col[i];
  }
  for (uint32_t g = 0; g < n && n_col >= 0; ++g)
    for (uint32_t i = 0; i < pol.dim[g]; ++i)
      if (pol.col[g][i] >= n_col) refuse("a polar group names a column >= n_col", FDG_E_INVALID);
  return rc;
}

// The discrete variable's table: n_bin within bin_max (bin_max_name: its name in the message), n_ext within FDG_VEGAS_EXT_MAX, the
// table and its columns given when it has any; ecols = the columns.
inline int check_discrete_table(uint32_t n_bin, uint32_t bin_max, const char *bin_max_name, const double *d_ext, uint32_t n_ext,
                                const uint32_t *ext_col, SamplerExtCols &ecols) {
  if (n_bin == 0) { fdg::set_error("n_bin == 0"); return FDG_E_INVALID; }
  if (n_bin > bin_max) { fdg::set_error(std::string("n_bin > ") + bin_max_name); return FDG_E_UNSUPPORTED; }
  if (n_ext > FDG_VEGAS_EXT_MAX) { fdg::set_error("n_ext > FDG_VEGAS_EXT_MAX"); return FDG_E_UNSUPPORTED; }
  if (n_ext && (!d_ext || !ext_col)) { fdg::set_error("n_ext > 0 needs d_ext and ext_col"); return FDG_E_INVALID; }
  for (uint32_t e = 0; e < FDG_VEGAS_EXT_MAX; ++e) ecols.c[e] = e < n_ext ? ext_col[e] : 0u;
  return FDG_OK;
}

// The table's columns against the variables': below n_col (n_col >= 0), none twice, none a variable's (bit d of skip set: col[d] is
// not read).  The calls without polar groups make this check; they do not ask the variables' own columns to differ.
inline int check_ext_cols(const SamplerExtCols &ecols, uint32_t n_ext, const SamplerCols &cols, uint32_t n_dim, uint64_t skip, int64_t n_col) {
  for (uint32_t e = 0; e < n_ext; ++e) {
    if (n_col >= 0 && ecols.c[e] >= n_col) { fdg::set_error("ext_col names a column >= n_col"); return FDG_E_INVALID; }
    for (uint32_t f = 0; f < e; ++f)
      if (ecols.c[f] == ecols.c[e]) { fdg::set_error("ext_col names a column twice"); return FDG_E_INVALID; }
    for (uint32_t d = 0; d < n_dim; ++d)
      if (!((skip >> d) & 1u) && cols.c[d] == ecols.c[e]) { fdg::set_error("ext_col names a column of col"); return FDG_E_INVALID; }
  }
  return FDG_OK;
}

// Every written column named once: the variables of no group, the groups' components, the discrete variable's table.  The calls with
// polar groups make this check.
inline int check_cols_once(const SamplerCols &cols, uint32_t n_dim, const SamplerPolar &pol, const SamplerExtCols &ecols, uint32_t n_ext) {
  std::vector<uint32_t> named;
  for (uint32_t d = 0; d < n_dim; ++d)
    if (!((pol.grouped >> d) & 1u)) named.push_back(cols.c[d]);
  for (uint32_t g = 0; g < pol.n; ++g) named.insert(named.end(), pol.col[g], pol.col[g] + pol.dim[g]);
  named.insert(named.end(), ecols.c, ecols.c + n_ext);
  std::sort(named.begin(), named.end());
  if (std::adjacent_find(named.begin(), named.end()) != named.end()) { fdg::set_error("a column of x is named twice"); return FDG_E_INVALID; }
  return FDG_OK;
}

}  // namespace
