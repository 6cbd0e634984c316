// Binned accumulation (include/fdg.h: fdg_accumulate_device_binned, fdg_mc_accumulate_device_binned): the `measure` step of a
// Monte-Carlo integrand whose observable is a function of an external variable, acc[j][k] += w[b] root_k(b) for the samples b whose bin
// is j.  The roots of a chunk of samples are evaluated into the column-major root scratch by whatever route the handle takes for
// fdg_eval_device (every back end, layout and association, the same bits), then the pass below bins them; after the last chunk the
// per-segment partial histograms are added into acc in segment order.
//
// No float atomics, in global memory or in LDS: every sum below has an order fixed by the arguments alone.
//  * A workgroup owns one segment of the chunk's 64-sample tiles and one slice of the roots, and keeps the slice's histogram
//    (n_bin x RS doubles) in LDS.  Its four waves take the segment's tiles in rounds, wave w the tile 4 r + w of round r.
//  * Inside a wave the 64 lanes are sorted by (bin, lane) (a bitonic network over the lanes); a segmented suffix scan in that order
//    leaves every run of equal bins summed in its first lane, which adds the run's sum into the histogram.  Runs have distinct bins,
//    so no two lanes of a wave touch one LDS word.
//  * The waves add their runs in turn, wave 0 first, a barrier between turns: per bin, tiles are added in tile order.
//  * The histogram starts at zero in the first chunk and at the segment's partial of the previous chunk in the others; the partials
//    [segment][bin][root] are summed in segment order by fdg_binned_reduce, whose result is added to acc.
// Samples past n_sample and samples whose bin is out of range never reach a sum (no 0 * root term: an inf or nan root of such a sample
// cannot poison a bin).  Work is split by samples, never by bin, so a crowded bin costs what a sparse one does.
//
// Second moments (fdg_accumulate_device_moments, fdg_mc_accumulate_device_moments): the same pass over t = w root_k and t * t.  The
// chunk size and the segment count are the binned call's (binned_plan), and the order of the t sums is the one above, so acc comes out
// with the binned call's bits.  A workgroup keeps both histograms (2 x n_bin x RS doubles) and scans t and t * t together; when even one
// root does not fit twice (n_bin > 8192), every root slice gets two workgroups, one per moment, and the second reads the scratch columns again.
// The slab is then [segment][moment][bin][root], and the reduce adds both moments in segment order.
//
// VEGAS importance sampling (fdg_vegas_sample_device, fdg_accumulate_device_vegas, fdg_mc_accumulate_device_vegas, fdg_vegas_refine):
// the sampler draws through a piecewise-linear map per variable; the accumulate calls are the second-moment calls without a bin vector
// plus one more pass per chunk over the same roots (fdg_vegas_partials below) that sums (w sum_k c_k root_k)^2 into a histogram per
// variable and map cell, the cell recomputed from the sample's Philox counter; the refinement of the map is host code at the end.
//
// The discrete external variable (fdg_vegas_sample_device_discrete, fdg_[mc_]accumulate_device_vegas_binned, fdg_vegas_refine_discrete):
// the sampler draws one of n_bin values by its cumulative distribution next to the continuous variables; the accumulate calls are the
// moments calls WITH their bin vector plus the training pass above plus one more pass (fdg_vegas_bin_partials) that sums the same
// (w sum_k c_k root_k)^2 per value of the discrete variable, the key read from the bin vector.
//
// Spherical momentum variables (fdg_vegas_sample_device_polar): groups of 2 or 3 consecutive variables are (k, phi) or (k, theta, phi);
// the sampler writes their Cartesian components and folds k (or k k sin theta) into the weight, the sine and cosine from fdg_sincos.h.
// The accumulate side is untouched: the training pass recomputes cells from the Philox counters and never reads x.
//
// Matsubara projection (fdg_[mc_]accumulate_device_matsubara): one more pass per chunk over the same roots (fdg_matsubara_partials
// below) that multiplies every root by the phase of its own pair of external times at every frequency and sums the real and imaginary
// parts and their squares per (bin, frequency, root); the moments pass and the training passes run beside it when the call asks for them.
//
// Weight groups (fdg_vegas_sample_device_grouped, fdg_[mc_]accumulate_device_grouped): roots are assigned to groups, every group owns a
// set of the VEGAS variables and has its own weight column.  Each kernel above carries a GRP template flag: the sampler folds every
// variable into the jacobians of the groups that own it, the moments and projection passes read the weight column of a root's group,
// and the training passes sum (w_g s_g)^2 over the groups that own a variable.  The ungrouped instantiations are the code they were;
// a grouped call with one group and a full mask runs them.
//
// Observables (fdg_[mc_]accumulate_device_observables): one more pass per chunk over the same roots (fdg_obs_partials below) that
// forms up to FDG_OBS_MAX linear combinations o_m of the weighted roots per sample and sums o_m and the products o_a o_c per bin: the
// first moment and the covariance of sums, differences and series of roots, which the per-root acc2 cannot give because all roots
// share their samples.  A kernel of its own: every instance above is the code it was.
//
// Frequency observables (fdg_[mc_]accumulate_device_freq_observables): the same over the PROJECTED roots (fdg_fobs_partials below), 2 M
// components per frequency in the place of the rows.  The two passes share everything but their partials kernels: one plan
// (obs_plan), one table builder (obs_tables), one reduce (fdg_obs_reduce) and one host path (ObsPass).
//
// Adaptive stratified sampling (fdg_vegas_sample_device_strat, fdg_[mc_]accumulate_device_strat, fdg_strat_allocate): the unit cube of
// the map's coordinates is cut into H hypercubes whose samples are contiguous; the sampler finds a sample's hypercube by a binary
// search in the prefix sums and draws inside its strata; the training pass carries a STRAT flag that recomputes the cell by the same
// formula; one more pass per chunk (fdg_strat_partials, fdg_strat_stitch below) sums w root_k and its square per hypercube, runs of
// equal hypercubes inside a wave by the segmented scan above, runs that cross waves, tiles or chunks level by level from edge records.
// With polar groups and weight groups (the _strat_grouped calls): the polar sampler carries the same STRAT flag, the training pass runs
// with STRAT beside GRP, and the per-hypercube pass takes one column per group behind the roots' in the place of the one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#define FDG_RUNTIME_TU 1
#include "fdg_internal.h"
#include "fdg_matsubara.h"
#include "fdg_sincos.h"
#include "fdg_sampler.h"

using namespace fdg;

namespace {

constexpr uint32_t kBinWaves = 4;                         // waves per workgroup of the binned pass
constexpr size_t kBinLdsBudget = 64u << 10;               // LDS of a histogram slice, unless one root of FDG_BIN_MAX bins needs more
constexpr size_t kBinSlabBytes = 64ull << 20;             // bound of the partial slab [segment][bin][root]
constexpr uint32_t kKeyInvalid = 0xFFFFFFC0u;             // (bin << 6 | lane) of a sample that adds nothing: sorts behind every bin

__device__ inline void bin_barrier() {
  // LDS only: the pending global loads of the next round stay in flight across the barrier
  __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The wave-level pieces of the passes below.  key = (bin << 6 | lane), kKeyInvalid | lane for a lane that adds nothing; valid = the ballot of
// key < kKeyInvalid (not zero).  Sorts the 64 keys ascending over the lanes -- a bitonic network; the keys are unique, the lane is part of
// them -- unless every lane is valid and in one bin, and returns the lane this lane's key came from.
__device__ inline uint32_t wave_sort_keys(uint32_t &key, uint32_t lane, uint64_t valid) {
  const uint32_t key0 = __shfl(key, 0);
  if (valid == ~0ull && __ballot((key >> 6) == (key0 >> 6)) == ~0ull) return lane;
#pragma unroll
  for (uint32_t kb = 2; kb <= 64; kb <<= 1)
#pragma unroll
    for (uint32_t jb = kb >> 1; jb > 0; jb >>= 1) {
      const uint32_t other = __shfl_xor(key, (int)jb);
      const bool keep_min = ((lane & kb) == 0) == ((lane & jb) == 0);
      key = keep_min ? min(key, other) : max(key, other);
    }
  return key & 63u;
}

// The runs of equal bins among the sorted keys: j = this lane's bin, head = it is the first lane of a run of valid keys, end = the last
// lane of its run (the lane itself where the key is invalid).
__device__ inline void wave_runs(uint32_t key, uint32_t lane, uint32_t &j, bool &head, uint32_t &end) {
  j = key >> 6;
  const bool ok = key < kKeyInvalid;
  const uint32_t j_prev = __shfl_up(j, 1);
  const uint32_t j_next = __shfl_down(j, 1);
  head = ok && (lane == 0 || j_prev != j);
  const uint64_t tails = __ballot(!ok || lane == 63 || j_next != j);
  end = ok ? (uint32_t)__builtin_ctzll(tails & (~0ull << lane)) : lane;
}

// The tiles t0 .. t1 - 1 of a chunk of n samples that segment seg of seg_tiles tiles holds, and the rounds its four waves take them in.
struct SegTiles { long t0, t1, rounds; };
__device__ inline SegTiles seg_tiles_of(long n, uint32_t seg, long seg_tiles) {
  const long ntile = (n + 63) / 64, t0 = (long)seg * seg_tiles, t1 = min(t0 + seg_tiles, ntile);
  return {t0, t1, t1 > t0 ? (t1 - t0 + kBinWaves - 1) / kBinWaves : 0};
}

// What a workgroup of the pass accumulates: the first moment (the binned call), both moments in one LDS, or one moment per root slice
// (slices n_slice .. 2 n_slice - 1 are the second moment's; the histograms of both do not fit the LDS).
enum BinMode { kFirst = 0, kBoth = 1, kSplit = 2 };

// One workgroup per (segment, root slice); roots of the chunk at root[k * ld + b], b < n.  bins == null: every sample is in bin 0.
// GRP (the grouped calls with more than one group): the weight of root k is the column of its group, weight[g * wstride + b]; the
// prefetch loads the distinct columns of the slice (gtab, below), one when its roots share a group, and the term picks its own by
// wave-uniform selects.  Nothing else differs: the sorts, the scans and the order of every sum are those of the ungrouped instance.
// gtab, one table per call as uint32: the group of every root [R] (a root that does not exist takes a neighbour's, so that it adds
// no column to a slice), then per root slice of this pass kGrpEntry words -- the number of distinct groups among the slice's roots,
// their numbers (the weight columns the slice loads), and for each of the slice's roots the place of its group in that list.
constexpr uint32_t kGrpCols = FDG_WEIGHT_GROUP_MAX, kGrpEntry = 1u + kGrpCols + 16u;

template <int RS, int MODE, bool GRP = false>
__global__ void __launch_bounds__(256)
fdg_binned_partials(const double *__restrict__ root, long ld, long n, const int32_t *__restrict__ bins, int32_t bin_base, uint32_t n_bin,
                    const double *__restrict__ weight, uint32_t R, uint32_t n_slice, long seg_tiles, double *__restrict__ partial, int first,
                    const uint32_t *__restrict__ gtab, long wstride) {
  extern __shared__ double hist[];                        // [moment][bin][RS]
  constexpr uint32_t NH = MODE == kBoth ? 2 : 1;          // histograms in LDS
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t n_grp = MODE == kSplit ? 2 * n_slice : n_slice;
  const uint32_t grp = blockIdx.x % n_grp, seg = blockIdx.x / n_grp;
  const uint32_t mom = MODE == kSplit ? grp / n_slice : 0, slice = grp % n_slice;   // kSplit: the moment this slice sums
  const uint32_t k0 = slice * RS, kn = min((uint32_t)RS, R - k0);
  const size_t hist_cols = (size_t)n_bin * R;
  double *slab = partial + (size_t)seg * hist_cols * (MODE == kFirst ? 1 : 2) + (size_t)mom * hist_cols + k0;
  for (uint32_t i = threadIdx.x; i < NH * n_bin * RS; i += 256) {
    const uint32_t j = i / RS, kk = i % RS;               // j: moment * n_bin + bin, as in the slab
    hist[i] = (first || kk >= kn) ? 0.0 : slab[(size_t)j * R + kk];
  }
  __syncthreads();
  const SegTiles sg = seg_tiles_of(n, seg, seg_tiles);
  const long t0 = sg.t0, t1 = sg.t1, rounds = sg.rounds;

  // this lane's sample of round r, loaded one round ahead without a branch (indices clamped into the chunk: every load is issued at once
  // and stays in flight while the round before is binned); whether the sample adds anything is decided when it is used
  constexpr int WC = !GRP ? 1 : RS < (int)kGrpCols ? RS : (int)kGrpCols;   // the weight columns a slice can need
  uint32_t n_wcol = 1, wcol[WC] = {}, widx[RS] = {};
  if constexpr (GRP) {
    const uint32_t *e = gtab + R + (size_t)slice * kGrpEntry;
    n_wcol = e[0];
#pragma unroll
    for (int c = 0; c < WC; ++c) wcol[c] = e[1 + c];
#pragma unroll
    for (int kk = 0; kk < RS; ++kk) widx[kk] = e[1 + kGrpCols + kk];
  }
  int32_t bin_n;
  double w_n[WC] = {}, r_n[RS];
  auto fetch = [&](long r) {
    const long b = min((t0 + r * (long)kBinWaves + wave) * 64 + lane, n - 1);
    bin_n = bins ? bins[b] : bin_base;
    if constexpr (GRP) {
#pragma unroll
      for (int c = 0; c < WC; ++c)
        if ((uint32_t)c < n_wcol) w_n[c] = weight[(size_t)wcol[c] * (size_t)wstride + (size_t)b];
    } else {
      w_n[0] = weight ? weight[b] : 1.0;
    }
#pragma unroll
    for (int kk = 0; kk < RS; ++kk) r_n[kk] = root[(size_t)min(k0 + kk, R - 1) * (size_t)ld + (size_t)b];
  };
  fetch(0);
  for (long r = 0; r < rounds; ++r) {
    // key (bin << 6 | lane) and w * root_k: kKeyInvalid and 0 where the sample adds nothing (selected, never multiplied by 0)
    const long t = t0 + r * (long)kBinWaves + wave, b = t * 64 + lane;
    const int64_t jb = (int64_t)bin_n - (int64_t)bin_base;
    const bool in = t < t1 && b < n && jb >= 0 && jb < (int64_t)n_bin;
    uint32_t key = in ? ((uint32_t)jb << 6) | lane : kKeyInvalid | lane;
    double v[RS];
#pragma unroll
    for (int kk = 0; kk < RS; ++kk) {
      double wk = w_n[0];
#pragma unroll
      for (int c = 1; c < WC; ++c) wk = widx[kk] == (uint32_t)c ? w_n[c] : wk;
      v[kk] = in ? wk * r_n[kk] : 0.0;
    }
    fetch(r + 1);                                        // the next round's loads are in flight while this one is binned

    const uint64_t valid = __ballot(key < kKeyInvalid);
    double s[RS] = {}, s2[RS] = {};                       // s2: kBoth only
    bool head = false;
    uint32_t j = 0;
    if (valid) {
      const uint32_t src = wave_sort_keys(key, lane, valid);
      uint32_t end;
      wave_runs(key, lane, j, head, end);
#pragma unroll
      for (int kk = 0; kk < RS; ++kk) s[kk] = __shfl(v[kk], (int)src);
      // the square of the source lane's term (t * t, rounded, no fma: -ffp-contract=off); 0 where the term was selected away
      if (MODE == kBoth) {
#pragma unroll
        for (int kk = 0; kk < RS; ++kk) s2[kk] = s[kk] * s[kk];
      } else if (MODE == kSplit && mom) {
#pragma unroll
        for (int kk = 0; kk < RS; ++kk) s[kk] = s[kk] * s[kk];
      }
      // segmented suffix scan: after the step of distance d, lane i holds the sum of lanes i .. min(i + 2d - 1, end)
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const bool take = lane + d <= end;
        if (!__ballot(take)) break;
#pragma unroll
        for (int kk = 0; kk < RS; ++kk) {
          const double t = __shfl_down(s[kk], d);
          if (take) s[kk] = s[kk] + t;
        }
        if (MODE == kBoth) {
#pragma unroll
          for (int kk = 0; kk < RS; ++kk) {
            const double t = __shfl_down(s2[kk], d);
            if (take) s2[kk] = s2[kk] + t;
          }
        }
      }
    }
    // the waves' turns, in wave order (the LDS words of one bin are only ever written by one wave at a time)
    for (uint32_t w = 0; w < kBinWaves; ++w) {
      if (wave == w && head) {
#pragma unroll
        for (int kk = 0; kk < RS; ++kk)
          if ((uint32_t)kk < kn) {
            hist[j * RS + kk] = hist[j * RS + kk] + s[kk];
            if (MODE == kBoth) hist[(n_bin + j) * RS + kk] = hist[(n_bin + j) * RS + kk] + s2[kk];
          }
      }
      bin_barrier();
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < NH * n_bin * RS; i += 256) {
    const uint32_t jj = i / RS, kk = i % RS;
    if (kk < kn) slab[(size_t)jj * R + kk] = hist[i];
  }
}

// acc[c] += sum over segments s of partial[s][c] (c = bin * R + k), segments in order: thread (q, c) adds the segments q, q + Q, ...,
// then the Q sums are added q = 0, 1, ...; columns of roots that do not exist are left alone.  blockIdx.y = moment m: its partials at
// partial + m * ncol, segment s at s * seg_stride, added into acc (m = 0) or acc2 (m = 1).
__global__ void __launch_bounds__(256)
fdg_binned_reduce(const double *__restrict__ partial, uint32_t n_seg, long seg_stride, long ncol, uint32_t R, uint32_t C,
                  double *__restrict__ acc, double *__restrict__ acc2, const uint8_t *__restrict__ live) {
  __shared__ double sh[256];
  const uint32_t Q = 256u / C, q = threadIdx.x / C, cl = threadIdx.x % C;
  const long c = (long)blockIdx.x * C + cl;
  const double *part = partial + (size_t)blockIdx.y * (size_t)ncol;
  double *out = blockIdx.y ? acc2 : acc;
  double s = 0.0;
  if (c < ncol)
    for (uint32_t sg = q; sg < n_seg; sg += Q) s = s + part[(size_t)sg * (size_t)seg_stride + (size_t)c];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (q == 0 && c < ncol) {
    double t = sh[cl];
    for (uint32_t qq = 1; qq < Q && qq < n_seg; ++qq) t = t + sh[qq * C + cl];
    if (!live || live[c % R]) out[c] = out[c] + t;
  }
}

// ---- Observables: linear combinations of the roots and their covariance (include/fdg.h: fdg_[mc_]accumulate_device_observables) ----
// The value columns of a sample: o_0 .. o_{n_obs - 1}, then the products o_a o_c, a <= c, row by row of the upper triangle:
// V = n_obs + n_obs (n_obs + 1) / 2 columns.  One workgroup per (segment of the chunk's tiles, slice of CS consecutive columns), the
// slice's histogram (n_bin x CS doubles) in LDS; its four waves take the segment's tiles in rounds, wave w the tile 4 r + w, exactly
// as fdg_binned_partials deals them.
//  * A wave sorts its tile's lanes by (bin, lane) FIRST (the keys need the bin vector only), and every lane then forms the o_m of
//    the sample whose key it holds: the root and weight columns are read at the sorted position, still inside the tile's 512 bytes of
//    every column, so nothing has to cross lanes afterwards.
//  * The slice's table (one upload per call, built on the host) lists the roots that the rows it needs use, ascending, each with the
//    place of its weight column and its terms (row, coefficient), zero coefficients and roots that do not exist compacted away.  A
//    root column is loaded once per tile, t = w_g(k) root_k formed as the moments pass forms it, and every term folds coef * t into its
//    row's word of the lane's LDS stash ([row of the slice][256 lanes]: a lane only ever touches its own words).  The first term of a
//    row starts the fold (flag in the table); the fold runs over ascending k.
//  * The columns of the slice are then scanned kObsGroup at a time: a column is a stash word or the rounded product of two, 0.0
//    selected where the key is invalid; the segmented suffix scan and the waves' turns are fdg_binned_partials' own, so per (bin,
//    column) the tiles are added in tile order.
//  * Chunks and segments chain through partial [segment][bin][V], summed in segment order by fdg_obs_reduce.
// The tables (obs_tables builds them for this pass and for the frequency observables', which adds what is in brackets).  utab, per
// call: four words per column slice {rows needed, root records, offset of the slice's words in utab, offset of its coefficients in
// dtab}; the slice's words are colA[CS], colB[CS] (stash rows of a column's one or two factors; kObsNone: no second factor, or a
// column of a row without terms, which stays 0), then four [kFobsRec] words per root record {root, place of its weight column [bit
// 31: the time labels of the record before], first term, end of terms [, tin, tout: 0-based components of T]}, then a word per term
// (stash row, bit 31: the term starts its row's fold [bit 30: the term takes tim, else tre]).  dtab: [mult[FDG_MATSUBARA_FREQ_MAX],
// then] the terms' coefficients.
constexpr uint32_t kObsGroup = 16;                        // columns a wave scans together
constexpr uint32_t kObsNone = 0xFFFFFFFFu;
constexpr uint32_t kObsFirst = 0x80000000u;

__global__ void __launch_bounds__(256)
fdg_obs_partials(const double *__restrict__ root, long ld, long n, const int32_t *__restrict__ bins, int32_t bin_base, uint32_t n_bin,
                 const double *__restrict__ weight, long wstride, uint32_t n_wcol, uint32_t V, uint32_t CS, uint32_t n_slice, long seg_tiles,
                 double *__restrict__ partial, int first, const uint32_t *__restrict__ utab, const double *__restrict__ dtab) {
  extern __shared__ double hist[];                        // [bin][CS], then the stash [row][256]
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t slice = blockIdx.x % n_slice, seg = blockIdx.x / n_slice;
  const uint32_t c0 = slice * CS, cn = min(CS, V - c0);
  const uint32_t *hdr = utab + (size_t)slice * 4u;
  const uint32_t n_rec = hdr[1];
  const uint32_t *colA = utab + hdr[2], *colB = colA + CS, *rec = colB + CS, *tslot = rec + (size_t)n_rec * 4u;
  const double *tcoef = dtab + hdr[3];
  double *stash = hist + (size_t)n_bin * CS + threadIdx.x;
  double *slab = partial + (size_t)seg * n_bin * V + c0;
  for (uint32_t i = threadIdx.x; i < n_bin * CS; i += 256) {
    const uint32_t j = i / CS, cl = i % CS;
    hist[i] = (first || cl >= cn) ? 0.0 : slab[(size_t)j * V + cl];
  }
  __syncthreads();
  const SegTiles sg = seg_tiles_of(n, seg, seg_tiles);
  const long t0 = sg.t0, t1 = sg.t1, rounds = sg.rounds;
  int32_t bin_n;
  auto fetch = [&](long r) {                              // the bin of this lane's sample of round r, one round ahead (index clamped)
    const long b = min((t0 + r * (long)kBinWaves + wave) * 64 + lane, n - 1);
    bin_n = bins ? bins[b] : bin_base;
  };
  fetch(0);
  for (long r = 0; r < rounds; ++r) {
    const long t = t0 + r * (long)kBinWaves + wave, b = t * 64 + lane;
    const int64_t jb = (int64_t)bin_n - (int64_t)bin_base;
    const bool in = t < t1 && b < n && jb >= 0 && jb < (int64_t)n_bin;
    uint32_t key = in ? ((uint32_t)jb << 6) | lane : kKeyInvalid | lane;
    fetch(r + 1);
    const uint64_t valid = __ballot(key < kKeyInvalid);
    bool head = false, ok = false;
    uint32_t j = 0, end = lane;
    if (valid) {
      const uint32_t src = wave_sort_keys(key, lane, valid);
      wave_runs(key, lane, j, head, end);
      ok = key < kKeyInvalid;
      // the sample this lane now stands for (clamped into the chunk: what an invalid key loads is selected away below)
      const size_t bs = (size_t)min(t * 64 + (long)src, n - 1);
      double wv[kGrpCols] = {};
#pragma unroll
      for (uint32_t c = 0; c < kGrpCols; ++c)
        if (c < n_wcol) wv[c] = weight[(size_t)c * (size_t)wstride + bs];
      for (uint32_t i0 = 0; i0 < n_rec; i0 += 4) {
        double rv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) rv[u] = root[(size_t)rec[(size_t)min(i0 + u, n_rec - 1u) * 4u] * (size_t)ld + bs];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
          if (i0 + u >= n_rec) break;
          const uint32_t *e = rec + (size_t)(i0 + u) * 4u;
          const uint32_t wc = e[1];
          double wk = wv[0];
#pragma unroll
          for (uint32_t c = 1; c < kGrpCols; ++c) wk = wc == c ? wv[c] : wk;
          const double tk = n_wcol ? wk * rv[u] : rv[u];
          for (uint32_t ti = e[2]; ti < e[3]; ++ti) {
            const uint32_t sl = tslot[ti];
            double *o = stash + (size_t)(sl & ~kObsFirst) * 256u;
            const double p = tcoef[ti] * tk;
            *o = (sl & kObsFirst) ? p : *o + p;
          }
        }
      }
    }
    for (uint32_t g0 = 0; g0 < cn; g0 += kObsGroup) {
      double s[kObsGroup];
      if (valid) {
#pragma unroll
        for (uint32_t i = 0; i < kObsGroup; ++i) {
          const uint32_t cl = min(g0 + i, cn - 1u), a = colA[cl], c = colB[cl];
          double v = 0.0;
          if (a != kObsNone) {
            v = stash[(size_t)a * 256u];
            if (c != kObsNone) v = v * stash[(size_t)c * 256u];
          }
          s[i] = ok ? v : 0.0;                            // selected, never multiplied by 0
        }
        for (uint32_t d = 1; d < 64; d <<= 1) {           // segmented suffix scan, as in fdg_binned_partials
          const bool take = lane + d <= end;
          if (!__ballot(take)) break;
#pragma unroll
          for (uint32_t i = 0; i < kObsGroup; ++i) {
            const double up = __shfl_down(s[i], d);
            if (take) s[i] = s[i] + up;
          }
        }
      }
      for (uint32_t w = 0; w < kBinWaves; ++w) {          // the waves' turns, in wave order
        if (wave == w && head) {
#pragma unroll
          for (uint32_t i = 0; i < kObsGroup; ++i)
            if (g0 + i < cn) hist[(size_t)j * CS + g0 + i] = hist[(size_t)j * CS + g0 + i] + s[i];
        }
        bin_barrier();
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_bin * CS; i += 256) {
    const uint32_t jj = i / CS, cl = i % CS;
    if (cl < cn) slab[(size_t)jj * V + cl] = hist[i];
  }
}

// The reduce of both passes, over n_obs rows (the observables) or components (2 M, the frequency observables) and histogram rows jb
// (a bin, or bin * n_freq + frequency): d_obs[jb][m] and d_cov[jb][a][c] += the segments' partials [segment][jb][V], with
// fdg_binned_reduce's order (thread (q, c) adds the segments q, q + Q, ..., then the Q sums are added q = 0, 1, ...; Q = 256 / C).
// The column of a product goes to [a][c] and to its mirror [c][a]; rows or components without a term (bit m of rowlive clear) leave
// their column of d_obs and their rows and columns of d_cov alone.
__global__ void __launch_bounds__(256)
fdg_obs_reduce(const double *__restrict__ partial, uint32_t n_seg, long ncol, uint32_t n_obs, uint32_t V, uint32_t C, uint32_t rowlive,
               double *__restrict__ obs, double *__restrict__ cov) {
  __shared__ double sh[256];
  const uint32_t Q = 256u / C, q = threadIdx.x / C, cl = threadIdx.x % C;
  const long c = (long)blockIdx.x * C + cl;
  double s = 0.0;
  if (c < ncol)
    for (uint32_t sg = q; sg < n_seg; sg += Q) s = s + partial[(size_t)sg * (size_t)ncol + (size_t)c];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (q == 0 && c < ncol) {
    double t = sh[cl];
    for (uint32_t qq = 1; qq < Q && qq < n_seg; ++qq) t = t + sh[qq * C + cl];
    const size_t jb = (size_t)(c / V);
    const uint32_t v = (uint32_t)(c % V);
    if (v < n_obs) {
      if ((rowlive >> v) & 1u) obs[jb * n_obs + v] = obs[jb * n_obs + v] + t;
    } else {
      uint32_t a = 0, p = v - n_obs;                      // the p-th entry of the upper triangle, row by row
      while (p >= n_obs - a) { p -= n_obs - a; ++a; }
      const uint32_t cc = a + p;
      if (((rowlive >> a) & 1u) && ((rowlive >> cc) & 1u)) {
        double *m = cov + jb * n_obs * n_obs;
        const double up = m[a * n_obs + cc] + t;
        m[a * n_obs + cc] = up;
        if (cc != a) m[cc * n_obs + a] = m[cc * n_obs + a] + t;
      }
    }
  }
}

// ---- Frequency observables: linear combinations of the PROJECTED roots and their covariance (include/fdg.h:
// fdg_[mc_]accumulate_device_freq_observables) ----
// Per (sample, frequency) the components are z = (a_0 .. a_{M-1}, b_0 .. b_{M-1}), a_m and b_m the folds of coef[m][k] tre_k and
// coef[m][k] tim_k; the value columns are the 2 M components, then the products z_p z_q, p <= q, row by row of the upper triangle:
// V = 2 M + M (2 M + 1) columns.  fdg_obs_partials with 2 M rows and a histogram row per (bin, frequency): one workgroup per (segment of
// the chunk's tiles, slice of FS consecutive frequencies, slice of CS consecutive columns), the slice's histogram (n_bin x FS x CS
// doubles) in LDS, the tiles dealt to the four waves as there.
//  * A wave sorts its tile's lanes by (bin, lane) once, before any root is touched; a lane then forms the values of the sample whose
//    key it holds.  Unlike a bin, every frequency of the slice takes the sample: the frequencies are walked one after the other with
//    the same keys and runs.
//  * Per frequency the slice's root records are walked in ascending k: t = w_g(k) root_k as the moments pass forms it, x = tau / beta
//    and (s, c) = matsubara_phase_of(x, mult[f]) as the projection pass forms them (a record whose pair of time labels is the record's
//    before it keeps that phase: the same operands, the same bits), tre = t c, tim = t s; every term folds coef * tre or coef * tim
//    into its component's word of the lane's LDS stash ([component of the slice][256 lanes]).
//  * The columns are scanned kObsGroup at a time and the waves add their run heads in wave order, as in fdg_obs_partials.
//  * Chunks and segments chain through partial [segment][bin][frequency][V], summed in segment order by fdg_obs_reduce over the
//    2 M components.
// utab and dtab: the observables' tables with the bracketed parts (stated there), a header per COLUMN slice.
constexpr uint32_t kFobsRec = 6;
constexpr uint32_t kFobsSame = 0x80000000u;
constexpr uint32_t kFobsIm = 0x40000000u;

__global__ void __launch_bounds__(256)
fdg_fobs_partials(const double *__restrict__ root, long ld, long n, const int32_t *__restrict__ bins, int32_t bin_base, uint32_t n_bin,
                  const double *__restrict__ weight, long wstride, uint32_t n_wcol, const double *__restrict__ T, long ts, long tc,
                  double beta, uint32_t n_freq, uint32_t FS, uint32_t n_fslice, uint32_t V, uint32_t CS, uint32_t n_cslice, long seg_tiles,
                  double *__restrict__ partial, int first, const uint32_t *__restrict__ utab, const double *__restrict__ dtab) {
  extern __shared__ double hist[];                        // [bin][FS][CS], then the stash [row][256]
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t n_grp = n_fslice * n_cslice, grp = blockIdx.x % n_grp, seg = blockIdx.x / n_grp;
  const uint32_t cslice = grp % n_cslice, fslice = grp / n_cslice;
  const uint32_t c0 = cslice * CS, cn = min(CS, V - c0), fb = fslice * FS, fn = min(FS, n_freq - fb);
  const uint32_t *hdr = utab + (size_t)cslice * 4u;
  const uint32_t n_rec = hdr[1];
  const uint32_t *colA = utab + hdr[2], *colB = colA + CS, *rec = colB + CS, *tslot = rec + (size_t)n_rec * kFobsRec;
  const double *tcoef = dtab + hdr[3];
  const uint32_t per = n_bin * FS * CS;                   // words of the histogram in LDS
  double *stash = hist + per + threadIdx.x;
  double *slab = partial + (size_t)seg * n_bin * n_freq * V;
  // (j, fl, cl) of LDS word i, and its place in the slab
  auto slab_at = [&](uint32_t i, bool &live) {
    const uint32_t cl = i % CS, fl = (i / CS) % FS, j = i / (CS * FS);
    live = cl < cn && fl < fn;
    return ((size_t)j * n_freq + fb + fl) * V + c0 + cl;
  };
  for (uint32_t i = threadIdx.x; i < per; i += 256) {
    bool live;
    const size_t at = slab_at(i, live);
    hist[i] = (first || !live) ? 0.0 : slab[at];
  }
  __syncthreads();
  const SegTiles sg = seg_tiles_of(n, seg, seg_tiles);
  const long t0 = sg.t0, t1 = sg.t1, rounds = sg.rounds;
  int32_t bin_n;
  auto fetch = [&](long r) {                              // the bin of this lane's sample of round r, one round ahead (index clamped)
    const long b = min((t0 + r * (long)kBinWaves + wave) * 64 + lane, n - 1);
    bin_n = bins ? bins[b] : bin_base;
  };
  fetch(0);
  for (long r = 0; r < rounds; ++r) {
    const long t = t0 + r * (long)kBinWaves + wave, b = t * 64 + lane;
    const int64_t jb = (int64_t)bin_n - (int64_t)bin_base;
    const bool in = t < t1 && b < n && jb >= 0 && jb < (int64_t)n_bin;
    uint32_t key = in ? ((uint32_t)jb << 6) | lane : kKeyInvalid | lane;
    fetch(r + 1);
    const uint64_t valid = __ballot(key < kKeyInvalid);
    bool head = false, ok = false;
    uint32_t j = 0, end = lane;
    size_t bs = 0;
    double wv[kGrpCols] = {};
    if (valid) {
      const uint32_t src = wave_sort_keys(key, lane, valid);
      wave_runs(key, lane, j, head, end);
      ok = key < kKeyInvalid;
      // the sample this lane now stands for (clamped into the chunk: what an invalid key loads is selected away below)
      bs = (size_t)min(t * 64 + (long)src, n - 1);
#pragma unroll
      for (uint32_t c = 0; c < kGrpCols; ++c)
        if (c < n_wcol) wv[c] = weight[(size_t)c * (size_t)wstride + bs];
    }
    for (uint32_t fl = 0; fl < fn; ++fl) {
      if (valid) {
        const double mult = dtab[fb + fl];
        double ps = 0.0, pc = 0.0;                        // the phase of the last pair of time labels
        for (uint32_t i0 = 0; i0 < n_rec; i0 += 4) {
          double rv[4];
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) rv[u] = root[(size_t)rec[(size_t)min(i0 + u, n_rec - 1u) * kFobsRec] * (size_t)ld + bs];
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) {
            if (i0 + u >= n_rec) break;
            const uint32_t *e = rec + (size_t)(i0 + u) * kFobsRec;
            const uint32_t wc = e[1] & ~kFobsSame;
            double wk = wv[0];
#pragma unroll
            for (uint32_t c = 1; c < kGrpCols; ++c) wk = wc == c ? wv[c] : wk;
            const double tk = n_wcol ? wk * rv[u] : rv[u];
            if (!(e[1] & kFobsSame)) {
              const double ti = T[(long)bs * ts + (long)e[4] * tc], to = T[(long)bs * ts + (long)e[5] * tc];
              const double tau = to - ti;
              const double x = ok ? tau / beta : 0.0;
              matsubara_phase_of(x, mult, ps, pc);
            }
            const double tre = tk * pc, tim = tk * ps;
            for (uint32_t tt = e[2]; tt < e[3]; ++tt) {
              const uint32_t sl = tslot[tt];
              double *o = stash + (size_t)(sl & ~(kObsFirst | kFobsIm)) * 256u;
              const double p = tcoef[tt] * ((sl & kFobsIm) ? tim : tre);
              *o = (sl & kObsFirst) ? p : *o + p;
            }
          }
        }
      }
      for (uint32_t g0 = 0; g0 < cn; g0 += kObsGroup) {
        double s[kObsGroup];
        if (valid) {
#pragma unroll
          for (uint32_t i = 0; i < kObsGroup; ++i) {
            const uint32_t cl = min(g0 + i, cn - 1u), a = colA[cl], c = colB[cl];
            double v = 0.0;
            if (a != kObsNone) {
              v = stash[(size_t)a * 256u];
              if (c != kObsNone) v = v * stash[(size_t)c * 256u];
            }
            s[i] = ok ? v : 0.0;                          // selected, never multiplied by 0
          }
          for (uint32_t d = 1; d < 64; d <<= 1) {         // segmented suffix scan, as in fdg_binned_partials
            const bool take = lane + d <= end;
            if (!__ballot(take)) break;
#pragma unroll
            for (uint32_t i = 0; i < kObsGroup; ++i) {
              const double up = __shfl_down(s[i], d);
              if (take) s[i] = s[i] + up;
            }
          }
        }
        for (uint32_t w = 0; w < kBinWaves; ++w) {        // the waves' turns, in wave order
          if (wave == w && head) {
            double *hw = hist + ((size_t)j * FS + fl) * CS + g0;
#pragma unroll
            for (uint32_t i = 0; i < kObsGroup; ++i)
              if (g0 + i < cn) hw[i] = hw[i] + s[i];
          }
          bin_barrier();
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < per; i += 256) {
    bool live;
    const size_t at = slab_at(i, live);
    if (live) slab[at] = hist[i];
  }
}

// ---- VEGAS importance sampling: the sampler, the training pass (include/fdg.h: fdg_vegas_sample_device, fdg_accumulate_device_vegas) ----
// The map's statements (vegas_cell, vegas_draw, discrete_pick, strat_cube, polar_point) are fdg_sampler.h's.

// What the instances of the sampler take beside the map and the outputs, each only where its flag is set (kernel arguments, by value).
// The discrete variable: its cdf, the base of bin[], its table ext [n_bin][n_ext] and the table's columns.
struct VegasDiscArgs {
  const double *cdf;
  uint32_t n_bin;
  int32_t bin_base;
  const double *ext;
  uint32_t n_ext;
  SamplerExtCols ecol;
  int32_t *bin;
};
// The weight groups: bit d of m[g] set = variable d belongs to group g; group g's jacobian goes to jac[g * jstride + b].
struct VegasGroupArgs {
  uint64_t m[FDG_WEIGHT_GROUP_MAX];
  uint32_t n;
  long jstride;
};
// The strata, the prefix sums start[0 .. H] of the samples per hypercube, and cube[b] to write.
struct VegasStratArgs {
  VegasStrat sv;
  const int64_t *start;
  int32_t *cube;
};

// The one sampler, one lane per sample in a grid-stride loop.  The continuous variables of sample b in order: each through the map
// (vegas_draw), its value to its column of x, its factor f = G * wd into the jacobian (a left fold), its cell to cell[] when given.
// DISC: one discrete variable behind them (discrete_pick): bin[b], row j of ext to the columns ecol, every jacobian divided by p.
// POLAR: groups of variables read as (k, phi) or (k, theta, phi).  The drawn values of the grouped variables wait in LDS (one slot of
//   256 lanes per grouped variable, in ascending d, dynamic: 2 KiB each) until the fold over all variables is done, then every group
//   gives its columns and its factors of the jacobian (k, or k k sin theta), in the order of the array.  A lane touches its own LDS
//   words only, so no barrier.
// GRP: one jacobian per weight group, each the same fold over the variables and polar groups of its mask only (1.0 * f = f exactly:
//   a group's first factor enters as the plain fold's does; a mask holds all of a polar group's variables or none: its first one
//   decides).  Every variable is drawn once, and x, bin and cell are written by the very statements of the ungrouped instances.
// STRAT (no discrete variable): the lane finds its hypercube h (strat_cube, cube[b]), peels h's digits variable by variable and draws
//   every variable inside its stratum; every jacobian is multiplied by fac_h = n_total / (H * n_h) last.
template <bool POLAR, bool GRP, bool STRAT, bool DISC>
__global__ void __launch_bounds__(256)
fdg_vegas_sample(const double *__restrict__ grid, uint32_t D, uint32_t G, SamplerCols col, uint64_t seed, uint64_t off, double *__restrict__ x,
                 long xs, long xc, double *__restrict__ jac, int32_t *__restrict__ cell, long n, ArgIf<DISC, VegasDiscArgs> da,
                 ArgIf<POLAR, SamplerPolar> pol, ArgIf<GRP, VegasGroupArgs> ga, ArgIf<STRAT, VegasStratArgs> sa) {
  static_assert(!(STRAT && DISC), "the stratified calls take no discrete variable");
  constexpr int NG = GRP ? FDG_WEIGHT_GROUP_MAX : 1;
  [[maybe_unused]] double *stash = nullptr;
  if constexpr (POLAR) {
    extern __shared__ double polar_stash[];
    stash = polar_stash;
  }
  [[maybe_unused]] double n_total = 0.0;
  if constexpr (STRAT) n_total = (double)sa.start[sa.sv.H];
  for (long b = blockIdx.x * 256L + threadIdx.x; b < n; b += (long)gridDim.x * 256L) {
    const uint64_t sample = off + (uint64_t)b;
    [[maybe_unused]] double fac = 1.0;                     // STRAT: fac_h of this lane's hypercube
    [[maybe_unused]] uint32_t rem = 0;                     // STRAT: the hypercube's digits not yet peeled
    if constexpr (STRAT) {
      int64_t n_h;
      rem = strat_cube(sa.start, sa.sv.H, (int64_t)sample, n_h);
      sa.cube[b] = (int32_t)rem;
      fac = n_total / ((double)sa.sv.H * (double)n_h);
    }
    double jb = 0.0;
    [[maybe_unused]] double jg[NG];
    if constexpr (GRP) {
#pragma unroll
      for (int g = 0; g < NG; ++g) jg[g] = 1.0;
    }
    [[maybe_unused]] uint32_t slot = 0;
    for (uint32_t d = 0; d < D; ++d) {
      uint32_t s = 0, ns = 1;
      if constexpr (STRAT) {
        ns = sa.sv.n[d];
        s = rem % ns;
        rem /= ns;
      }
      uint32_t c;
      double f;
      const double v = vegas_draw<STRAT>(grid, d, G, sample, seed, s, ns, c, f);
      bool stashed = false;
      if constexpr (POLAR) stashed = (pol.grouped >> d) & 1u;
      if (stashed) stash[(slot++) * 256u + threadIdx.x] = v;
      else x[b * xs + (long)col.c[d] * xc] = v;
      jb = d ? jb * f : f;
      if constexpr (GRP) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
          if ((uint32_t)g < ga.n && ((ga.m[g] >> d) & 1u)) jg[g] = jg[g] * f;
      }
      if (cell) cell[(size_t)d * (size_t)n + (size_t)b] = (int32_t)c;
    }
    if constexpr (POLAR) {
      for (uint32_t g = 0; g < pol.n; ++g) {
        const uint32_t var = pol.var[g];
        const bool three = pol.dim[g] == 3;
        const double *v = stash + (size_t)__popcll(pol.grouped & ((1ull << var) - 1ull)) * 256u + threadIdx.x;
        double *xb = x + b * xs;
        const double k = v[0];
        double c0, c1, c2, st;
        polar_point(three, k, v[256], v[three ? 512 : 256], c0, c1, c2, st);
        xb[(long)pol.col[g][0] * xc] = c0;
        xb[(long)pol.col[g][1] * xc] = c1;
        if (three) xb[(long)pol.col[g][2] * xc] = c2;
        jb = jb * k;
        if (three) {
          jb = jb * k;
          jb = jb * st;
        }
        if constexpr (GRP) {
#pragma unroll
          for (int h = 0; h < NG; ++h)
            if ((uint32_t)h < ga.n && ((ga.m[h] >> var) & 1u)) {
              jg[h] = jg[h] * k;
              if (three) {
                jg[h] = jg[h] * k;
                jg[h] = jg[h] * st;
              }
            }
        }
      }
    }
    [[maybe_unused]] double p = 1.0;                       // DISC: the probability of the value drawn; shared by every group
    if constexpr (DISC) {
      const uint32_t j = discrete_pick(da.cdf, da.n_bin, sample, D, seed, p);
      da.bin[b] = (int32_t)j + da.bin_base;
      for (uint32_t e = 0; e < da.n_ext; ++e) x[b * xs + (long)da.ecol.c[e] * xc] = da.ext[(size_t)j * da.n_ext + e];
    }
    auto out = [&](double j) { return DISC ? j / p : STRAT ? j * fac : j; };
    if constexpr (GRP) {
#pragma unroll
      for (int g = 0; g < NG; ++g)
        if ((uint32_t)g < ga.n) jac[(size_t)g * (size_t)ga.jstride + (size_t)b] = out(jg[g]);
    } else {
      jac[b] = out(jb);
    }
  }
}

// t = w (c_0 r_0 + c_1 r_1 + ...) of the sample at bb of the chunk, over the n_live roots kidx[] that exist, a left fold (coef null: plain
// sum; weight null: t = the sum).  What both training passes below square.
__device__ __forceinline__ double vegas_term(const double *__restrict__ root, long ld, size_t bb, const double *__restrict__ weight,
                                             const uint32_t *__restrict__ kidx, const double *__restrict__ coef, uint32_t n_live) {
  double sum = 0.0;
  for (uint32_t i = 0; i < n_live; ++i) {
    const double rk = root[(size_t)kidx[i] * (size_t)ld + bb];
    const double term = coef ? coef[i] * rk : rk;
    sum = i ? sum + term : term;
  }
  return weight ? weight[bb] * sum : sum;
}

// The training passes' view of the weight groups: the lists kidx / coef are sorted by (group, root) and gstart[g] .. gstart[g + 1]
// bounds group g's part of them (empty: the group has no root that exists).  vegas_group_term: t_g = w_g s_g of the sample at bb,
// s_g the left fold over the group's roots, ascending; the caller squares it.
__device__ __forceinline__ double vegas_group_term(const double *__restrict__ root, long ld, size_t bb, const double *__restrict__ weight,
                                                   long wstride, const uint32_t *__restrict__ kidx, const double *__restrict__ coef,
                                                   const uint32_t *__restrict__ gstart, uint32_t g) {
  const uint32_t i0 = gstart[g], i1 = gstart[g + 1u];
  return vegas_term(root, ld, bb, weight + (size_t)g * (size_t)wstride, kidx + i0, coef ? coef + i0 : nullptr, i1 - i0);
}

// The groups that train each variable (a kernel argument, by value): bit g of g[d] set = variable d is in the mask of group g and
// the group has a root that exists.
struct VegasVarGroups { uint8_t g[FDG_VEGAS_DIM_MAX]; };

// The training pass over a chunk's roots (root k of sample b at root[k * ld + b], b < n): hist[d][c] += v(b) for every variable d, c = the
// cell of sample off + b in d, v = (w (c_0 r_0 + c_1 r_1 + ...))^2 over the n_live roots kidx[] that exist (coef null: plain sum).
// One workgroup per (segment of the chunk's tiles, slice of DS variables), the slice's histograms (DS x G doubles) in LDS.
//  * In a round the four waves form v for one tile each (wave w the tile 4 r + w, as the binned pass deals them) and leave it in LDS.
//  * Every wave then walks the round's tiles in tile order for ITS variables of the slice (dd = wave, wave + 4, ...): it recomputes
//    the cell from the counter, sorts the lanes by (cell, lane), sums v over every run of equal cells (the binned pass's segmented scan,
//    one value instead of RS) and the run heads add into the histogram.  A histogram word is only ever touched by one wave, in
//    program order: per (variable, cell) the tiles are added in tile order, and there is nothing to wait for but the v exchange
//    (two buffers, one barrier per round).
//  * Chunks and segments chain as in the binned pass: partial [segment][variable][cell], summed in segment order by fdg_binned_reduce.
// Lanes past n are selected away (key invalid, v = 0 never enters a sum); no float atomics.
// BINNED (the calls with a discrete variable): a sample whose bin lies outside [bin_base, bin_base + n_bin) is selected away like a lane
// past n.  The wave that forms v leaves -1 for it in the exchange buffer (v is a square: never negative), and the waves that walk the
// tile give such a lane the invalid key.  With every bin in range no key changes: the sums are those of the unbinned instance.
// GRP (the grouped calls): the wave that forms v leaves q_g = (w_g s_g)^2 for each of the NG groups, the exchange buffer
// [2][kBinWaves][NG][64] (the lanes innermost: a wave reads one group's 64 words at unit stride); a walking wave folds the q_g of its
// variable's groups (vgm, ascending g) into v before the sort, and skips a variable that no group with a root owns.  The marker
// survives the fold: the q_g of a lane are all -1 or all squares.
// STRAT (the stratified calls): the cell is vegas_cell_strat's, the stratum the digit of cube[b] in the variable; a sample whose
// hypercube lies outside [0, H) is selected away like a lane past n.  Nothing else differs, and with one stratum per variable and
// cube = 0 every key is the unstratified instance's.
template <int BINNED, bool GRP = false, bool STRAT = false>
__global__ void __launch_bounds__(256)
fdg_vegas_partials(const double *__restrict__ root, long ld, long n, const double *__restrict__ weight, const uint32_t *__restrict__ kidx,
                   const double *__restrict__ coef, uint32_t n_live, uint64_t seed, uint64_t off, uint32_t D, uint32_t G, uint32_t DS,
                   uint32_t n_slice, long seg_tiles, double *__restrict__ partial, int first, const int32_t *__restrict__ bins,
                   int32_t bin_base, uint32_t n_bin, const uint32_t *__restrict__ gstart, uint32_t NG, long wstride, VegasVarGroups vgm,
                   const int32_t *__restrict__ cube, VegasStrat sv) {
  extern __shared__ double hist[];                        // [DS][G], then v of the round's tiles [2][kBinWaves][64] (GRP: x NG)
  const uint32_t vtile = GRP ? NG * 64u : 64u;            // words of one tile in the exchange buffer
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t slice = blockIdx.x % n_slice, seg = blockIdx.x / n_slice;
  const uint32_t d0 = slice * DS, dn = min(DS, D - d0);
  double *vbuf = hist + (size_t)DS * G;
  double *slab = partial + ((size_t)seg * D + d0) * G;
  for (uint32_t i = threadIdx.x; i < dn * G; i += 256) hist[i] = first ? 0.0 : slab[i];
  __syncthreads();
  const SegTiles sg = seg_tiles_of(n, seg, seg_tiles);
  const long t0 = sg.t0, t1 = sg.t1, rounds = sg.rounds;
  for (long r = 0; r < rounds; ++r) {
    {
      const long t = t0 + r * (long)kBinWaves + wave, b = t * 64 + lane;
      bool in = t < t1 && b < n;
      const size_t bb = (size_t)min(b, n - 1);            // clamped into the chunk; what it loads is used only where `in`
      if (BINNED) {
        const int64_t jb = (int64_t)bins[bb] - (int64_t)bin_base;
        in = in && jb >= 0 && jb < (int64_t)n_bin;
      }
      const double out = (BINNED && t < t1 && b < n) ? -1.0 : 0.0;
      double *vb = vbuf + ((r & 1) * kBinWaves + wave) * vtile + lane;
      if constexpr (GRP) {
        for (uint32_t g = 0; g < NG; ++g) {
          const double tw = vegas_group_term(root, ld, bb, weight, wstride, kidx, coef, gstart, g);
          vb[g * 64u] = in ? tw * tw : out;
        }
      } else {
        const double tw = vegas_term(root, ld, bb, weight, kidx, coef, n_live);
        vb[0] = in ? tw * tw : out;
      }
    }
    __syncthreads();
    for (uint32_t tt = 0; tt < kBinWaves; ++tt) {
      const long t = t0 + r * (long)kBinWaves + tt, b = t * 64 + lane;
      if (t >= t1) break;
      const double *vb = vbuf + ((r & 1) * kBinWaves + tt) * vtile + lane;
      double v = GRP ? 0.0 : vb[0];
      uint32_t hc = 0;                                     // STRAT: this lane's hypercube (index clamped into the chunk)
      if constexpr (STRAT) hc = (uint32_t)cube[(size_t)min(b, n - 1)];
      for (uint32_t dd = wave; dd < dn; dd += kBinWaves) {
        if constexpr (GRP) {
          const uint32_t owners = vgm.g[d0 + dd];
          if (!owners) continue;
          bool any = false;
          for (uint32_t g = 0; g < NG; ++g)
            if ((owners >> g) & 1u) {
              const double q = vb[g * 64u];
              v = any ? v + q : q;
              any = true;
            }
        }
        double y;
        uint32_t c;
        if constexpr (STRAT) c = vegas_cell_strat(off + (uint64_t)b, d0 + dd, seed, G, hc / sv.div[d0 + dd] % sv.n[d0 + dd], sv.n[d0 + dd], y);
        else c = vegas_cell(off + (uint64_t)b, d0 + dd, seed, G, y);
        uint32_t key = (b < n && !(STRAT && hc >= sv.H) && !(BINNED && v < 0.0)) ? (c << 6) | lane : kKeyInvalid | lane;
        const uint64_t valid = __ballot(key < kKeyInvalid);
        if (!valid) continue;
        const uint32_t src = wave_sort_keys(key, lane, valid);
        uint32_t j, end;
        bool head;
        wave_runs(key, lane, j, head, end);
        double s = __shfl(v, (int)src);
        for (uint32_t dist = 1; dist < 64; dist <<= 1) {   // segmented suffix scan, as in fdg_binned_partials
          const bool take = lane + dist <= end;
          if (!__ballot(take)) break;
          const double up = __shfl_down(s, dist);
          if (take) s = s + up;
        }
        if (head) hist[dd * G + j] = hist[dd * G + j] + s;
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < dn * G; i += 256) slab[i] = hist[i];
}

// The training pass of the discrete variable: hbin[j] += v(b) over the samples b of the chunk whose bin is j + bin_base, v as above.
// The variable is one more key column of the pass above whose key is read from `bins`, but its histogram has up to FDG_BIN_MAX cells
// (128 KiB), so it is a slice of its own: one workgroup per segment of the chunk's tiles, the whole histogram (n_bin doubles) in LDS,
// and with one variable there is nothing to deal over the waves but the tiles, so the round is fdg_binned_partials': wave w forms v for
// tile 4 r + w, sorts its lanes by (bin, lane), sums every run of equal bins, and the run heads add into the histogram in the waves'
// turns, wave 0 first: per bin, tiles are added in tile order.  Chunks and segments chain through partial [segment][bin], summed in
// segment order by fdg_binned_reduce.  Out-of-range bins and lanes past n are selected away (key invalid); no float atomics.
// GRP (the grouped calls): v = the left fold, over the groups with a root that exists, ascending, of q_g = (w_g s_g)^2.
template <bool GRP = false>
__global__ void __launch_bounds__(256)
fdg_vegas_bin_partials(const double *__restrict__ root, long ld, long n, const int32_t *__restrict__ bins, int32_t bin_base, uint32_t n_bin,
                       const double *__restrict__ weight, const uint32_t *__restrict__ kidx, const double *__restrict__ coef, uint32_t n_live,
                       long seg_tiles, double *__restrict__ partial, int first, const uint32_t *__restrict__ gstart, uint32_t NG,
                       long wstride) {
  extern __shared__ double hist[];                        // [n_bin]
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t seg = blockIdx.x;
  double *slab = partial + (size_t)seg * n_bin;
  for (uint32_t i = threadIdx.x; i < n_bin; i += 256) hist[i] = first ? 0.0 : slab[i];
  __syncthreads();
  const SegTiles sg = seg_tiles_of(n, seg, seg_tiles);
  const long t0 = sg.t0, t1 = sg.t1, rounds = sg.rounds;
  // this lane's sample of round r, formed one round ahead (indices clamped into the chunk; used only where the sample is `in`)
  int32_t bin_n;
  double t_n = 0.0;
  auto fetch = [&](long r) {
    const size_t bb = (size_t)min((t0 + r * (long)kBinWaves + wave) * 64 + lane, n - 1);
    bin_n = bins[bb];
    if constexpr (GRP) {                                  // (t_n holds the folded squares themselves)
      bool any = false;
      for (uint32_t g = 0; g < NG; ++g) {
        if (gstart[g] == gstart[g + 1u]) continue;
        const double tw = vegas_group_term(root, ld, bb, weight, wstride, kidx, coef, gstart, g), q = tw * tw;
        t_n = any ? t_n + q : q;
        any = true;
      }
    } else {
      t_n = vegas_term(root, ld, bb, weight, kidx, coef, n_live);
    }
  };
  fetch(0);
  for (long r = 0; r < rounds; ++r) {
    const long t = t0 + r * (long)kBinWaves + wave, b = t * 64 + lane;
    const int64_t jb = (int64_t)bin_n - (int64_t)bin_base;
    const bool in = t < t1 && b < n && jb >= 0 && jb < (int64_t)n_bin;
    uint32_t key = in ? ((uint32_t)jb << 6) | lane : kKeyInvalid | lane;
    const double v = in ? (GRP ? t_n : t_n * t_n) : 0.0;
    fetch(r + 1);
    const uint64_t valid = __ballot(key < kKeyInvalid);
    double s = 0.0;
    bool head = false;
    uint32_t j = 0;
    if (valid) {
      const uint32_t src = wave_sort_keys(key, lane, valid);
      uint32_t end;
      wave_runs(key, lane, j, head, end);
      s = __shfl(v, (int)src);
      for (uint32_t dist = 1; dist < 64; dist <<= 1) {     // segmented suffix scan, as in fdg_binned_partials
        const bool take = lane + dist <= end;
        if (!__ballot(take)) break;
        const double up = __shfl_down(s, dist);
        if (take) s = s + up;
      }
    }
    for (uint32_t w = 0; w < kBinWaves; ++w) {            // the waves' turns, in wave order
      if (wave == w && head) hist[j] = hist[j] + s;
      bin_barrier();
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_bin; i += 256) slab[i] = hist[i];
}

// The projection pass over a chunk's roots (fdg_[mc_]accumulate_device_matsubara): for the samples b of bin j, the roots k and the
// frequencies f, with t = w_b root_k(b), x = (T[b][tout_k] - T[b][tin_k]) / beta and (s, c) = matsubara_phase_of(x, mult[f]),
//     hist[0][j][f][k] += t c;  hist[1] += t s;  hist[2] += (t c)(t c);  hist[3] += (t s)(t s).
// One workgroup per (segment of the chunk's tiles, slice of RS roots, slice of FS frequencies), the slice's four histograms
// (4 x n_bin x FS x RS doubles) in LDS.  The slice's (root, frequency) items are dealt over the waves, item kk + RS fl to wave
// (kk + RS fl) % nw, and every wave walks ALL the segment's tiles in tile order for its items, as the training pass walks its
// variables: a histogram word is only ever touched by one wave, in program order, so per (bin, frequency, root) the tiles are added
// in tile order with no barrier inside the loop.  Per tile a wave sorts its lanes by (bin, lane) once for all its items (not at all
// when the tile lies in one bin), forms t and x at the sample's own lane and moves them to the sorted position; then per item the
// phase, the four terms, the binned pass's segmented scan over every run of equal bins, and the run heads add into the histograms.
// Lanes past n or with a bin out of range carry the invalid key: they belong to no run and enter no sum.
// HSPLIT (four histograms of one (root, frequency) do not fit the LDS: n_bin > 4096): RS = FS = 1 and every slice gets four
// workgroups, one per histogram.  Chunks and segments chain through partial [segment][histogram][bin][frequency][root].
// tab: mult[FDG_MATSUBARA_FREQ_MAX] doubles, then tin[R], tout[R] (0-based components of T) as int32.
// GRP (the grouped calls with more than one group): t = w_g(k) root_k, the weight column of the root's group (rgrp[k], the head of
// gtab above); a wave loads one column per distinct group among its KW roots, so roots of one group load what the ungrouped pass does.
template <int KW, bool HSPLIT, bool GRP = false>
__global__ void __launch_bounds__(256)
fdg_matsubara_partials(const double *__restrict__ root, long ld, long n, const int32_t *__restrict__ bins, int32_t bin_base, uint32_t n_bin,
                       const double *__restrict__ weight, const double *__restrict__ T, long ts, long tc, const double *__restrict__ tab,
                       double beta, uint32_t n_freq, uint32_t R, uint32_t RS, uint32_t FS, uint32_t n_fslice, long seg_tiles,
                       double *__restrict__ partial, int first, const uint32_t *__restrict__ rgrp, long wstride) {
  extern __shared__ double hist[];                        // [histogram][bin][FS][RS]
  constexpr uint32_t NH = HSPLIT ? 1 : 4;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const uint32_t n_rslice = (R + RS - 1) / RS, n_grp = n_rslice * n_fslice * (HSPLIT ? 4u : 1u);
  const uint32_t grp = blockIdx.x % n_grp, seg = blockIdx.x / n_grp;
  const uint32_t h0 = HSPLIT ? grp / (n_rslice * n_fslice) : 0u;            // HSPLIT: the histogram this workgroup sums
  const uint32_t fslice = (grp / n_rslice) % n_fslice, rslice = grp % n_rslice;
  const uint32_t k0 = rslice * RS, kn = min(RS, R - k0), fb = fslice * FS, fn = min(FS, n_freq - fb);
  const size_t ncol = (size_t)n_bin * n_freq * R;
  double *slab = partial + ((size_t)seg * 4u + h0) * ncol;
  const uint32_t per = n_bin * FS * RS;                   // words of one histogram in LDS
  // (hh, j, fl, kk) of LDS word i, and its place in the slab
  auto slab_at = [&](uint32_t i, bool &live) {
    const uint32_t kk = i % RS, fl = (i / RS) % FS, j = (i / (RS * FS)) % n_bin, hh = i / per;
    live = kk < kn && fl < fn;
    return (size_t)hh * ncol + ((size_t)j * n_freq + fb + fl) * R + k0 + kk;
  };
  for (uint32_t i = threadIdx.x; i < NH * per; i += blockDim.x) {
    bool live;
    const size_t at = slab_at(i, live);
    hist[i] = (first || !live) ? 0.0 : slab[at];
  }
  __syncthreads();
  const SegTiles sg = seg_tiles_of(n, seg, seg_tiles);
  // this wave's items: the roots kk0 + nw m (m < KW) at every frequency when a slice has at least nw roots, else one root at the
  // frequencies f0, f0 + fstep, ...
  const uint32_t kk0 = RS >= nw ? wave : wave % RS, f0 = RS >= nw ? 0u : wave / RS, fstep = RS >= nw ? 1u : nw / RS;
  const int32_t *tio = (const int32_t *)(tab + FDG_MATSUBARA_FREQ_MAX);
  long off_in[KW], off_out[KW];
  size_t col[KW], wcol[KW] = {};
  int wfrom[KW] = {};                                      // GRP: the earliest of the wave's roots with root m's group (it loads the column)
#pragma unroll
  for (int m = 0; m < KW; ++m) {
    const uint32_t k = min(k0 + kk0 + nw * (uint32_t)m, R - 1u);            // clamped: what it loads is used only for kk < kn
    col[m] = (size_t)k * (size_t)ld;
    if constexpr (GRP) {
      wcol[m] = (size_t)rgrp[k] * (size_t)wstride;
      wfrom[m] = m;
#pragma unroll
      for (int e = m - 1; e >= 0; --e)
        if (wcol[e] == wcol[m]) wfrom[m] = e;
    }
    off_in[m] = (long)tio[k] * tc;
    off_out[m] = (long)tio[R + k] * tc;
  }
  if (kk0 < kn && f0 < fn) {
    // this lane's sample of the next tile, loaded one tile ahead (indices clamped into the chunk; used only where the sample is `in`)
    int32_t bin_n;
    double w_n[GRP ? KW : 1] = {}, r_n[KW], ti_n[KW], to_n[KW];
    auto fetch = [&](long t) {
      const size_t bb = (size_t)min(t * 64 + (long)lane, n - 1);
      bin_n = bins ? bins[bb] : bin_base;
      if constexpr (!GRP) w_n[0] = weight ? weight[bb] : 1.0;
#pragma unroll
      for (int m = 0; m < KW; ++m) {
        if constexpr (GRP)
          if (wfrom[m] == m) w_n[m] = weight[wcol[m] + bb];
        r_n[m] = root[col[m] + bb];
        ti_n[m] = T[(long)bb * ts + off_in[m]];
        to_n[m] = T[(long)bb * ts + off_out[m]];
      }
    };
    fetch(sg.t0);
    for (long t = sg.t0; t < sg.t1; ++t) {
      const long b = t * 64 + lane;
      const int64_t jb = (int64_t)bin_n - (int64_t)bin_base;
      const bool in = b < n && jb >= 0 && jb < (int64_t)n_bin;
      uint32_t key = in ? ((uint32_t)jb << 6) | lane : kKeyInvalid | lane;
      double tv[KW], xv[KW];
#pragma unroll
      for (int m = 0; m < KW; ++m) {
        const double tau = to_n[m] - ti_n[m];
        double wk = w_n[0];
        if constexpr (GRP) {
#pragma unroll
          for (int e = 1; e <= m; ++e) wk = wfrom[m] == e ? w_n[e] : wk;
        }
        tv[m] = in ? wk * r_n[m] : 0.0;                   // selected, never multiplied by 0
        xv[m] = in ? tau / beta : 0.0;
      }
      fetch(min(t + 1, sg.t1 - 1));
      const uint64_t valid = __ballot(key < kKeyInvalid);
      if (!valid) continue;
      const uint32_t src = wave_sort_keys(key, lane, valid);
      uint32_t j, end;
      bool head;
      wave_runs(key, lane, j, head, end);
#pragma unroll
      for (int m = 0; m < KW; ++m) {
        const uint32_t kk = kk0 + nw * (uint32_t)m;
        if (kk >= kn) break;
        const double ts_ = __shfl(tv[m], (int)src), xs = __shfl(xv[m], (int)src);
        for (uint32_t fl = f0; fl < fn; fl += fstep) {
          double s, c;
          matsubara_phase_of(xs, tab[fb + fl], s, c);
          const double tre = ts_ * c, tim = ts_ * s;
          double v[NH];                                   // the squares rounded before they are added (no fma: -ffp-contract=off)
          if constexpr (HSPLIT) {
            v[0] = h0 == 0 ? tre : h0 == 1 ? tim : h0 == 2 ? tre * tre : tim * tim;
          } else {
            v[0] = tre;
            v[1] = tim;
            v[2] = tre * tre;
            v[3] = tim * tim;
          }
          for (uint32_t d = 1; d < 64; d <<= 1) {         // segmented suffix scan, as in fdg_binned_partials
            const bool take = lane + d <= end;
            if (!__ballot(take)) break;
#pragma unroll
            for (uint32_t hh = 0; hh < NH; ++hh) {
              const double up = __shfl_down(v[hh], d);
              if (take) v[hh] = v[hh] + up;
            }
          }
          if (head) {
            double *hw = hist + ((size_t)j * FS + fl) * RS + kk;
#pragma unroll
            for (uint32_t hh = 0; hh < NH; ++hh) hw[(size_t)hh * per] = hw[(size_t)hh * per] + v[hh];
          }
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < NH * per; i += blockDim.x) {
    bool live;
    const size_t at = slab_at(i, live);
    if (live) slab[at] = hist[i];
  }
}

// ---- Per-hypercube moments of the stratified calls (include/fdg.h: fdg_[mc_]accumulate_device_strat) ----
// sum[h][k] += t_k and sum2[h][k] += t_k t_k over the samples of hypercube h, t_k = w root_k for k < R and t_R = w (c_0 r_0 + ...), the
// training pass's term.  The keys (cube[b]) are non-decreasing along the samples, so nothing is sorted and nothing is kept in LDS:
//  * One wave per 64-sample tile and group of kStratCols columns (blockIdx.y): 2 kStratCols values per lane in registers, t and t t.
//    A lane that adds nothing (past n, hypercube out of range) carries 0.0, selected, and the key of the nearest valid lane below it
//    (above it where there is none), so that it never splits a run; wave_runs' logic on the filled keys and the binned pass's
//    segmented suffix scan leave every run of equal keys summed in its first lane.
//  * A run that touches neither end of the wave holds ALL samples of its hypercube (the keys are monotone): its head adds the sums
//    into sum / sum2, the only writer of those words in the whole call.
//  * The run at lane 0 and the run at lane 63 may go on in the neighbouring tiles: they leave the wave as two edge records
//    (key, values) in slots 2 w and 2 w + 1 of the next level; a wave that is one run leaves it in the first slot and the same key
//    with zeros in the second.  fdg_strat_stitch treats the records of a level as this kernel treats samples, 64 slots per wave:
//    interior runs are written, edge runs go up, and every level is 32 times shorter.  The level that fits one wave leaves its two
//    edge runs as the CHUNK's records; after the last chunk the chunks' records go through the same levels, and the last wave
//    (final) writes every run.  A hypercube of 10^8 samples is thus summed by a tree of depth 6 + 6 levels, never by one lane.
// The shape of every level follows from the chunk sizes alone -- (n_sample, n_root, FDG_ROOT_SCRATCH_MB) -- and every word of sum /
// sum2 is written by exactly one lane of one launch: no atomics, bitwise repeatable.
// Records of a level: keys [slot] (int32, -1: nothing), values [column][slot] with the C1 = R + E columns of the first moment, then
// the C1 of the second (E = 1 but for the grouped calls with several groups: one column per group).  wmask: bit j set = the column of value j is written to sum / sum2 (a root that exists).
constexpr uint32_t kStratCols = 8, kStratVals = 2 * kStratCols;

// E columns behind the roots' (1: the coef combination; the grouped calls: one per weight group); bit e of emask set = column R + e
// has a root that exists behind it.
__device__ __forceinline__ uint32_t strat_wmask(uint32_t k0, uint32_t R, uint32_t E, const uint8_t *__restrict__ live, uint32_t emask) {
  uint32_t m = 0;
  for (uint32_t j = 0; j < kStratVals; ++j) {
    const uint32_t kk = k0 + (j & (kStratCols - 1u));
    const bool on = kk < R ? (!live || live[kk]) : (kk - R < E && ((emask >> (kk - R)) & 1u) != 0);
    m |= on ? 1u << j : 0u;
  }
  return m;
}

// The shared end of both kernels: s[] = this lane's values (0.0 where !ok), key its hypercube; slot = the wave's first output slot.
__device__ __forceinline__ void strat_wave_reduce(int32_t key, bool ok, uint32_t lane, double (&s)[kStratVals], uint32_t k0, uint32_t C1,
                                                  uint32_t wmask, double *__restrict__ sum, double *__restrict__ sum2, bool final,
                                                  int32_t *__restrict__ rkey, double *__restrict__ rval, long rstride, long slot) {
  const bool wkey = blockIdx.y == 0;                      // every column group sees the same keys: the first one records them
  const uint64_t valid = __ballot(ok);
  if (!valid) {
    if (!final && wkey && lane < 2) rkey[slot + lane] = -1;
    return;
  }
  const uint64_t upto = valid & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
  const int src = upto ? 63 - __builtin_clzll(upto) : __builtin_ctzll(valid);
  const int32_t kf = __shfl(key, src);
  const int32_t k_prev = __shfl_up(kf, 1), k_next = __shfl_down(kf, 1);
  const bool head = lane == 0 || k_prev != kf;
  const uint64_t tails = __ballot(lane == 63 || k_next != kf);
  const uint32_t end = (uint32_t)__builtin_ctzll(tails & (~0ull << lane));
  for (uint32_t d = 1; d < 64; d <<= 1) {                 // segmented suffix scan, as in fdg_binned_partials
    const bool take = lane + d <= end;
    if (!__ballot(take)) break;
#pragma unroll
    for (uint32_t j = 0; j < kStratVals; ++j) {
      const double up = __shfl_down(s[j], d);
      if (take) s[j] = s[j] + up;
    }
  }
  if (!head) return;
  const bool at0 = lane == 0, at63 = end == 63;
  if (final || (!at0 && !at63)) {
#pragma unroll
    for (uint32_t j = 0; j < kStratVals; ++j)
      if ((wmask >> j) & 1u) {
        double *o = (j < kStratCols ? sum : sum2) + (size_t)kf * C1 + k0 + (j & (kStratCols - 1u));
        *o = *o + s[j];
      }
    return;
  }
  const long at = slot + (at0 ? 0 : 1);
  if (wkey) rkey[at] = kf;
  if (wkey && at0 && at63) rkey[at + 1] = kf;
#pragma unroll
  for (uint32_t j = 0; j < kStratVals; ++j) {
    const uint32_t kk = k0 + (j & (kStratCols - 1u));
    if (kk >= C1) continue;
    double *o = rval + (size_t)((j < kStratCols ? 0u : C1) + kk) * (size_t)rstride + (size_t)at;
    o[0] = s[j];
    if (at0 && at63) o[1] = 0.0;
  }
}

// Level 0: the samples of a chunk (root k of sample b at root[k * ld + b], b < n).  The scratch columns are read for the last time
// in the chunk: non-temporal loads.
// GRP (fdg_[mc_]accumulate_device_strat_grouped with more than one group): column k < R is weighted by the column of its root's group
// (rgrp[k], the first R words of the groups' table: a root that does not exist carries a neighbour's group and is never written), and
// NG columns follow, R + g = w_g s_g (vegas_group_term); bit g of emask: group g has a root that exists.  The lists kidx / coef are
// then sorted by (group, root), as the grouped training pass takes them.
template <bool GRP = false>
__global__ void __launch_bounds__(256)
fdg_strat_partials(const double *__restrict__ root, long ld, long n, const int32_t *__restrict__ cube, uint32_t H,
                   const double *__restrict__ weight, const uint32_t *__restrict__ kidx, const double *__restrict__ coef, uint32_t n_live,
                   uint32_t R, const uint8_t *__restrict__ live, double *__restrict__ sum, double *__restrict__ sum2,
                   int32_t *__restrict__ rkey, double *__restrict__ rval, long rstride, long slot_base,
                   const uint32_t *__restrict__ rgrp, const uint32_t *__restrict__ gstart, uint32_t NG, long wstride, uint32_t emask) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const long t = (long)blockIdx.x * kBinWaves + wave;
  if (t >= (n + 63) / 64) return;                          // (whole waves leave; the kernel has no barrier)
  const uint32_t E = GRP ? NG : 1u;
  const uint32_t k0 = blockIdx.y * kStratCols, C1 = R + E;
  const long b = t * 64 + lane;
  const size_t bb = (size_t)min(b, n - 1);                 // clamped into the chunk; what it loads is used only where `ok`
  const int32_t h = cube[bb];
  const bool ok = b < n && (uint32_t)h < H;
  double w = 1.0;
  if constexpr (!GRP) w = weight ? weight[bb] : 1.0;
  double s[kStratVals];
#pragma unroll
  for (uint32_t i = 0; i < kStratCols; ++i) {
    const uint32_t kk = k0 + i;
    double tk = 0.0;
    if constexpr (GRP) {
      if (kk < R) tk = weight[(size_t)rgrp[kk] * (size_t)wstride + bb] * __builtin_nontemporal_load(root + (size_t)kk * (size_t)ld + bb);
      else if (kk < C1) tk = vegas_group_term(root, ld, bb, weight, wstride, kidx, coef, gstart, kk - R);
    } else {
      if (kk < R) tk = w * __builtin_nontemporal_load(root + (size_t)kk * (size_t)ld + bb);
      else if (kk == R) tk = vegas_term(root, ld, bb, weight, kidx, coef, n_live);
    }
    s[i] = ok ? tk : 0.0;                                  // selected, never multiplied by 0
    s[kStratCols + i] = ok ? tk * tk : 0.0;
  }
  const uint32_t em = GRP ? emask : (n_live != 0 ? 1u : 0u);
  strat_wave_reduce(h, ok, lane, s, k0, C1, strat_wmask(k0, R, E, live, em), sum, sum2, false, rkey, rval, rstride, slot_base + 2 * t);
}

// Levels 1 ..: the n_slot records of the level below.
// GRP: NG columns behind the roots' in the place of one (emask as in fdg_strat_partials).
template <bool GRP = false>
__global__ void __launch_bounds__(256)
fdg_strat_stitch(const int32_t *__restrict__ ikey, const double *__restrict__ ival, long istride, long n_slot, uint32_t R,
                 const uint8_t *__restrict__ live, uint32_t n_live, double *__restrict__ sum, double *__restrict__ sum2, int final,
                 int32_t *__restrict__ rkey, double *__restrict__ rval, long rstride, long slot_base, uint32_t NG, uint32_t emask) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const long wv = (long)blockIdx.x * kBinWaves + wave;
  if (wv >= (n_slot + 63) / 64) return;
  const uint32_t E = GRP ? NG : 1u, em = GRP ? emask : (n_live != 0 ? 1u : 0u);
  const uint32_t k0 = blockIdx.y * kStratCols, C1 = R + E;
  const long i = wv * 64 + lane;
  const size_t ii = (size_t)min(i, n_slot - 1);
  const int32_t key = ikey[ii];
  const bool ok = i < n_slot && key >= 0;
  double s[kStratVals];
#pragma unroll
  for (uint32_t j = 0; j < kStratVals; ++j) {
    const uint32_t kk = min(k0 + (j & (kStratCols - 1u)), C1 - 1u);   // clamped: a column past the last is never written
    const double v = ival[(size_t)((j < kStratCols ? 0u : C1) + kk) * (size_t)istride + ii];
    s[j] = ok ? v : 0.0;
  }
  strat_wave_reduce(key, ok, lane, s, k0, C1, strat_wmask(k0, R, E, live, em), sum, sum2, final != 0, rkey, rval, rstride,
                    slot_base + 2 * wv);
}

// The training pass of one call, as the entry point was given it (aggregate-initialised there, in this order).
struct VegasRun {
  const double *coef = nullptr;      // host, [R] or null
  uint64_t seed = 0, offset = 0;
  uint32_t D = 0, G = 0;
  double *d_hist = nullptr;
  bool binned = false;               // the calls with a discrete variable: d_bin selects the samples of the training pass too
  double *d_hist_bin = nullptr;      // ... and, when given, the discrete variable is trained: [n_bin]
};

// The projection of one call (fdg_[mc_]accumulate_device_matsubara): the descriptor, and the T the pass reads (the descriptor's, or the
// Monte-Carlo call's own).
struct MatsubaraRun {
  const fdg_matsubara *m = nullptr;
  const double *d_T = nullptr;
  int64_t ts = 0, tc = 0;
};

// The observables of one call (fdg_[mc_]accumulate_device_observables): the descriptor as the entry point was given it.
struct ObsRun {
  const fdg_observables *ob = nullptr;
};

// The stratification of one call (fdg_[mc_]accumulate_device_strat), as the entry point was given it.
struct StratRun {
  const uint32_t *strat = nullptr;   // host, [n_dim]
  const int32_t *d_cube = nullptr;
  double *d_sum = nullptr, *d_sum2 = nullptr;
};

// One accumulate call, as the entry point was given it (aggregate-initialised there, in this order): what the checks, the shared body
// and run_binned read.
struct BinnedCall {
  const int32_t *d_bin = nullptr;    // null: every sample in bin 0 (n_bin == 1)
  int32_t bin_base = 0;
  uint32_t n_bin = 1;
  const double *d_weight = nullptr;
  double *d_acc = nullptr, *d_acc2 = nullptr;     // d_acc2 != null: the second moment too
  int64_t B = 0;
  void *stream = nullptr;
  const VegasRun *vg = nullptr;      // the VEGAS calls: the training pass runs too
  const MatsubaraRun *mz = nullptr;  // the projection calls: the projection pass runs too; d_acc and d_acc2 may then both be null
  const fdg_weight_groups *wg = nullptr;   // the grouped calls: d_weight holds one column per group
  const ObsRun *ob = nullptr;        // the observables calls: the observables pass runs too; d_acc and d_acc2 may then both be null
  const StratRun *sr = nullptr;      // the stratified calls: the training pass reads the hypercubes, the per-hypercube pass runs too
  // the frequency-observables calls: their pass runs too, with mz's frequencies, time labels, beta and T; mz's four arrays may then
  // all be null (no per-root projection) and ob may be null
  const fdg_freq_observables *fo = nullptr;
};

constexpr size_t page_up(size_t bytes) { return (bytes + 4095) & ~(size_t)4095; }

// How a chunk of Bc samples is cut into segments for a histogram of hist_bytes that n_grp workgroups per segment share the columns of:
// at least 16 tiles (four rounds) per workgroup, the partial slab [segment][histogram] within kBinSlabBytes, at most 2048 workgroups.
// These numbers fix the order of every sum.  slab_alloc: the slab's reservation; it grows with n_sample and the histogram only, so a
// later call that is not larger allocates nothing.
struct SegCut {
  uint32_t n_seg;
  size_t slab_alloc;
};
SegCut seg_cut(long Bc, size_t hist_bytes, long n_grp) {
  const long by_size = std::max<long>(1, Bc / 64 / 16);
  const long by_slab = std::max<long>(1, (long)(kBinSlabBytes / hist_bytes));
  const long by_blocks = std::max<long>(1, 2048 / n_grp);
  return {(uint32_t)std::min(std::min(by_size, by_slab), by_blocks), std::max(hist_bytes, std::min(kBinSlabBytes, (size_t)by_size * hist_bytes))};
}

// How one call is cut: chunks of Bc samples through the root scratch, RS roots per slice, n_seg segments per chunk.  mode: what the
// pass keeps (BinMode); n_slice counts the root slices of one moment.
struct BinnedPlan {
  long Bc = 0;
  uint32_t rs = 1, n_slice = 1, n_seg = 1;
  int mode = kFirst;
  size_t lds = 0, slab_alloc = 0;
};

// moments: the plan of the second-moment call.  Bc and n_seg are the binned call's (its own slice count and slab size), so the first
// moment is summed in the binned call's order; only the slices (two histograms per workgroup, or one moment per slice) differ.
BinnedPlan binned_plan(const fdg_graph *g, int64_t B, uint32_t R, uint32_t n_bin, bool moments) {
  BinnedPlan p;
  p.Bc = std::max<long>(64, (long)((g->cfg.root_scratch_mb << 20) / (8ull * R)) & ~63l);
  p.Bc = std::min<long>(p.Bc, (long)((B + 63) & ~(int64_t)63));
  // the roots per slice by the LDS budget, for histograms of `bytes` per (bin, root)
  auto slice = [&](size_t bytes) {
    uint32_t rs = 16;
    while (rs > 1 && (size_t)n_bin * rs * bytes > kBinLdsBudget) rs >>= 1;
    while (rs > 1 && rs / 2 >= R) rs >>= 1;
    p.rs = rs;
    p.n_slice = (R + rs - 1) / rs;
    p.lds = (size_t)n_bin * rs * bytes;
  };
  slice(8);
  const SegCut cut = seg_cut(p.Bc, (size_t)n_bin * R * 8u, p.n_slice);
  p.n_seg = cut.n_seg;
  p.slab_alloc = cut.slab_alloc;
  if (moments) {
    p.slab_alloc *= 2;                                                 // [segment][moment][bin][root]
    if ((size_t)n_bin * 16u <= (size_t)FDG_BIN_MAX * 8u) {             // both histograms of one root fit: kBoth, the same budget rule
      p.mode = kBoth;
      slice(16);
    } else {                                                           // n_bin > 8192: one root of one moment per workgroup
      p.mode = kSplit;
      p.rs = 1;
      p.n_slice = R;
      p.lds = (size_t)n_bin * 8u;
    }
  }
  return p;
}

// How the training pass is cut.  Variables per slice by the binned plan's LDS budget (whole histograms of G cells), spread evenly over
// the slices; segments by the binned plan's cut with the histogram [variable][cell] in the place of [bin][root].  A function of
// (n_sample, n_dim, n_grid, n_root, FDG_ROOT_SCRATCH_MB) only.
// bin_*: the discrete variable's slice (fdg_vegas_bin_partials), segments by the same cut with the histogram [bin]; a function
// of (n_sample, n_bin, n_root, FDG_ROOT_SCRATCH_MB) that leaves the continuous variables' cut as it is.
struct VegasPlan {
  uint32_t ds = 1, n_slice = 1, n_seg = 1, bin_seg = 1;
  size_t lds = 0, slab_alloc = 0, list_bytes = 0, bin_slab_alloc = 0;
};

// n_group: the exchange buffer holds one value per group, on top of the histograms' budget (1: today's plan).
VegasPlan vegas_plan(const BinnedPlan &p, const VegasRun &v, uint32_t R, uint32_t n_bin, uint32_t n_group) {
  VegasPlan q;
  const uint32_t fit = (uint32_t)std::max<size_t>(1, kBinLdsBudget / ((size_t)v.G * 8u));
  q.n_slice = (v.D + fit - 1) / fit;
  q.ds = (v.D + q.n_slice - 1) / q.n_slice;
  q.n_slice = (v.D + q.ds - 1) / q.ds;
  q.lds = ((size_t)q.ds * v.G + 2u * kBinWaves * 64u * n_group) * 8u;
  const SegCut cut = seg_cut(p.Bc, (size_t)v.D * v.G * 8u, q.n_slice);
  q.n_seg = cut.n_seg;
  q.slab_alloc = page_up(cut.slab_alloc);
  q.list_bytes = page_up((size_t)R * 12u);                       // coef[R] doubles, then kidx[R]
  if (v.d_hist_bin) {
    const SegCut bin_cut = seg_cut(p.Bc, (size_t)n_bin * 8u, 1);
    q.bin_seg = bin_cut.n_seg;
    q.bin_slab_alloc = page_up(bin_cut.slab_alloc);
  }
  return q;
}

// How the projection pass is cut.  Roots and frequencies per slice by the binned plan's LDS budget for four histograms (32 bytes per
// (bin, frequency, root)): roots first, as the moments pass slices them, then as many frequencies as still fit, spread evenly over the
// slices; when four histograms of one (root, frequency) do not fit in what one root of FDG_BIN_MAX bins takes, one histogram per
// workgroup (hsplit).  nw: waves per workgroup, one per item up to four.  Segments by the binned plan's cut with the histogram
// [4][bin][frequency][root].  A function of (n_sample, n_bin, n_freq, n_root, FDG_ROOT_SCRATCH_MB) only.
struct MatsubaraPlan {
  uint32_t rs = 1, fs = 1, n_fslice = 1, n_grp = 1, nw = 1, kw = 1, n_seg = 1;
  bool hsplit = false;
  size_t lds = 0, slab_alloc = 0, tab_bytes = 0;
};

MatsubaraPlan matsubara_plan(const BinnedPlan &p, uint32_t R, uint32_t n_bin, uint32_t n_freq) {
  MatsubaraPlan q;
  q.hsplit = (size_t)n_bin * 32u > (size_t)FDG_BIN_MAX * 8u;
  if (!q.hsplit) {
    uint32_t rs = 16;
    while (rs > 1 && (size_t)n_bin * rs * 32u > kBinLdsBudget) rs >>= 1;
    while (rs > 1 && rs / 2 >= R) rs >>= 1;
    q.rs = rs;
    const uint32_t fit = (uint32_t)std::max<size_t>(1, kBinLdsBudget / ((size_t)n_bin * rs * 32u));
    q.n_fslice = (n_freq + fit - 1) / fit;
    q.fs = (n_freq + q.n_fslice - 1) / q.n_fslice;
  }
  q.n_fslice = (n_freq + q.fs - 1) / q.fs;
  q.n_grp = ((R + q.rs - 1) / q.rs) * q.n_fslice * (q.hsplit ? 4u : 1u);
  while (q.nw < kBinWaves && q.nw * 2 <= q.rs * q.fs) q.nw <<= 1;
  q.kw = std::max(1u, q.rs / q.nw);
  q.lds = (size_t)(q.hsplit ? 1 : 4) * n_bin * q.fs * q.rs * 8u;
  const SegCut cut = seg_cut(p.Bc, (size_t)n_bin * n_freq * R * 32u, q.n_grp);
  q.n_seg = cut.n_seg;
  q.slab_alloc = page_up(cut.slab_alloc);
  q.tab_bytes = page_up(FDG_MATSUBARA_FREQ_MAX * 8u + (size_t)R * 8u);      // mult[], then tin[R], tout[R]
  return q;
}

// How the two observables passes are cut.  A histogram row is a (bin, frequency) pair of V value columns (the observables: one
// frequency, V = M + M (M + 1) / 2; the frequency observables: V = 2 M + M (2 M + 1)).  Frequencies are sliced first (a frequency
// slice forms only its own phases): as many whole frequencies of V columns as the binned plan's LDS budget holds, spread evenly over
// the slices; only when not even one fits are the columns sliced too: as many as the budget holds (whole columns of n_bin bins; one
// column of more than 8192 bins takes what one root of FDG_BIN_MAX bins takes), spread evenly over the slices.  Segments: the binned
// call's own count whenever the slab [segment][bin][frequency][V] fits in 2 kBinSlabBytes (the moments call's bound), so that a unit
// row sums in the moments call's order; else the largest count that fits.  A function of (n_sample, n_bin, n_freq, n_obs, n_root,
// FDG_ROOT_SCRATCH_MB) only.
struct ObsPlan {
  uint32_t V = 1, fs = 1, n_fslice = 1, cs = 1, n_cslice = 1, n_seg = 1;
  size_t hist_bytes = 0, slab_alloc = 0;
};

ObsPlan obs_plan(const BinnedPlan &p, uint32_t n_bin, uint32_t n_freq, uint32_t V) {
  ObsPlan q;
  q.V = V;
  const uint32_t fit = (uint32_t)std::max<size_t>(1, kBinLdsBudget / ((size_t)n_bin * 8u));     // words per bin
  if (fit >= q.V) {
    const uint32_t ffit = fit / q.V;
    q.n_fslice = (n_freq + ffit - 1) / ffit;
    q.fs = (n_freq + q.n_fslice - 1) / q.n_fslice;
    q.cs = q.V;
  } else {
    q.n_cslice = (q.V + fit - 1) / fit;
    q.cs = (q.V + q.n_cslice - 1) / q.n_cslice;
  }
  q.n_fslice = (n_freq + q.fs - 1) / q.fs;
  q.n_cslice = (q.V + q.cs - 1) / q.cs;
  q.hist_bytes = (size_t)n_bin * q.fs * q.cs * 8u;
  const size_t seg_bytes = (size_t)n_bin * n_freq * q.V * 8u;
  q.n_seg = (uint32_t)std::max<size_t>(1, std::min<size_t>(p.n_seg, 2u * kBinSlabBytes / seg_bytes));
  q.slab_alloc = page_up((size_t)q.n_seg * seg_bytes);
  return q;
}

// The tables of fdg_obs_partials or fdg_fobs_partials for one call (the layout is stated at fdg_obs_partials), built from the M rows
// of host coefficients: need = the most stash rows a column slice uses, live = bit p set when row p has a term.  mz == null: the
// observables, the rows are the M rows.  Else the frequency observables: 2 M rows, the components a_m (p = m) and b_m (p = M + m),
// both reading row p % M of coef; dtab starts with the descriptor's multipliers, a record carries its root's time labels, a term of
// b_m the bit kFobsIm.
struct ObsTables {
  std::vector<uint32_t> u;
  std::vector<double> d;
  uint32_t need = 1, live = 0;
};

ObsTables obs_tables(const fdg_graph *g, const ObsPlan &q, const double *coef, uint32_t M, const fdg_matsubara *mz,
                     const fdg_weight_groups *wg) {
  const uint32_t R = g->prog.R, P = mz ? 2u * M : M, W = mz ? kFobsRec : 4u;
  ObsTables t;
  auto coef_of = [&](uint32_t p, uint32_t k) { return coef[(size_t)(p % M) * R + k]; };
  auto term = [&](uint32_t p, uint32_t k) { return g->prog.root_slot[k] != FDG_NO_ROOT && coef_of(p, k) != 0.0; };
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t k = 0; k < R; ++k)
      if (term(p, k)) { t.live |= 1u << p; break; }
  if (mz) {
    t.d.assign(FDG_MATSUBARA_FREQ_MAX, 0.0);
    for (uint32_t f = 0; f < mz->n_freq; ++f) t.d[f] = matsubara_multiplier(mz->freq[f], mz->fermionic);
  }
  std::vector<uint32_t> pa, pc;                            // the factors of every value column
  for (uint32_t p = 0; p < P; ++p) { pa.push_back(p); pc.push_back(kObsNone); }
  for (uint32_t a = 0; a < P; ++a)
    for (uint32_t c = a; c < P; ++c) { pa.push_back(a); pc.push_back(c); }
  t.u.assign((size_t)q.n_cslice * 4u, 0u);
  for (uint32_t s = 0; s < q.n_cslice; ++s) {
    const uint32_t c0 = s * q.cs, cn = std::min(q.cs, q.V - c0);
    std::vector<uint32_t> slot(P, kObsNone);               // the stash row of every row the slice needs, ascending
    std::vector<uint32_t> colA(q.cs, kObsNone), colB(q.cs, kObsNone);
    uint32_t used = 0;
    for (uint32_t cl = 0; cl < cn; ++cl) {
      const uint32_t a = pa[c0 + cl], c = pc[c0 + cl];
      if (!((t.live >> a) & 1u) || (c != kObsNone && !((t.live >> c) & 1u))) continue;
      used |= 1u << a;
      if (c != kObsNone) used |= 1u << c;
    }
    uint32_t n_need = 0;
    for (uint32_t p = 0; p < P; ++p)
      if ((used >> p) & 1u) slot[p] = n_need++;
    for (uint32_t cl = 0; cl < cn; ++cl) {
      const uint32_t a = pa[c0 + cl], c = pc[c0 + cl];
      if (slot[a] == kObsNone || (c != kObsNone && slot[c] == kObsNone)) continue;
      colA[cl] = slot[a];
      colB[cl] = c == kObsNone ? kObsNone : slot[c];
    }
    std::vector<uint32_t> recs, terms;
    std::vector<bool> started(P, false);
    const size_t d0 = t.d.size();
    int32_t last_in = -1, last_out = -1;
    for (uint32_t k = 0; k < R; ++k) {
      const uint32_t tb = (uint32_t)terms.size();
      for (uint32_t p = 0; p < P; ++p)
        if (slot[p] != kObsNone && term(p, k)) {
          terms.push_back(slot[p] | (started[p] ? 0u : kObsFirst) | (p >= M ? kFobsIm : 0u));
          started[p] = true;
          t.d.push_back(coef_of(p, k));
        }
      if (terms.size() == tb) continue;
      uint32_t rk[kFobsRec] = {k, wg && wg->n_group > 1 ? wg->root_group[k] : 0u, tb, (uint32_t)terms.size(), 0u, 0u};
      if (mz) {
        const int32_t tin = mz->root_tau_in[k] - 1, tout = mz->root_tau_out[k] - 1;
        if (!recs.empty() && tin == last_in && tout == last_out) rk[1] |= kFobsSame;
        rk[4] = (uint32_t)tin;
        rk[5] = (uint32_t)tout;
        last_in = tin;
        last_out = tout;
      }
      recs.insert(recs.end(), rk, rk + W);
    }
    uint32_t *hdr = t.u.data() + (size_t)s * 4u;
    hdr[0] = n_need;
    hdr[1] = (uint32_t)(recs.size() / W);
    hdr[2] = (uint32_t)t.u.size();
    hdr[3] = (uint32_t)d0;
    t.need = std::max(t.need, n_need);
    t.u.insert(t.u.end(), colA.begin(), colA.end());
    t.u.insert(t.u.end(), colB.begin(), colB.end());
    t.u.insert(t.u.end(), recs.begin(), recs.end());
    t.u.insert(t.u.end(), terms.begin(), terms.end());
  }
  return t;
}

// What run_binned keeps of one of the two passes: P rows (the 2 M components of the frequency observables; 0: the call has no such
// pass) over n_freq frequencies (one for the observables), the plan, the tables, and its region of the workspace: the partial slab,
// then dtab, then utab, each from a page boundary.
struct ObsPass {
  uint32_t P = 0, n_freq = 1;
  bool freq = false;                                       // the frequency observables' pass
  ObsPlan q;
  ObsTables t;
  size_t bytes = 0;
  double *partial = nullptr, *d_dtab = nullptr;
  uint32_t *d_utab = nullptr;

  // mz: the descriptor of the frequency observables' pass, null for the observables'
  void set_up(const fdg_graph *g, const BinnedPlan &p, uint32_t n_bin, const double *coef, uint32_t M, const fdg_matsubara *mz,
              const fdg_weight_groups *wg) {
    freq = mz != nullptr;
    P = mz ? 2u * M : M;
    n_freq = mz ? mz->n_freq : 1u;
    q = obs_plan(p, n_bin, n_freq, P + P * (P + 1u) / 2u);
    t = obs_tables(g, q, coef, M, mz, wg);
    bytes = q.slab_alloc + page_up(t.d.size() * 8u) + page_up(t.u.size() * 4u);
  }
  // the region starts at `at`: one upload per table (the observables' dtab is empty when no row has a term)
  int place(char *at, hipStream_t st) {
    partial = (double *)at;
    d_dtab = (double *)(at + q.slab_alloc);
    d_utab = (uint32_t *)((char *)d_dtab + page_up(t.d.size() * 8u));
    if (!t.d.empty()) HIP_TRY(hipMemcpyAsync(d_dtab, t.d.data(), t.d.size() * 8u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_utab, t.u.data(), t.u.size() * 4u, hipMemcpyHostToDevice, st));
    return FDG_OK;
  }
  // d_o and d_c += the segments' partials, C columns per workgroup: C fixes the order of the segments' sum (0: by the moments
  // reduce's rule from the pass's own columns)
  int reduce(uint32_t n_bin, uint32_t C, double *d_o, double *d_c, hipStream_t st) const {
    const long ncol = (long)n_bin * n_freq * q.V;
    if (!C)
      for (C = 1; C < 64 && (long)C < ncol;) C <<= 1;
    hipLaunchKernelGGL(fdg_obs_reduce, dim3((unsigned)((ncol + C - 1) / C)), dim3(256), 0, st, partial, q.n_seg, ncol, P, q.V, C, t.live, d_o,
                       d_c);
    HIP_TRY(hipGetLastError());
    return FDG_OK;
  }
};

// How the per-hypercube pass is cut: the record buffers of the levels (slots: two per wave of the level below).  A chunk's levels
// alternate between a and b, the chunks' own records (two per chunk) lie in c and go through a and b again after the last chunk.
// A function of (n_sample, n_root, the E columns behind the roots', FDG_ROOT_SCRATCH_MB) only.
struct StratPlan {
  uint32_t H = 1, n_grp = 1, V2 = 2;
  long n_chunk = 1, cap_a = 2, cap_b = 2, cap_c = 2;
  size_t bytes = 0;
  static size_t buf_bytes(long cap, uint32_t V2) { return page_up((size_t)cap * 4u) + page_up((size_t)cap * V2 * 8u); }
};

StratPlan strat_plan(const BinnedPlan &p, int64_t B, uint32_t R, uint32_t H, uint32_t E) {
  StratPlan q;
  q.H = H;
  q.V2 = 2u * (R + E);
  q.n_grp = (R + E + kStratCols - 1u) / kStratCols;
  q.n_chunk = ((long)B + p.Bc - 1) / p.Bc;
  q.cap_c = 2 * q.n_chunk;
  q.cap_a = std::max(2 * ((p.Bc + 63) / 64), 2 * ((q.cap_c + 63) / 64));
  q.cap_b = 2 * ((q.cap_a + 63) / 64);
  q.bytes = StratPlan::buf_bytes(q.cap_a, q.V2) + StratPlan::buf_bytes(q.cap_b, q.V2) + StratPlan::buf_bytes(q.cap_c, q.V2);
  return q;
}

// The strata of a call as the kernels take them (strat checked: every entry >= 1, the product within FDG_STRAT_CUBE_MAX).
VegasStrat vegas_strat(const uint32_t *strat, uint32_t n_dim) {
  VegasStrat sv;
  uint32_t H = 1;
  for (uint32_t d = 0; d < FDG_VEGAS_DIM_MAX; ++d) {
    sv.n[d] = d < n_dim ? strat[d] : 1u;
    sv.div[d] = H;
    H *= sv.n[d];
  }
  sv.H = H;
  return sv;
}

// The stratified calls' own checks, after the map's: H = prod strat[d] in *H.
int check_strat(const uint32_t *strat, uint32_t n_dim, uint32_t *H) {
  uint64_t h = 1;
  for (uint32_t d = 0; d < n_dim; ++d) {
    if (strat[d] == 0) { set_error("strat[d] == 0"); return FDG_E_INVALID; }
    h *= strat[d];
    if (h > FDG_STRAT_CUBE_MAX) { set_error("prod strat[d] > FDG_STRAT_CUBE_MAX"); return FDG_E_UNSUPPORTED; }
  }
  *H = (uint32_t)h;
  return FDG_OK;
}

using MatsubaraKernel = void (*)(const double *, long, long, const int32_t *, int32_t, uint32_t, const double *, const double *, long, long,
                                 const double *, double, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, long, double *, int,
                                 const uint32_t *, long);

template <bool GRP>
MatsubaraKernel matsubara_kernel_of(const MatsubaraPlan &q) {
  if (q.hsplit) return fdg_matsubara_partials<1, true, GRP>;
  return q.kw == 4   ? fdg_matsubara_partials<4, false, GRP>
         : q.kw == 2 ? fdg_matsubara_partials<2, false, GRP>
                     : fdg_matsubara_partials<1, false, GRP>;
}

MatsubaraKernel matsubara_kernel(const MatsubaraPlan &q, bool grp) { return grp ? matsubara_kernel_of<true>(q) : matsubara_kernel_of<false>(q); }

// The instance of the binned pass a plan asks for.
using PartialsKernel = void (*)(const double *, long, long, const int32_t *, int32_t, uint32_t, const double *, uint32_t, uint32_t, long,
                                double *, int, const uint32_t *, long);

template <int MODE, bool GRP = false>
PartialsKernel partials_kernel_rs(uint32_t rs) {
  switch (rs) {
    case 1: return fdg_binned_partials<1, MODE, GRP>;
    case 2: return fdg_binned_partials<2, MODE, GRP>;
    case 4: return fdg_binned_partials<4, MODE, GRP>;
    case 8: return fdg_binned_partials<8, MODE, GRP>;
    default: return fdg_binned_partials<16, MODE, GRP>;
  }
}

// grp: the instance that reads one weight column per group (the grouped calls keep both moments: kBoth or kSplit)
PartialsKernel partials_kernel(const BinnedPlan &p, bool grp) {
  if (p.mode == kBoth) return grp ? partials_kernel_rs<kBoth, true>(p.rs) : partials_kernel_rs<kBoth>(p.rs);
  if (p.mode == kSplit) return grp ? fdg_binned_partials<1, kSplit, true> : fdg_binned_partials<1, kSplit>;
  return partials_kernel_rs<kFirst>(p.rs);
}

// Lets every pass ask for more than the default 64 KiB of dynamic LDS: a histogram slice of one root of up to FDG_BIN_MAX bins
// (128 KiB of the CU's 160), and the training pass's kBinLdsBudget plus its exchange buffers.
void raise_lds_limits() {
  static std::once_flag once;
  std::call_once(once, [] {
    const int hist = (int)(FDG_BIN_MAX * 8), train = (int)(kBinLdsBudget + 2u * kBinWaves * 64u * 8u);
    const int train_grp = (int)(kBinLdsBudget + 2u * kBinWaves * 64u * 8u * FDG_WEIGHT_GROUP_MAX);
    // the observables pass: a histogram slice and the stash, 2 KiB per row (every row beside kBinLdsBudget, two beside one column of FDG_BIN_MAX bins)
    const int obs = (int)std::max<size_t>(kBinLdsBudget + FDG_OBS_MAX * 2048u, FDG_BIN_MAX * 8u + 2u * 2048u);
    static_assert(2 * FDG_FREQ_OBS_MAX <= FDG_OBS_MAX, "the frequency observables' stash is sized by the observables'");
    std::vector<std::pair<const void *, int>> limits = {{(const void *)fdg_obs_partials, obs},
                                                        {(const void *)fdg_fobs_partials, obs},   // 2 M components in the place of the rows
                                                        {(const void *)fdg_binned_partials<1, kSplit>, hist},
                                                        {(const void *)fdg_binned_partials<1, kSplit, true>, hist},
                                                        {(const void *)fdg_vegas_bin_partials<false>, hist},
                                                        {(const void *)fdg_vegas_bin_partials<true>, hist},
                                                        {(const void *)fdg_vegas_partials<0>, train},
                                                        {(const void *)fdg_vegas_partials<1>, train},
                                                        {(const void *)fdg_vegas_partials<0, true>, train_grp},
                                                        {(const void *)fdg_vegas_partials<1, true>, train_grp},
                                                        {(const void *)fdg_vegas_partials<0, false, true>, train},
                                                        {(const void *)fdg_vegas_partials<0, true, true>, train_grp}};
    MatsubaraPlan mq;
    for (int i = 0; i < 4; ++i) {                          // hsplit, then kw = 1, 2, 4
      mq.hsplit = i == 0;
      mq.kw = i ? 1u << (i - 1) : 1u;
      limits.push_back({(const void *)matsubara_kernel(mq, false), hist});
      limits.push_back({(const void *)matsubara_kernel(mq, true), hist});
    }
    for (uint32_t rs = 1; rs <= 16; rs <<= 1) {
      limits.push_back({(const void *)partials_kernel_rs<kFirst>(rs), hist});
      limits.push_back({(const void *)partials_kernel_rs<kBoth>(rs), hist});
      limits.push_back({(const void *)partials_kernel_rs<kBoth, true>(rs), hist});
    }
    for (const auto &l : limits) (void)hipFuncSetAttribute(l.first, hipFuncAttributeMaxDynamicSharedMemorySize, l.second);
    (void)hipGetLastError();
  });
}

// out[c] += the n_seg segments' partials [segment][moment][ncol], in segment order (fdg_binned_reduce; C columns per workgroup).
int reduce_partials(const double *partial, uint32_t n_seg, long ncol, uint32_t R, uint32_t C, double *d_acc, double *d_acc2,
                    const uint8_t *live, hipStream_t st) {
  const uint32_t n_mom = d_acc2 ? 2 : 1;
  hipLaunchKernelGGL(fdg_binned_reduce, dim3((unsigned)((ncol + C - 1) / C), n_mom), dim3(256), 0, st, partial, n_seg, ncol * n_mom, ncol, R,
                     C, d_acc, d_acc2, live);
  HIP_TRY(hipGetLastError());
  return FDG_OK;
}

// The bin count of a call against its bin vector and FDG_BIN_MAX: three refusals that every call makes, in this order.
int check_n_bin(const BinnedCall &c) {
  if (c.n_bin == 0) { set_error("n_bin == 0"); return FDG_E_INVALID; }
  if (!c.d_bin && c.n_bin != 1) { set_error("d_bin == NULL (one bin) needs n_bin == 1"); return FDG_E_INVALID; }
  if (c.n_bin > FDG_BIN_MAX) { set_error("n_bin > FDG_BIN_MAX"); return FDG_E_UNSUPPORTED; }
  return FDG_OK;
}

// The checks every accumulate entry point makes before any device work.  The binned calls need d_bin; the moments calls need d_acc2
// and take d_bin == NULL (every sample in bin 0, which needs n_bin == 1).
int check_call(const fdg_graph *g, const BinnedCall &c, bool moments) {
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  if (c.B < 0) { set_error("n_sample < 0"); return FDG_E_INVALID; }
  const bool no_acc = c.ob && moments && !c.d_acc && !c.d_acc2;    // the observables calls: no per-root moments asked for
  if (!no_acc && (!c.d_acc || (moments ? !c.d_acc2 : !c.d_bin))) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (!no_acc && c.d_acc == c.d_acc2) { set_error("d_acc and d_acc2 are the same buffer"); return FDG_E_INVALID; }
  return check_n_bin(c);
}

// ... and the VEGAS calls': the map's limits (every call), then the output arrays of the accumulate calls.
int check_vegas_map(uint32_t n_dim, uint32_t n_grid) {
  if (n_dim == 0 || n_grid == 0) { set_error("n_dim == 0 or n_grid == 0"); return FDG_E_INVALID; }
  if (n_dim > FDG_VEGAS_DIM_MAX) { set_error("n_dim > FDG_VEGAS_DIM_MAX"); return FDG_E_UNSUPPORTED; }
  if (n_grid > FDG_VEGAS_GRID_MAX) { set_error("n_grid > FDG_VEGAS_GRID_MAX"); return FDG_E_UNSUPPORTED; }
  return FDG_OK;
}

// The moments calls' cases (with a bin vector where there is a discrete variable), distinct output arrays, the map's limits.
int check_vegas(const fdg_graph *g, const BinnedCall &c) {
  const VegasRun &v = *c.vg;
  if (v.binned && g && !c.d_bin) { set_error("d_bin == NULL: use the call without a discrete variable"); return FDG_E_INVALID; }
  const int rc = check_call(g, c, true);
  if (rc) return rc;
  if (!v.d_hist) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (v.d_hist == c.d_acc || v.d_hist == c.d_acc2) { set_error("d_hist is the same buffer as d_acc or d_acc2"); return FDG_E_INVALID; }
  if (v.d_hist_bin && (v.d_hist_bin == c.d_acc || v.d_hist_bin == c.d_acc2 || v.d_hist_bin == v.d_hist)) {
    set_error("d_hist_bin is the same buffer as d_acc, d_acc2 or d_hist"); return FDG_E_INVALID;
  }
  return check_vegas_map(v.D, v.G);
}

// ... and the stratified calls': the VEGAS calls' cases, then the strata and the per-hypercube arrays.
int check_strat_arrays(const fdg_graph *g, const BinnedCall &c, uint32_t n_extra) {
  const StratRun &s = *c.sr;
  const double *out[5] = {s.d_sum, s.d_sum2, c.d_acc, c.d_acc2, c.vg->d_hist};
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 5; ++b)
      if (out[a] == out[b]) { set_error("d_cube_sum or d_cube_sum2 is the same buffer as another output"); return FDG_E_INVALID; }
  uint32_t H;
  const int rc = check_strat(s.strat, c.vg->D, &H);
  if (rc) return rc;
  if ((uint64_t)H * ((uint64_t)g->prog.R + n_extra) > (1ull << 24)) {
    set_error(n_extra == 1 && !c.wg ? "H * (n_root + 1) > 1 << 24" : "H * (n_root + n_group) > 1 << 24"); return FDG_E_UNSUPPORTED;
  }
  return FDG_OK;
}

int check_strat_call(const fdg_graph *g, const BinnedCall &c) {
  const StratRun &s = *c.sr;
  if (!s.strat || !s.d_cube || !s.d_sum || !s.d_sum2) { set_error("null strat, d_cube, d_cube_sum or d_cube_sum2"); return FDG_E_INVALID; }
  const int rc = check_vegas(g, c);
  return rc ? rc : check_strat_arrays(g, c, 1u);
}

// ... and the projection calls': the descriptor, then what the call asks for besides (moments: d_acc and d_acc2 together; training:
// the VEGAS block, c.vg non-null).  mc_T: the Monte-Carlo form's own T, which a NULL d_T of the descriptor falls back on.
int check_matsubara(const fdg_graph *g, const BinnedCall &c, const fdg_matsubara *m, const double *mc_T) {
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  if (!m) { set_error("null descriptor"); return FDG_E_INVALID; }
  if (c.B < 0) { set_error("n_sample < 0"); return FDG_E_INVALID; }
  const bool no_sums = !m->d_acc_re && !m->d_acc_im && !m->d_acc2_re && !m->d_acc2_im;
  if (c.fo && !no_sums && (!m->d_acc_re || !m->d_acc_im || !m->d_acc2_re || !m->d_acc2_im)) {
    set_error("some but not all of the descriptor's four arrays are NULL"); return FDG_E_INVALID;
  }
  if (!c.fo && (!m->d_acc_re || !m->d_acc_im || !m->d_acc2_re || !m->d_acc2_im)) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (!m->freq || !m->root_tau_in || !m->root_tau_out) { set_error("null host array in the descriptor"); return FDG_E_INVALID; }
  if (!m->d_T && !mc_T) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (!c.d_acc != !c.d_acc2) { set_error("d_acc and d_acc2 go together"); return FDG_E_INVALID; }
  const VegasRun *v = c.vg;
  if (v && !v->d_hist) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (!c.d_bin && v && v->d_hist_bin) { set_error("d_hist_bin needs d_bin"); return FDG_E_INVALID; }
  const double *out[8] = {m->d_acc_re, m->d_acc_im, m->d_acc2_re, m->d_acc2_im, c.d_acc, c.d_acc2, v ? v->d_hist : nullptr,
                          v ? v->d_hist_bin : nullptr};
  for (int a = 0; a < 8; ++a)
    for (int b = 0; b < a; ++b)
      if (out[a] && out[a] == out[b]) { set_error("two output arrays are the same buffer"); return FDG_E_INVALID; }
  const int rc = check_n_bin(c);
  if (rc) return rc;
  if (m->n_freq == 0) { set_error("n_freq == 0"); return FDG_E_INVALID; }
  if (m->n_freq > FDG_MATSUBARA_FREQ_MAX) { set_error("n_freq > FDG_MATSUBARA_FREQ_MAX"); return FDG_E_UNSUPPORTED; }
  if ((uint64_t)c.n_bin * m->n_freq > FDG_BIN_MAX) { set_error("n_bin * n_freq > FDG_BIN_MAX"); return FDG_E_UNSUPPORTED; }
  if (!(m->beta > 0.0)) { set_error("beta <= 0"); return FDG_E_INVALID; }
  for (uint32_t k = 0; k < g->prog.R; ++k) {
    if (g->prog.root_slot[k] == FDG_NO_ROOT) continue;
    const int32_t ti = m->root_tau_in[k], to = m->root_tau_out[k];
    if (ti < 1 || to < 1 || (uint32_t)ti > m->n_tau || (uint32_t)to > m->n_tau) { set_error("time label of a root outside [1, n_tau]"); return FDG_E_INVALID; }
  }
  return v ? check_vegas_map(v->D, v->G) : FDG_OK;
}

// What a call's blocks amount to once its weights are checked: the projection calls' cases with a descriptor, else the VEGAS calls'
// with a training block, else the moments calls'.
int check_blocks(const fdg_graph *g, const BinnedCall &c, const fdg_matsubara *m, const double *mc_T) {
  if (m) return check_matsubara(g, c, m, mc_T);
  if (!c.vg) return check_call(g, c, true);
  if (!c.d_bin && c.vg->d_hist_bin) { set_error("d_hist_bin needs d_bin"); return FDG_E_INVALID; }
  return check_vegas(g, c);
}

// ... and the grouped calls': the weight groups first, then the cases of the call the arguments amount to (the projection calls'
// with a descriptor, else the VEGAS calls' with a training block, else the moments calls').
int check_grouped(const fdg_graph *g, const BinnedCall &c, const fdg_matsubara *m, const double *mc_T, bool wg_optional = false) {
  const fdg_weight_groups *w = c.wg;
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  if (!w && wg_optional) return check_blocks(g, c, m, mc_T);
  if (!w || !w->root_group || !w->var_mask) { set_error("null weight groups, root_group or var_mask"); return FDG_E_INVALID; }
  if (!c.d_weight) { set_error("the grouped calls need d_weight"); return FDG_E_INVALID; }
  if (w->n_group == 0) { set_error("n_group == 0"); return FDG_E_INVALID; }
  if (w->n_group > FDG_WEIGHT_GROUP_MAX) { set_error("n_group > FDG_WEIGHT_GROUP_MAX"); return FDG_E_UNSUPPORTED; }
  for (uint32_t k = 0; k < g->prog.R; ++k)
    if (g->prog.root_slot[k] != FDG_NO_ROOT && w->root_group[k] >= w->n_group) { set_error("root_group names a group >= n_group"); return FDG_E_INVALID; }
  if (c.vg && c.vg->D < 64)
    for (uint32_t gi = 0; gi < w->n_group; ++gi)
      if (w->var_mask[gi] >> c.vg->D) { set_error("var_mask names a variable >= n_dim"); return FDG_E_INVALID; }
  if (w->n_group > 1 && w->weight_group_stride < c.B) { set_error("weight_group_stride < n_sample"); return FDG_E_INVALID; }
  return check_blocks(g, c, m, mc_T);
}

// ... and the stratified grouped calls': the stratified calls' NULL arrays, the grouped calls' cases (which end in the VEGAS calls'),
// then the strata and the per-hypercube arrays, [H][n_root + n_group].
int check_strat_grouped_call(const fdg_graph *g, const BinnedCall &c) {
  const StratRun &s = *c.sr;
  if (!s.strat || !s.d_cube || !s.d_sum || !s.d_sum2) { set_error("null strat, d_cube, d_cube_sum or d_cube_sum2"); return FDG_E_INVALID; }
  const int rc = check_grouped(g, c, nullptr, nullptr);
  return rc ? rc : check_strat_arrays(g, c, c.wg->n_group);
}

// What the descriptors of the observables and of the frequency observables are both checked for, in this order, each refusal in
// its caller's words: the three arrays, the number of rows against 1 .. n_max, every coefficient finite.
struct RowTexts { const char *null_array, *none, *many, *not_finite; };
int check_rows(const fdg_graph *g, const double *coef, const double *d_o, const double *d_c, uint32_t n_obs, uint32_t n_max, const RowTexts &t) {
  if (!coef || !d_o || !d_c) { set_error(t.null_array); return FDG_E_INVALID; }
  if (n_obs == 0) { set_error(t.none); return FDG_E_INVALID; }
  if (n_obs > n_max) { set_error(t.many); return FDG_E_UNSUPPORTED; }
  for (size_t i = 0; i < (size_t)n_obs * g->prog.R; ++i)
    if (!std::isfinite(coef[i])) { set_error(t.not_finite); return FDG_E_INVALID; }
  return FDG_OK;
}

// ... and the observables calls': the descriptor first (the coefficients need the handle's n_root), then the grouped calls' cases
// with wg optional and, through c.ob, d_acc and d_acc2 optional together.
int check_observables(const fdg_graph *g, const BinnedCall &c, const fdg_matsubara *m, const double *mc_T) {
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  const fdg_observables *o = c.ob ? c.ob->ob : nullptr;
  if (!o) { set_error("null observables"); return FDG_E_INVALID; }
  const int rc = check_rows(g, o->coef, o->d_obs, o->d_cov, o->n_obs, FDG_OBS_MAX,
                            {"null array in the observables", "n_obs == 0", "n_obs > FDG_OBS_MAX", "a coefficient of the observables is not finite"});
  if (rc) return rc;
  if (o->d_obs == o->d_cov) { set_error("d_obs and d_cov are the same buffer"); return FDG_E_INVALID; }
  for (const double *out : {c.d_acc, c.d_acc2})
    if (out && (out == o->d_obs || out == o->d_cov)) { set_error("d_obs or d_cov is the same buffer as d_acc or d_acc2"); return FDG_E_INVALID; }
  if (!c.d_acc != !c.d_acc2) { set_error("d_acc and d_acc2 go together"); return FDG_E_INVALID; }
  return check_grouped(g, c, m, mc_T, true);
}

// ... and the frequency-observables calls': the descriptor first, then the projection it stands on, then the observables calls'
// cases with ob optional (without ob: the grouped calls' with wg optional).  check_matsubara lets the four per-root arrays be NULL
// together when c.fo is set.
int check_freq_observables(const fdg_graph *g, const BinnedCall &c, const fdg_matsubara *m, const double *mc_T) {
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  const fdg_freq_observables *o = c.fo;
  if (!o) { set_error("null frequency observables"); return FDG_E_INVALID; }
  const int rc = check_rows(g, o->coef, o->d_fobs, o->d_fcov, o->n_obs, FDG_FREQ_OBS_MAX,
                            {"null array in the frequency observables", "n_obs == 0 in the frequency observables", "n_obs > FDG_FREQ_OBS_MAX",
                             "a coefficient of the frequency observables is not finite"});
  if (rc) return rc;
  if (!m) { set_error("null descriptor: the frequency observables need mz"); return FDG_E_INVALID; }
  const fdg_observables *ob = c.ob ? c.ob->ob : nullptr;
  const double *out[11] = {o->d_fcov, c.d_acc, c.d_acc2, c.vg ? c.vg->d_hist : nullptr, c.vg ? c.vg->d_hist_bin : nullptr,
                           m->d_acc_re, m->d_acc_im, m->d_acc2_re, m->d_acc2_im, ob ? ob->d_obs : nullptr, ob ? ob->d_cov : nullptr};
  for (int a = 0; a < 11; ++a)
    if (out[a] && (out[a] == o->d_fobs || (a && out[a] == o->d_fcov))) {
      set_error("d_fobs or d_fcov is the same buffer as another output of the call"); return FDG_E_INVALID;
    }
  return ob ? check_observables(g, c, m, mc_T) : check_grouped(g, c, m, mc_T, true);
}

// The chunk loop shared by the entry points (caller holds g->mu, stream bound): eval(c0, n, roots, ld) writes the roots of samples
// c0 .. c0 + n - 1 column-major into roots (root k of sample c0 + b at roots[k * ld + b]).  c.d_acc2 != null: the second moment too.
// c.vg != null (the VEGAS calls): after a chunk's moments pass the training pass runs over the same roots, its partials behind the
// moments' slab; with vg->d_hist_bin the discrete variable's pass follows, its partials behind the root list.
template <class Eval>
int run_binned(fdg_graph *g, const BinnedCall &c, Eval eval) {
  const uint32_t R = g->prog.R, n_bin = c.n_bin;
  const VegasRun *vg = c.vg;
  const hipStream_t st = (hipStream_t)c.stream;
  const BinnedPlan p = binned_plan(g, c.B, R, n_bin, c.d_acc2 != nullptr);
  const size_t root_bytes = page_up((size_t)p.Bc * R * sizeof(double)), slab_bytes = page_up(p.slab_alloc);
  // The grouped calls take the grouped instances only where the groups do not reduce to "one weight, every variable": the weight
  // columns with more than one group, the training passes also with one group whose mask leaves variables out.  Otherwise the call
  // is the ungrouped one: the same kernels on the same plan.  Which instances run depends on n_group and the masks' coverage, the
  // order of the sums on n_group alone.
  const fdg_weight_groups *wg = c.wg;
  const bool grp_w = wg && wg->n_group > 1;
  const bool grp_t = wg && vg && (grp_w || (~wg->var_mask[0] & (vg->D == 64 ? ~0ull : (1ull << vg->D) - 1ull)) != 0);
  const uint32_t NG = wg ? wg->n_group : 1u;
  const long wstride = wg ? (long)wg->weight_group_stride : 0;
  VegasPlan q;
  if (vg) q = vegas_plan(p, *vg, R, n_bin, grp_t ? NG : 1u);
  const MatsubaraRun *mz = c.mz;
  const bool proj = mz && mz->m->d_acc_re;      // (the frequency-observables calls may leave the four per-root arrays out)
  MatsubaraPlan mp;
  if (mz) mp = matsubara_plan(p, R, n_bin, mz->m->n_freq);
  // the projection's slab and table lie behind everything the call would reserve without it
  const size_t base_bytes = vg ? root_bytes + slab_bytes + q.slab_alloc + q.list_bytes + q.bin_slab_alloc
                               : mz ? root_bytes + slab_bytes : root_bytes + p.slab_alloc;
  // ... and the groups' table (gtab of fdg_binned_partials, then gstart[n_group + 1], then a byte per training histogram word:
  // 0 = its variable is trained by no group) behind that
  const size_t proj_bytes = mz ? base_bytes + mp.slab_alloc + mp.tab_bytes : base_bytes;
  const size_t gtab_words = (size_t)R + (size_t)p.n_slice * kGrpEntry + kGrpCols + 1u;
  const size_t grp_bytes = (grp_w || grp_t) ? page_up(gtab_words * 4u + (vg ? (size_t)vg->D * vg->G : 0)) : 0;
  // ... and the observables' slab and tables behind that, the frequency observables' behind those
  const fdg_observables *ob = c.ob ? c.ob->ob : nullptr;
  const fdg_freq_observables *fo = c.fo;
  ObsPass op, fp;
  if (ob) op.set_up(g, p, n_bin, ob->coef, ob->n_obs, nullptr, wg);
  if (fo) fp.set_up(g, p, n_bin, fo->coef, fo->n_obs, mz->m, wg);
  // ... and the record buffers of the per-hypercube pass behind that
  const StratRun *sr = c.sr;
  // (with several groups one column per group behind the roots', the GRP instances; else the one coef column of the ungrouped call,
  // whose root list a single group's is)
  StratPlan sp;
  VegasStrat sv = {};
  const bool grp_s = sr && grp_w;
  uint32_t semask = 0;                                     // grp_s: bit gi set = group gi has a root that exists
  if (sr) {
    sv = vegas_strat(sr->strat, vg->D);
    sp = strat_plan(p, c.B, R, sv.H, grp_s ? NG : 1u);
  }
  int rc = ensure_root_scratch(g, proj_bytes + grp_bytes + op.bytes + fp.bytes + sp.bytes);
  if (rc) return rc;
  double *roots = (double *)g->d_ws2, *partial = (double *)((char *)g->d_ws2 + root_bytes);
  const uint8_t *live = nullptr;
  rc = root_live_mask(g, &live);
  if (rc) return rc;
  raise_lds_limits();
  uint32_t *d_gtab = nullptr, *d_gstart = nullptr;
  const uint8_t *d_hlive = nullptr;
  VegasVarGroups vgm = {};
  std::vector<uint32_t> gstart(kGrpCols + 1u, 0u);         // bounds of every group's roots in the lists sorted by (group, root)
  if (grp_w || grp_t) {
    d_gtab = (uint32_t *)((char *)g->d_ws2 + proj_bytes);
    d_gstart = d_gtab + R + (size_t)p.n_slice * kGrpEntry;
    std::vector<uint32_t> hg(grp_bytes / 4u, 0u);
    auto exists = [&](uint32_t k) { return g->prog.root_slot[k] != FDG_NO_ROOT; };
    uint32_t near = 0;
    for (uint32_t k = R; k-- > 0;)
      if (exists(k)) near = wg->root_group[k];
    for (uint32_t k = 0; k < R; ++k) hg[k] = near = exists(k) ? wg->root_group[k] : near;
    for (uint32_t s = 0; s < p.n_slice; ++s) {
      uint32_t *e = hg.data() + R + (size_t)s * kGrpEntry, &n_col = e[0];
      for (uint32_t kk = 0; kk < p.rs && s * p.rs + kk < R; ++kk) {
        const uint32_t gk = hg[s * p.rs + kk];
        uint32_t at = 0;
        while (at < n_col && e[1 + at] != gk) ++at;
        if (at == n_col) e[1 + n_col++] = gk;
        e[1 + kGrpCols + kk] = at;
      }
    }
    for (uint32_t k = 0; k < R; ++k)
      if (exists(k)) ++gstart[wg->root_group[k] + 1u];
    for (uint32_t gi = 0; gi < NG; ++gi) gstart[gi + 1u] += gstart[gi];
    std::copy(gstart.begin(), gstart.end(), hg.begin() + (d_gstart - d_gtab));
    for (uint32_t gi = 0; gi < NG; ++gi)
      if (gstart[gi + 1u] > gstart[gi]) semask |= 1u << gi;
    if (grp_t) {
      uint8_t *hl = (uint8_t *)(hg.data() + gtab_words);
      bool dead = false;
      for (uint32_t d = 0; d < vg->D; ++d) {
        for (uint32_t gi = 0; gi < NG; ++gi)
          if (((wg->var_mask[gi] >> d) & 1u) && gstart[gi + 1u] > gstart[gi]) vgm.g[d] |= (uint8_t)(1u << gi);
        dead = dead || !vgm.g[d];
        std::fill(hl + (size_t)d * vg->G, hl + (size_t)(d + 1u) * vg->G, vgm.g[d] ? 1 : 0);
      }
      if (dead) d_hlive = (const uint8_t *)(d_gtab + gtab_words);
    }
    HIP_TRY(hipMemcpyAsync(d_gtab, hg.data(), grp_bytes, hipMemcpyHostToDevice, st));
  }
  double *vpartial = nullptr, *d_coef = nullptr, *bpartial = nullptr;
  uint32_t *d_kidx = nullptr, n_live = 0;
  if (vg) {
    // the roots that exist, ascending, and their factors: one small upload per call (pageable memory: staged before the call returns)
    vpartial = (double *)((char *)partial + slab_bytes);
    d_coef = (double *)((char *)vpartial + q.slab_alloc);
    d_kidx = (uint32_t *)(d_coef + R);
    bpartial = (double *)((char *)d_coef + q.list_bytes);
    std::vector<double> hc;
    std::vector<uint32_t> hk;
    // (the grouped training passes: sorted by (group, root), group gi's part at gstart[gi] .. gstart[gi + 1])
    for (uint32_t gi = 0; gi < (grp_t ? NG : 1u); ++gi)
      for (uint32_t k = 0; k < R; ++k)
        if (g->prog.root_slot[k] != FDG_NO_ROOT && (!grp_t || wg->root_group[k] == gi)) { hk.push_back(k); hc.push_back(vg->coef ? vg->coef[k] : 1.0); }
    n_live = (uint32_t)hk.size();
    if (n_live) {
      HIP_TRY(hipMemcpyAsync(d_coef, hc.data(), n_live * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_kidx, hk.data(), n_live * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
  }
  double *mpartial = nullptr, *d_mtab = nullptr;
  if (mz) {
    // the multipliers of the frequencies, then the roots' time components (0-based; 0 for a root that does not exist): one small upload
    const fdg_matsubara &m = *mz->m;
    mpartial = (double *)((char *)g->d_ws2 + base_bytes);
    d_mtab = (double *)((char *)mpartial + mp.slab_alloc);
    std::vector<double> hm(FDG_MATSUBARA_FREQ_MAX + R, 0.0);
    int32_t *hio = (int32_t *)(hm.data() + FDG_MATSUBARA_FREQ_MAX);
    for (uint32_t f = 0; f < m.n_freq; ++f) hm[f] = matsubara_multiplier(m.freq[f], m.fermionic);
    for (uint32_t k = 0; k < R; ++k) {
      const bool is = g->prog.root_slot[k] != FDG_NO_ROOT;
      hio[k] = is ? m.root_tau_in[k] - 1 : 0;
      hio[R + k] = is ? m.root_tau_out[k] - 1 : 0;
    }
    HIP_TRY(hipMemcpyAsync(d_mtab, hm.data(), hm.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (op.P) rc = op.place((char *)g->d_ws2 + proj_bytes + grp_bytes, st);
  if (!rc && fp.P) rc = fp.place((char *)g->d_ws2 + proj_bytes + grp_bytes + op.bytes, st);
  if (rc) return rc;
  // a chunk's launch of either pass (one weight column per group; without groups one, or none when the call has no weights)
  auto obs_launch = [&](const ObsPass &o, long c0, long n, long ntile, const int32_t *bins, const double *w, int first) {
    const ObsPlan &q = o.q;
    const dim3 grid(q.n_seg * q.n_fslice * q.n_cslice);
    const size_t lds = q.hist_bytes + (size_t)o.t.need * 2048u;
    const uint32_t n_wcol = w ? (grp_w ? NG : 1u) : 0u;
    const long seg_tiles = (ntile + q.n_seg - 1) / q.n_seg;
    if (!o.freq)
      hipLaunchKernelGGL(fdg_obs_partials, grid, dim3(256), lds, st, roots, (long)p.Bc, n, bins, c.bin_base, n_bin, w, wstride, n_wcol, q.V, q.cs,
                         q.n_cslice, seg_tiles, o.partial, first, o.d_utab, o.d_dtab);
    else
      hipLaunchKernelGGL(fdg_fobs_partials, grid, dim3(256), lds, st, roots, (long)p.Bc, n, bins, c.bin_base, n_bin, w, wstride, n_wcol,
                         mz->d_T + c0 * mz->ts, (long)mz->ts, (long)mz->tc, mz->m->beta, o.n_freq, q.fs, q.n_fslice, q.V, q.cs, q.n_cslice,
                         seg_tiles, o.partial, first, o.d_utab, o.d_dtab);
    HIP_TRY(hipGetLastError());
    return FDG_OK;
  };
  // the record buffers {keys, values, slots} a, b (the levels) and c (the chunks)
  struct StratBuf { int32_t *key; double *val; long cap; } sa = {}, sb = {}, sc = {};
  if (sr) {
    char *at = (char *)g->d_ws2 + proj_bytes + grp_bytes + op.bytes + fp.bytes;
    for (auto bc : {std::make_pair(&sa, sp.cap_a), std::make_pair(&sb, sp.cap_b), std::make_pair(&sc, sp.cap_c)}) {
      *bc.first = {(int32_t *)at, (double *)(at + page_up((size_t)bc.second * 4u)), bc.second};
      at += StratPlan::buf_bytes(bc.second, sp.V2);
    }
  }
  // the levels above `in` (n_slot records): interior runs are written, edge runs go up until one wave is left; that wave writes
  // everything (last) or leaves its two edge records in slots 2 c, 2 c + 1 of the chunks' buffer
  auto strat_levels = [&](StratBuf in, long n_slot, bool last, long chunk) {
    for (;;) {
      const long nw = (n_slot + 63) / 64;
      const bool top = nw == 1;
      const StratBuf out = !top ? (in.key == sa.key ? sb : sa) : sc;
      hipLaunchKernelGGL(grp_s ? fdg_strat_stitch<true> : fdg_strat_stitch<false>, dim3((unsigned)((nw + kBinWaves - 1) / kBinWaves), sp.n_grp),
                         dim3(256), 0, st, in.key, in.val, in.cap, n_slot, R, live, n_live, sr->d_sum, sr->d_sum2, (top && last) ? 1 : 0,
                         out.key, out.val, out.cap, top ? 2 * chunk : 0L, NG, semask);
      HIP_TRY(hipGetLastError());
      if (top) return FDG_OK;
      in = out;
      n_slot = 2 * nw;
    }
  };
  const MatsubaraKernel mpass = matsubara_kernel(mp, grp_w);
  const PartialsKernel pass = partials_kernel(p, grp_w);
  const uint32_t n_grp = p.mode == kSplit ? 2 * p.n_slice : p.n_slice;
  for (long c0 = 0; c0 < (long)c.B; c0 += p.Bc) {
    const long n = std::min<long>(p.Bc, (long)c.B - c0), ntile = (n + 63) / 64;
    const int first = c0 == 0;
    const int32_t *bins = c.d_bin ? c.d_bin + c0 : nullptr;
    const double *w = c.d_weight ? c.d_weight + c0 : nullptr;
    rc = eval(c0, n, roots, p.Bc);
    if (rc) return rc;
    if (c.d_acc) {
      hipLaunchKernelGGL(pass, dim3(p.n_seg * n_grp), dim3(256), p.lds, st, roots, (long)p.Bc, n, bins, c.bin_base, n_bin, w, R, p.n_slice,
                         (ntile + p.n_seg - 1) / p.n_seg, partial, first, d_gtab, wstride);
      HIP_TRY(hipGetLastError());
    }
    for (const ObsPass *o : {&op, &fp})
      if (o->P) {
        rc = obs_launch(*o, c0, n, ntile, bins, w, first);
        if (rc) return rc;
      }
    if (proj) {
      hipLaunchKernelGGL(mpass, dim3(mp.n_seg * mp.n_grp), dim3(64 * mp.nw), mp.lds, st, roots, (long)p.Bc, n, bins, c.bin_base, n_bin, w,
                         mz->d_T + c0 * mz->ts, (long)mz->ts, (long)mz->tc, d_mtab, mz->m->beta, mz->m->n_freq, R, mp.rs, mp.fs, mp.n_fslice,
                         (ntile + mp.n_seg - 1) / mp.n_seg, mpartial, first, d_gtab, wstride);
      HIP_TRY(hipGetLastError());
    }
    if (vg) {
      const double *cf = vg->coef ? d_coef : nullptr;
      // (the calls without a discrete variable carry no bin vector: null, base 0, one bin)
      const auto tpass = sr      ? (grp_t ? fdg_vegas_partials<0, true, true> : fdg_vegas_partials<0, false, true>)
                         : grp_t ? (vg->binned ? fdg_vegas_partials<1, true> : fdg_vegas_partials<0, true>)
                                 : (vg->binned ? fdg_vegas_partials<1> : fdg_vegas_partials<0>);
      hipLaunchKernelGGL(tpass, dim3(q.n_seg * q.n_slice), dim3(256), q.lds, st, roots, (long)p.Bc, n, w, d_kidx, cf, n_live, vg->seed,
                         vg->offset + (uint64_t)c0, vg->D, vg->G, q.ds, q.n_slice, (ntile + q.n_seg - 1) / q.n_seg, vpartial, first, bins,
                         c.bin_base, n_bin, d_gstart, NG, wstride, vgm, sr ? sr->d_cube + c0 : nullptr, sv);
      HIP_TRY(hipGetLastError());
      if (sr) {
        // the per-hypercube pass, the chunk's last reader of the roots: level 0 over the samples, then the levels over its records
        const bool top = ntile == 1;
        const StratBuf out = top ? sc : sa;
        hipLaunchKernelGGL(grp_s ? fdg_strat_partials<true> : fdg_strat_partials<false>,
                           dim3((unsigned)((ntile + kBinWaves - 1) / kBinWaves), sp.n_grp), dim3(256), 0, st, roots, (long)p.Bc, n,
                           sr->d_cube + c0, sp.H, w, d_kidx, cf, n_live, R, live, sr->d_sum, sr->d_sum2, out.key, out.val, out.cap,
                           top ? 2 * (c0 / p.Bc) : 0L, d_gtab, d_gstart, NG, wstride, semask);
        HIP_TRY(hipGetLastError());
        if (!top) {
          rc = strat_levels(sa, 2 * ntile, false, c0 / p.Bc);
          if (rc) return rc;
        }
      }
      if (vg->d_hist_bin) {
        hipLaunchKernelGGL(grp_t ? fdg_vegas_bin_partials<true> : fdg_vegas_bin_partials<false>, dim3(q.bin_seg), dim3(256),
                           (size_t)n_bin * 8u, st, roots, (long)p.Bc, n, bins, c.bin_base, n_bin, w, d_kidx, cf, n_live,
                           (ntile + q.bin_seg - 1) / q.bin_seg, bpartial, first, d_gstart, NG, wstride);
        HIP_TRY(hipGetLastError());
      }
    }
  }
  const long ncol = (long)n_bin * R;
  uint32_t C = 1;
  while (C < 64 && (long)C < ncol) C <<= 1;
  if (c.d_acc) rc = reduce_partials(partial, p.n_seg, ncol, R, C, c.d_acc, c.d_acc2, live, st);
  // (the observables: C, and with it the order of the segments' sum, is the moments reduce's own: a unit row then carries the moments
  // call's bits; the frequency observables: C by the same rule from their own columns)
  if (!rc && ob) rc = op.reduce(n_bin, C, ob->d_obs, ob->d_cov, st);
  if (!rc && fo) rc = fp.reduce(n_bin, 0u, fo->d_fobs, fo->d_fcov, st);
  if (!rc && proj) {
    // the four arrays += the segments' partials [segment][4][bin][frequency][root], in segment order: first both first moments, then both second
    const long mcol = ncol * mz->m->n_freq;
    const fdg_matsubara &m = *mz->m;
    double *out[2][2] = {{m.d_acc_re, m.d_acc_im}, {m.d_acc2_re, m.d_acc2_im}};
    for (int h = 0; h < 2; ++h) {
      hipLaunchKernelGGL(fdg_binned_reduce, dim3((unsigned)((mcol + 63) / 64), 2), dim3(256), 0, st, mpartial + (size_t)(2 * h) * mcol, mp.n_seg,
                         4 * mcol, mcol, R, 64u, out[h][0], out[h][1], live);
      HIP_TRY(hipGetLastError());
    }
  }
  // hist[d][c] and hist_bin[j] += the segments' partials, in segment order
  // (a variable that no group trains is not added to: the byte table stands in for the roots' mask, R = the histogram's size)
  if (!rc && vg) rc = reduce_partials(vpartial, q.n_seg, (long)vg->D * vg->G, d_hlive ? vg->D * vg->G : 1u, 64u, vg->d_hist, nullptr, d_hlive, st);
  if (!rc && vg && vg->d_hist_bin) rc = reduce_partials(bpartial, q.bin_seg, (long)n_bin, 1u, 64u, vg->d_hist_bin, nullptr, nullptr, st);
  // the chunks' edge records through the same levels; the last wave writes every run
  if (!rc && sr) rc = strat_levels(sc, 2 * sp.n_chunk, true, 0);
  return rc;
}

// The body every accumulate entry point shares after its own argument checks: null_input is the call's "an input array is missing",
// locked_check() what only the handle can tell once it is locked, eval the chunk evaluator of run_binned.
template <class Check, class Eval>
int accumulate(fdg_graph *g, const BinnedCall &c, bool null_input, Check locked_check, Eval eval) {
  if (null_input) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (c.B == 0 || g->prog.R == 0) return FDG_OK;
  std::lock_guard<std::mutex> lk(g->mu);
  fdg::KnobScope knob_scope(&g->knobs);
  int rc = locked_check();
  if (rc) return rc;
  rc = ensure_device(g);
  if (rc) return rc;
  rc = fdg_bind_stream_ws(g, c.stream);
  if (rc) return rc;
  return run_binned(g, c, eval);
}

// The leaf form of the calls (fdg_accumulate_device_*), after their own checks
int accumulate_leaf(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const BinnedCall &c) {
  const hipStream_t st = (hipStream_t)c.stream;
  return accumulate(
      g, c, g->prog.L && !d_leaf,
      [&] {
        if ((c.d_acc2 || c.mz || c.ob) && lts && !(g->isa && !g->code_object.empty())) {     // (the binned call finds it in the first chunk's evaluation)
          set_error("tile-major batches need a handle specialised with FDG_SPEC_ISA"); return FDG_E_UNSUPPORTED;
        }
        return FDG_OK;
      },
      [&](long c0, long n, double *roots, long ld) {
        const double *lf = lts ? d_leaf + (size_t)(c0 / 64) * (size_t)lts : d_leaf + c0 * ss;
        return fdg_run_locked(g, 0, lf, ss, ls, roots, 1, ld, nullptr, nullptr, n, st, lts, 0);
      });
}

// The Monte-Carlo form (fdg_mc_accumulate_device_*), after their own checks
int accumulate_mc(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc, double kF, double beta,
                  double lambda, const BinnedCall &c) {
  const hipStream_t st = (hipStream_t)c.stream;
  return accumulate(
      g, c, !d_K || !d_T,
      [&] {
        if (g->mc_route == 0) { set_error("fdg_graph_specialize_fused has not been called on this handle"); return FDG_E_INVALID; }
        return FDG_OK;
      },
      [&](long c0, long n, double *roots, long ld) {
        return fdg_mc_run_locked(g, 0, d_K + c0 * ks, ks, kc, d_T + c0 * ts, ts, tc, kF, beta, lambda, roots, 1, ld, nullptr, nullptr, n, st);
      });
}

// The samplers' shared checks (null_buffer: one of the call's required arrays is missing) and column list.
int check_sampler(int64_t B, bool null_buffer, uint32_t n_dim, uint32_t n_grid) {
  if (B < 0) { set_error("n_sample < 0"); return FDG_E_INVALID; }
  if (null_buffer) { set_error("null device buffer"); return FDG_E_INVALID; }
  return check_vegas_map(n_dim, n_grid);
}

// What a sampler entry carries beside the map and the outputs; an entry leaves what it does not take at these defaults.
struct VegasSampleCall {
  // the discrete variable; d_cdf null: none, and the rest is ignored.  need_discrete (fdg_vegas_sample_device_discrete): d_cdf and
  // d_bin are required
  const double *d_cdf = nullptr;
  uint32_t n_bin = 1;
  int32_t bin_base = 0;
  const double *d_ext = nullptr;
  uint32_t n_ext = 0;
  const uint32_t *ext_col = nullptr;
  int32_t *d_bin = nullptr;
  bool need_discrete = false;
  // the polar groups.  takes_polar (the _polar, _grouped and _strat_grouped entries): every written column is to be named once
  const fdg_vegas_polar *polar = nullptr;
  uint32_t n_polar = 0;
  bool takes_polar = false;
  // the weight groups: one jacobian per group
  bool grouped = false;
  const uint64_t *var_mask = nullptr;
  uint32_t n_group = 0;
  int64_t jac_group_stride = 0;
  // the strata
  bool stratified = false;
  const uint32_t *strat = nullptr;
  const int64_t *d_start = nullptr;
  int32_t *d_cube = nullptr;
};

// Every fdg_vegas_sample_device* entry: the checks in one order, then the instance of the sampler that reads what the call carries
// and nothing else (no polar group: no LDS and no group list, whichever entry was called).
int vegas_sample(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint64_t seed, uint64_t sample_offset, double *d_x,
                 int64_t x_sample_stride, int64_t x_col_stride, double *d_jac, int32_t *d_cell, int64_t B, void *stream, VegasSampleCall c) {
  const bool bad_discrete = c.need_discrete ? !c.d_cdf || !c.d_bin : c.d_cdf && !c.d_bin;
  int rc = check_sampler(B, !d_grid || !d_x || !d_jac || bad_discrete || (c.grouped && !c.var_mask), n_dim, n_grid);
  if (rc) return rc;
  if (!c.d_cdf) c.n_bin = 1, c.n_ext = 0;                 // no discrete variable: its arguments are ignored
  VegasDiscArgs da{c.d_cdf, c.n_bin, c.bin_base, c.d_ext, c.n_ext, {}, c.d_bin};
  rc = check_discrete_table(c.n_bin, FDG_BIN_MAX, "FDG_BIN_MAX", c.d_ext, c.n_ext, c.ext_col, da.ecol);
  if (rc) return rc;
  SamplerPolar pol;
  rc = parse_polar(c.polar, c.n_polar, n_dim, -1, pol);
  if (rc) return rc;
  const SamplerCols cols = sampler_cols(col, n_dim, pol.grouped);
  rc = c.takes_polar ? check_cols_once(cols, n_dim, pol, da.ecol, c.n_ext) : check_ext_cols(da.ecol, c.n_ext, cols, n_dim, 0, -1);
  if (rc) return rc;
  VegasGroupArgs ga = {};
  if (c.grouped) {
    if (c.n_group == 0) { set_error("n_group == 0"); return FDG_E_INVALID; }
    if (c.n_group > FDG_WEIGHT_GROUP_MAX) { set_error("n_group > FDG_WEIGHT_GROUP_MAX"); return FDG_E_UNSUPPORTED; }
    ga.n = c.n_group;
    ga.jstride = (long)c.jac_group_stride;
    for (uint32_t g = 0; g < c.n_group; ++g) {
      ga.m[g] = c.var_mask[g];
      if (n_dim < 64 && (c.var_mask[g] >> n_dim)) { set_error("var_mask names a variable >= n_dim"); return FDG_E_INVALID; }
      for (uint32_t pg = 0; pg < pol.n; ++pg) {
        const uint64_t bits = ((1ull << pol.dim[pg]) - 1ull) << pol.var[pg], has = c.var_mask[g] & bits;
        if (has && has != bits) { set_error("var_mask holds some but not all variables of a polar group"); return FDG_E_INVALID; }
      }
    }
    if (c.n_group > 1 && c.jac_group_stride < B) { set_error("jac_group_stride < n_sample"); return FDG_E_INVALID; }
  }
  VegasStratArgs sa = {};
  if (c.stratified) {
    if (!c.strat || !c.d_start || !c.d_cube) { set_error("null strat, d_start or d_cube"); return FDG_E_INVALID; }
    uint32_t H;
    rc = check_strat(c.strat, n_dim, &H);
    if (rc) return rc;
    sa = VegasStratArgs{vegas_strat(c.strat, n_dim), c.d_start, c.d_cube};
  }
  if (B == 0) return FDG_OK;
  const long grid = std::min<long>(((long)B + 255) / 256, 256L * 16);
  const size_t lds = (size_t)__builtin_popcountll(pol.grouped) * 256u * sizeof(double);
  auto launch = [&](auto polar, auto grp, auto stratified, auto disc) {
    constexpr bool P = decltype(polar)::value, Gr = decltype(grp)::value, S = decltype(stratified)::value, Dc = decltype(disc)::value;
    if constexpr (!(S && Dc)) {                            // (a stratified call has no discrete variable)
      const auto kernel = fdg_vegas_sample<P, Gr, S, Dc>;
      if constexpr (P) {
        static std::once_flag once;
        std::call_once(once, [&] {
          (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FDG_VEGAS_DIM_MAX * 256 * (int)sizeof(double));
          (void)hipGetLastError();
        });
      }
      // (the by-value arguments of the fullest instance -- cols, pol, the group masks and the strata -- come to about 1.4 KiB of the 4 KiB segment)
      hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), lds, (hipStream_t)stream, d_grid, n_dim, n_grid, cols, seed, sample_offset,
                         d_x, (long)x_sample_stride, (long)x_col_stride, d_jac, d_cell, (long)B, arg_if<Dc>(da), arg_if<P>(pol),
                         arg_if<Gr>(ga), arg_if<S>(sa));
    }
  };
  with_flag(pol.n != 0, [&](auto p) {
    with_flag(c.grouped, [&](auto g) {
      with_flag(c.stratified, [&](auto s) { with_flag(c.d_cdf != nullptr, [&](auto d) { launch(p, g, s, d); }); });
    });
  });
  HIP_TRY(hipGetLastError());
  return FDG_OK;
}

}  // namespace

extern "C" {

int fdg_accumulate_device_binned(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin, int32_t bin_base,
                                 uint32_t n_bin, const double *d_weight, double *d_acc, int64_t B, void *stream) {
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, nullptr, B, stream, nullptr};
  const int rc = check_call(g, c, false);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_binned(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                    double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                    const double *d_weight, double *d_acc, int64_t B, void *stream) {
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, nullptr, B, stream, nullptr};
  const int rc = check_call(g, c, false);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_moments(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin,
                                  int32_t bin_base, uint32_t n_bin, const double *d_weight, double *d_acc, double *d_acc2, int64_t B,
                                  void *stream) {
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, nullptr};
  const int rc = check_call(g, c, true);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_moments(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                     double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                     const double *d_weight, double *d_acc, double *d_acc2, int64_t B, void *stream) {
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, nullptr};
  const int rc = check_call(g, c, true);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_vegas(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const double *d_weight,
                                const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc,
                                double *d_acc2, double *d_hist, int64_t B, void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, false, nullptr};
  const BinnedCall c{nullptr, 0, 1, d_weight, d_acc, d_acc2, B, stream, &vg};
  const int rc = check_vegas(g, c);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_vegas(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                   double kF, double beta, double lambda, const double *d_weight, const double *coef, uint64_t seed,
                                   uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                   int64_t B, void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, false, nullptr};
  const BinnedCall c{nullptr, 0, 1, d_weight, d_acc, d_acc2, B, stream, &vg};
  const int rc = check_vegas(g, c);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_vegas_binned(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin,
                                       int32_t bin_base, uint32_t n_bin, const double *d_weight, const double *coef, uint64_t seed,
                                       uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                       double *d_hist_bin, int64_t B, void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, true, d_hist_bin};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, &vg};
  const int rc = check_vegas(g, c);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_vegas_binned(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                          double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                          const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                          uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin, int64_t B,
                                          void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, true, d_hist_bin};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, &vg};
  const int rc = check_vegas(g, c);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_strat(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const double *d_weight,
                                const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc,
                                double *d_acc2, double *d_hist, const uint32_t *strat, const int32_t *d_cube, double *d_cube_sum,
                                double *d_cube_sum2, int64_t B, void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, false, nullptr};
  const StratRun sr{strat, d_cube, d_cube_sum, d_cube_sum2};
  const BinnedCall c{nullptr, 0, 1, d_weight, d_acc, d_acc2, B, stream, &vg, nullptr, nullptr, nullptr, &sr};
  const int rc = check_strat_call(g, c);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_strat(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                   double kF, double beta, double lambda, const double *d_weight, const double *coef, uint64_t seed,
                                   uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                   const uint32_t *strat, const int32_t *d_cube, double *d_cube_sum, double *d_cube_sum2, int64_t B,
                                   void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, false, nullptr};
  const StratRun sr{strat, d_cube, d_cube_sum, d_cube_sum2};
  const BinnedCall c{nullptr, 0, 1, d_weight, d_acc, d_acc2, B, stream, &vg, nullptr, nullptr, nullptr, &sr};
  const int rc = check_strat_call(g, c);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_strat_grouped(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const double *d_weight,
                                        const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid,
                                        double *d_acc, double *d_acc2, double *d_hist, const uint32_t *strat, const int32_t *d_cube,
                                        double *d_cube_sum, double *d_cube_sum2, const fdg_weight_groups *wg, int64_t B, void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, false, nullptr};
  const StratRun sr{strat, d_cube, d_cube_sum, d_cube_sum2};
  const BinnedCall c{nullptr, 0, 1, d_weight, d_acc, d_acc2, B, stream, &vg, nullptr, wg, nullptr, &sr};
  const int rc = check_strat_grouped_call(g, c);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_strat_grouped(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                           double kF, double beta, double lambda, const double *d_weight, const double *coef, uint64_t seed,
                                           uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2,
                                           double *d_hist, const uint32_t *strat, const int32_t *d_cube, double *d_cube_sum,
                                           double *d_cube_sum2, const fdg_weight_groups *wg, int64_t B, void *stream) {
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, false, nullptr};
  const StratRun sr{strat, d_cube, d_cube_sum, d_cube_sum2};
  const BinnedCall c{nullptr, 0, 1, d_weight, d_acc, d_acc2, B, stream, &vg, nullptr, wg, nullptr, &sr};
  const int rc = check_strat_grouped_call(g, c);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

// The allocation of the next iteration's samples to the hypercubes; host only, fp64, in the order include/fdg.h states.
int fdg_strat_allocate(const double *cube_sum, const double *cube_sum2, uint32_t ld, uint32_t col, const int64_t *start_old, uint32_t H,
                       int64_t n_total, double beta, int64_t *start_new) {
  return fdg_strat_allocate_cols(cube_sum, cube_sum2, ld, &col, 1, start_old, H, n_total, beta, start_new);
}

int fdg_strat_allocate_cols(const double *cube_sum, const double *cube_sum2, uint32_t ld, const uint32_t *cols, uint32_t n_col,
                            const int64_t *start_old, uint32_t H, int64_t n_total, double beta, int64_t *start_new) {
  if (!start_new || !cols || (start_old && (!cube_sum || !cube_sum2))) { set_error("null argument"); return FDG_E_INVALID; }
  if (n_col == 0) { set_error("n_col == 0"); return FDG_E_INVALID; }
  if (H == 0) { set_error("H == 0"); return FDG_E_INVALID; }
  if (H > FDG_STRAT_CUBE_MAX) { set_error("H > FDG_STRAT_CUBE_MAX"); return FDG_E_UNSUPPORTED; }
  if (n_total < 2 * (int64_t)H) { set_error("n_total < 2 H"); return FDG_E_INVALID; }
  if (!(beta >= 0.0 && beta <= 1.0)) { set_error("beta outside [0, 1]"); return FDG_E_INVALID; }
  for (uint32_t i = 0; start_old && i < n_col; ++i)
    if (cols[i] >= ld) { set_error("col >= ld"); return FDG_E_INVALID; }
  const int64_t spare = n_total - 2 * (int64_t)H;
  std::vector<int64_t> cnt(H);
  std::vector<double> dh(H, 0.0);
  double S = 0.0;
  if (start_old) {
    const double n_old = (double)start_old[H];
    for (uint32_t h = 0; h < H; ++h) {
      const int64_t n_h = start_old[h + 1] - start_old[h];
      if (n_h < 2) { set_error("an old count below 2"); return FDG_E_INVALID; }
      const double nd = (double)n_h, fac = n_old / ((double)H * nd);
      double var = 0.0;                                     // the left fold over cols of each column's own var_h
      for (uint32_t i = 0; i < n_col; ++i) {
        const double s1 = cube_sum[(size_t)h * ld + cols[i]], s2 = cube_sum2[(size_t)h * ld + cols[i]];
        if (!std::isfinite(s1) || !std::isfinite(s2)) { set_error("a moment is not finite"); return FDG_E_INVALID; }
        const double vc = std::max(0.0, (s2 - s1 * s1 / nd) / (nd - 1.0)) / (fac * fac);
        var = i ? var + vc : vc;
      }
      dh[h] = var == 0.0 ? 0.0 : std::pow(var, beta / 2.0);
      S = h ? S + dh[h] : dh[h];
    }
  }
  if (!start_old || !(S > 0.0) || !std::isfinite(S) || beta == 0.0) {
    for (uint32_t h = 0; h < H; ++h) cnt[h] = 2 + spare / (int64_t)H;
  } else {
    for (uint32_t h = 0; h < H; ++h) cnt[h] = 2 + (int64_t)std::floor((double)spare * (dh[h] / S));
  }
  int64_t have = 0;
  for (uint32_t h = 0; h < H; ++h) have += cnt[h];
  for (uint32_t h = 0; have < n_total; h = (h + 1) % H) { ++cnt[h]; ++have; }
  for (uint32_t h = H; have > n_total;) {
    h = h ? h - 1 : H - 1;
    if (cnt[h] > 2) { --cnt[h]; --have; }
  }
  start_new[0] = 0;
  for (uint32_t h = 0; h < H; ++h) start_new[h + 1] = start_new[h] + cnt[h];
  return FDG_OK;
}

void fdg_matsubara_phase(double tau, double beta, int32_t n, int fermionic, double *s, double *c) {
  fdg_matsubara_phase_impl(tau, beta, n, fermionic, *s, *c);
}

int fdg_accumulate_device_matsubara(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin,
                                    int32_t bin_base, uint32_t n_bin, const double *d_weight, const double *coef, uint64_t seed,
                                    uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                    double *d_hist_bin, const fdg_matsubara *mz, int64_t B, void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const MatsubaraRun mr{mz, mz ? mz->d_T : nullptr, mz ? mz->t_sample_stride : 0, mz ? mz->t_comp_stride : 0};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, &mr};
  const int rc = check_matsubara(g, c, mz, nullptr);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_matsubara(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                       double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                       const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                       uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin,
                                       const fdg_matsubara *mz, int64_t B, void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const bool own_T = mz && mz->d_T;
  const MatsubaraRun mr{mz, own_T ? mz->d_T : d_T, own_T ? mz->t_sample_stride : ts, own_T ? mz->t_comp_stride : tc};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, &mr};
  const int rc = check_matsubara(g, c, mz, d_T);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_grouped(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin,
                                  int32_t bin_base, uint32_t n_bin, const double *d_weight, const double *coef, uint64_t seed,
                                  uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                  double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg, int64_t B, void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const MatsubaraRun mr{mz, mz ? mz->d_T : nullptr, mz ? mz->t_sample_stride : 0, mz ? mz->t_comp_stride : 0};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, mz ? &mr : nullptr, wg};
  const int rc = check_grouped(g, c, mz, nullptr);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_grouped(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                     double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                     const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                     uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin,
                                     const fdg_matsubara *mz, const fdg_weight_groups *wg, int64_t B, void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const bool own_T = mz && mz->d_T;
  const MatsubaraRun mr{mz, own_T ? mz->d_T : d_T, own_T ? mz->t_sample_stride : ts, own_T ? mz->t_comp_stride : tc};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, mz ? &mr : nullptr, wg};
  const int rc = check_grouped(g, c, mz, d_T);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_observables(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin,
                                      int32_t bin_base, uint32_t n_bin, const double *d_weight, const double *coef, uint64_t seed,
                                      uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist,
                                      double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg, const fdg_observables *ob,
                                      int64_t B, void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const MatsubaraRun mr{mz, mz ? mz->d_T : nullptr, mz ? mz->t_sample_stride : 0, mz ? mz->t_comp_stride : 0};
  const ObsRun orun{ob};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, mz ? &mr : nullptr, wg, &orun};
  const int rc = check_observables(g, c, mz, nullptr);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_observables(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                         double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                         const double *d_weight, const double *coef, uint64_t seed, uint64_t sample_offset, uint32_t n_dim,
                                         uint32_t n_grid, double *d_acc, double *d_acc2, double *d_hist, double *d_hist_bin,
                                         const fdg_matsubara *mz, const fdg_weight_groups *wg, const fdg_observables *ob, int64_t B,
                                         void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const bool own_T = mz && mz->d_T;
  const MatsubaraRun mr{mz, own_T ? mz->d_T : d_T, own_T ? mz->t_sample_stride : ts, own_T ? mz->t_comp_stride : tc};
  const ObsRun orun{ob};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, mz ? &mr : nullptr, wg, &orun};
  const int rc = check_observables(g, c, mz, d_T);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

int fdg_accumulate_device_freq_observables(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin,
                                           int32_t bin_base, uint32_t n_bin, const double *d_weight, const double *coef, uint64_t seed,
                                           uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2,
                                           double *d_hist, double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg,
                                           const fdg_observables *ob, const fdg_freq_observables *fo, int64_t B, void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const MatsubaraRun mr{mz, mz ? mz->d_T : nullptr, mz ? mz->t_sample_stride : 0, mz ? mz->t_comp_stride : 0};
  const ObsRun orun{ob};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, mz ? &mr : nullptr, wg,
                     ob ? &orun : nullptr, nullptr, fo};
  const int rc = check_freq_observables(g, c, mz, nullptr);
  return rc ? rc : accumulate_leaf(g, d_leaf, ss, ls, lts, c);
}

int fdg_mc_accumulate_device_freq_observables(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts,
                                              int64_t tc, double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base,
                                              uint32_t n_bin, const double *d_weight, const double *coef, uint64_t seed,
                                              uint64_t sample_offset, uint32_t n_dim, uint32_t n_grid, double *d_acc, double *d_acc2,
                                              double *d_hist, double *d_hist_bin, const fdg_matsubara *mz, const fdg_weight_groups *wg,
                                              const fdg_observables *ob, const fdg_freq_observables *fo, int64_t B, void *stream) {
  const bool train = n_dim != 0 || d_hist;
  const VegasRun vg{coef, seed, sample_offset, n_dim, n_grid, d_hist, d_bin != nullptr, d_hist_bin};
  const bool own_T = mz && mz->d_T;
  const MatsubaraRun mr{mz, own_T ? mz->d_T : d_T, own_T ? mz->t_sample_stride : ts, own_T ? mz->t_comp_stride : tc};
  const ObsRun orun{ob};
  const BinnedCall c{d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream, train ? &vg : nullptr, mz ? &mr : nullptr, wg,
                     ob ? &orun : nullptr, nullptr, fo};
  const int rc = check_freq_observables(g, c, mz, d_T);
  return rc ? rc : accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, c);
}

// The six sampler entries: each names what it carries and goes through vegas_sample.
int fdg_vegas_sample_device(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, uint64_t seed, uint64_t sample_offset,
                            double *d_x, int64_t x_sample_stride, int64_t x_col_stride, double *d_jac, int32_t *d_cell, int64_t B,
                            void *stream) {
  return vegas_sample(d_grid, n_dim, n_grid, col, seed, sample_offset, d_x, x_sample_stride, x_col_stride, d_jac, d_cell, B, stream, {});
}

int fdg_vegas_sample_device_strat(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const uint32_t *strat,
                                  const int64_t *d_start, uint64_t seed, uint64_t sample_offset, double *d_x, int64_t x_sample_stride,
                                  int64_t x_col_stride, double *d_jac, int32_t *d_cube, int32_t *d_cell, int64_t B, void *stream) {
  VegasSampleCall c;
  c.stratified = true, c.strat = strat, c.d_start = d_start, c.d_cube = d_cube;
  return vegas_sample(d_grid, n_dim, n_grid, col, seed, sample_offset, d_x, x_sample_stride, x_col_stride, d_jac, d_cell, B, stream, c);
}

int fdg_vegas_sample_device_discrete(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const double *d_cdf,
                                     uint32_t n_bin, int32_t bin_base, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                     uint64_t seed, uint64_t sample_offset, double *d_x, int64_t x_sample_stride, int64_t x_col_stride,
                                     double *d_jac, int32_t *d_bin, int32_t *d_cell, int64_t B, void *stream) {
  VegasSampleCall c{d_cdf, n_bin, bin_base, d_ext, n_ext, ext_col, d_bin};
  c.need_discrete = true;
  return vegas_sample(d_grid, n_dim, n_grid, col, seed, sample_offset, d_x, x_sample_stride, x_col_stride, d_jac, d_cell, B, stream, c);
}

int fdg_vegas_sample_device_polar(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const double *d_cdf,
                                  uint32_t n_bin, int32_t bin_base, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                  const fdg_vegas_polar *polar, uint32_t n_polar, uint64_t seed, uint64_t sample_offset, double *d_x,
                                  int64_t x_sample_stride, int64_t x_col_stride, double *d_jac, int32_t *d_bin, int32_t *d_cell, int64_t B,
                                  void *stream) {
  VegasSampleCall c{d_cdf, n_bin, bin_base, d_ext, n_ext, ext_col, d_bin};
  c.polar = polar, c.n_polar = n_polar, c.takes_polar = true;
  return vegas_sample(d_grid, n_dim, n_grid, col, seed, sample_offset, d_x, x_sample_stride, x_col_stride, d_jac, d_cell, B, stream, c);
}

int fdg_vegas_sample_device_grouped(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col, const double *d_cdf,
                                    uint32_t n_bin, int32_t bin_base, const double *d_ext, uint32_t n_ext, const uint32_t *ext_col,
                                    const fdg_vegas_polar *polar, uint32_t n_polar, const uint64_t *var_mask, uint32_t n_group,
                                    int64_t jac_group_stride, uint64_t seed, uint64_t sample_offset, double *d_x, int64_t x_sample_stride,
                                    int64_t x_col_stride, double *d_jac, int32_t *d_bin, int32_t *d_cell, int64_t B, void *stream) {
  VegasSampleCall c{d_cdf, n_bin, bin_base, d_ext, n_ext, ext_col, d_bin};
  c.polar = polar, c.n_polar = n_polar, c.takes_polar = true;
  c.grouped = true, c.var_mask = var_mask, c.n_group = n_group, c.jac_group_stride = jac_group_stride;
  return vegas_sample(d_grid, n_dim, n_grid, col, seed, sample_offset, d_x, x_sample_stride, x_col_stride, d_jac, d_cell, B, stream, c);
}

int fdg_vegas_sample_device_strat_grouped(const double *d_grid, uint32_t n_dim, uint32_t n_grid, const uint32_t *col,
                                          const fdg_vegas_polar *polar, uint32_t n_polar, const uint64_t *var_mask, uint32_t n_group,
                                          int64_t jac_group_stride, const uint32_t *strat, const int64_t *d_start, uint64_t seed,
                                          uint64_t sample_offset, double *d_x, int64_t x_sample_stride, int64_t x_col_stride, double *d_jac,
                                          int32_t *d_cube, int32_t *d_cell, int64_t B, void *stream) {
  VegasSampleCall c;
  c.polar = polar, c.n_polar = n_polar, c.takes_polar = true;
  c.grouped = var_mask || n_group;                        // neither: one jacobian, the full fold (polar without groups)
  c.var_mask = var_mask, c.n_group = n_group, c.jac_group_stride = jac_group_stride;
  c.stratified = true, c.strat = strat, c.d_start = d_start, c.d_cube = d_cube;
  return vegas_sample(d_grid, n_dim, n_grid, col, seed, sample_offset, d_x, x_sample_stride, x_col_stride, d_jac, d_cell, B, stream, c);
}

void fdg_sincos(double x, double *s, double *c) { fdg_sincos_impl(x, *s, *c); }

// Lepage's refinement of the map from the training histogram; host only, fp64, in the order include/fdg.h states.
int fdg_vegas_refine(double *grid, const double *hist, uint32_t n_dim, uint32_t n_grid, double alpha) {
  if (!grid || !hist) { set_error("null argument"); return FDG_E_INVALID; }
  const int rc = check_vegas_map(n_dim, n_grid);
  if (rc) return rc;
  if (!(alpha >= 0.0 && alpha <= 2.0)) { set_error("alpha outside [0, 2]"); return FDG_E_INVALID; }
  const uint32_t G = n_grid;
  for (size_t i = 0; i < (size_t)n_dim * G; ++i)
    if (!(hist[i] >= 0.0) || !std::isfinite(hist[i])) { set_error("histogram entry negative or not finite"); return FDG_E_INVALID; }
  if (alpha == 0.0 || G == 1) return FDG_OK;
  std::vector<double> out(grid, grid + (size_t)n_dim * (G + 1)), sm(G), w(G);
  for (uint32_t d = 0; d < n_dim; ++d) {
    const double *h = hist + (size_t)d * G, *e = grid + (size_t)d * (G + 1);
    double *ne = out.data() + (size_t)d * (G + 1);
    double total = 0.0;
    for (uint32_t i = 0; i < G; ++i) total += h[i];
    if (!(total > 0.0)) continue;
    sm[0] = (7.0 * h[0] + h[1]) / 8.0;
    sm[G - 1] = (h[G - 2] + 7.0 * h[G - 1]) / 8.0;
    for (uint32_t i = 1; i + 1 < G; ++i) sm[i] = (h[i - 1] + 6.0 * h[i] + h[i + 1]) / 8.0;
    double ssum = 0.0;
    for (uint32_t i = 0; i < G; ++i) ssum += sm[i];
    if (!(ssum > 0.0) || !std::isfinite(ssum)) { set_error("histogram sum overflows"); return FDG_E_INVALID; }
    double wsum = 0.0;
    for (uint32_t i = 0; i < G; ++i) {
      const double x = sm[i] / ssum;
      w[i] = x <= 0.0 ? 0.0 : x >= 1.0 ? 1.0 : std::pow((1.0 - x) / (-std::log(x)), alpha);
      wsum += w[i];
    }
    if (!(wsum > 0.0)) continue;
    const double delta = wsum / (double)G;
    uint32_t j = 0;
    double below = 0.0, cum = w[0];                       // sum of w before cell j, and through it
    for (uint32_t i = 1; i < G; ++i) {
      const double target = (double)i * delta;
      while (cum < target && j + 1 < G) { below = cum; cum += w[++j]; }
      const double frac = w[j] > 0.0 ? std::min(1.0, std::max(0.0, (target - below) / w[j])) : 1.0;
      ne[i] = e[j] + frac * (e[j + 1] - e[j]);
    }
    for (uint32_t i = 0; i < G; ++i)
      if (!(ne[i] < ne[i + 1])) { set_error("refined edges are not strictly increasing"); return FDG_E_INTERNAL; }
  }
  std::copy(out.begin(), out.end(), grid);
  return FDG_OK;
}

// The refinement of the discrete variable's probabilities; host only, fp64, in the order include/fdg.h states.
int fdg_vegas_refine_discrete(double *cdf, const double *hist_bin, uint32_t n_bin, double alpha, double floor) {
  if (!cdf || !hist_bin) { set_error("null argument"); return FDG_E_INVALID; }
  if (n_bin == 0) { set_error("n_bin == 0"); return FDG_E_INVALID; }
  if (n_bin > FDG_BIN_MAX) { set_error("n_bin > FDG_BIN_MAX"); return FDG_E_UNSUPPORTED; }
  if (!(alpha >= 0.0 && alpha <= 2.0)) { set_error("alpha outside [0, 2]"); return FDG_E_INVALID; }
  if (!(floor >= 0.0 && floor < 1.0)) { set_error("floor outside [0, 1)"); return FDG_E_INVALID; }
  if (cdf[0] != 0.0 || cdf[n_bin] != 1.0) { set_error("cdf does not run from 0 to 1"); return FDG_E_INVALID; }
  for (uint32_t j = 0; j < n_bin; ++j) {
    if (!(cdf[j] < cdf[j + 1])) { set_error("cdf is not strictly increasing"); return FDG_E_INVALID; }
    if (!(hist_bin[j] >= 0.0) || !std::isfinite(hist_bin[j])) { set_error("histogram entry negative or not finite"); return FDG_E_INVALID; }
  }
  if (alpha == 0.0 || n_bin == 1) return FDG_OK;
  std::vector<double> w(n_bin), out(n_bin + 1);
  double qsum = 0.0;
  for (uint32_t j = 0; j < n_bin; ++j) {
    w[j] = hist_bin[j] * (cdf[j + 1] - cdf[j]);
    qsum += w[j];
  }
  if (!(qsum > 0.0)) return FDG_OK;
  if (!std::isfinite(qsum)) { set_error("histogram sum overflows"); return FDG_E_INVALID; }
  double wsum = 0.0;
  for (uint32_t j = 0; j < n_bin; ++j) {
    const double s = w[j] / qsum;
    w[j] = s > 0.0 ? std::pow(s, alpha) : 0.0;
    wsum += w[j];
  }
  const double keep = 1.0 - floor, base = floor / (double)n_bin;
  out[0] = 0.0;
  for (uint32_t j = 0; j < n_bin; ++j) out[j + 1] = out[j] + (keep * w[j] / wsum + base);
  out[n_bin] = 1.0;
  for (uint32_t j = 0; j < n_bin; ++j)
    if (!(out[j] < out[j + 1])) { set_error("refined probabilities are not all positive"); return FDG_E_INTERNAL; }
  std::copy(out.begin(), out.end(), cdf);
  return FDG_OK;
}

}  // extern "C"
