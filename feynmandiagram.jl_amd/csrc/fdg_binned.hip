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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#define FDG_RUNTIME_TU 1
#include "fdg_internal.h"

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

// What a workgroup of the pass accumulates: the first moment (the binned call), both moments in one LDS, or one moment per root slice
// (slices n_slice .. 2 n_slice - 1 are the second moment's; the histograms of both do not fit the LDS).
enum BinMode { kFirst = 0, kBoth = 1, kSplit = 2 };

// One workgroup per (segment, root slice); roots of the chunk at root[k * ld + b], b < n.  bins == null: every sample is in bin 0.
template <int RS, int MODE>
__global__ void __launch_bounds__(256)
fdg_binned_partials(const double *__restrict__ root, long ld, long n, const int32_t *__restrict__ bins, int32_t bin_base, uint32_t n_bin,
                    const double *__restrict__ weight, uint32_t R, uint32_t n_slice, long seg_tiles, double *__restrict__ partial, int first) {
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
  const long ntile = (n + 63) / 64, t0 = (long)seg * seg_tiles, t1 = min(t0 + seg_tiles, ntile);
  const long rounds = t1 > t0 ? (t1 - t0 + kBinWaves - 1) / kBinWaves : 0;

  // this lane's sample of round r, loaded one round ahead without a branch (indices clamped into the chunk: every load is issued at once
  // and stays in flight while the round before is binned); whether the sample adds anything is decided when it is used
  int32_t bin_n;
  double w_n, r_n[RS];
  auto fetch = [&](long r) {
    const long b = min((t0 + r * (long)kBinWaves + wave) * 64 + lane, n - 1);
    bin_n = bins ? bins[b] : bin_base;
    w_n = weight ? weight[b] : 1.0;
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
    for (int kk = 0; kk < RS; ++kk) v[kk] = in ? w_n * r_n[kk] : 0.0;
    fetch(r + 1);                                         // the next round's loads are in flight while this one is binned

    const uint64_t valid = __ballot(key < kKeyInvalid);
    double s[RS] = {}, s2[RS] = {};                       // s2: kBoth only
    bool head = false;
    uint32_t j = 0;
    if (valid) {
      const uint32_t key0 = __shfl(key, 0);
      uint32_t src = lane;
      if (!(valid == ~0ull && __ballot((key >> 6) == (key0 >> 6)) == ~0ull)) {
        // bitonic sort of the 64 keys (unique: the lane is part of the key), ascending over the lanes
#pragma unroll
        for (uint32_t kb = 2; kb <= 64; kb <<= 1)
#pragma unroll
          for (uint32_t jb = kb >> 1; jb > 0; jb >>= 1) {
            const uint32_t other = __shfl_xor(key, (int)jb);
            const bool keep_min = ((lane & kb) == 0) == ((lane & jb) == 0);
            key = keep_min ? min(key, other) : max(key, other);
          }
        src = key & 63u;
      }
      j = key >> 6;
      const bool ok = key < kKeyInvalid;
      const uint32_t j_prev = __shfl_up(j, 1);
      const uint32_t j_next = __shfl_down(j, 1);
      head = ok && (lane == 0 || j_prev != j);
      const uint64_t tails = __ballot(!ok || lane == 63 || j_next != j);
      const uint32_t end = ok ? (uint32_t)__builtin_ctzll(tails & (~0ull << lane)) : lane;   // last lane of this lane's run
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
BinnedPlan binned_plan(const fdg_graph *g, int64_t B, uint32_t R, uint32_t n_bin, bool moments = false) {
  BinnedPlan p;
  p.Bc = std::max<long>(64, (long)((g->cfg.root_scratch_mb << 20) / (8ull * R)) & ~63l);
  p.Bc = std::min<long>(p.Bc, (long)((B + 63) & ~(int64_t)63));
  uint32_t rs = 16;
  while (rs > 1 && (size_t)n_bin * rs * 8u > kBinLdsBudget) rs >>= 1;
  while (rs > 1 && rs / 2 >= R) rs >>= 1;
  p.rs = rs;
  p.n_slice = (R + rs - 1) / rs;
  p.lds = (size_t)n_bin * rs * 8u;
  const size_t hist_bytes = (size_t)n_bin * R * 8u;
  const long by_size = std::max<long>(1, p.Bc / 64 / 16);            // at least 16 tiles (four rounds) per workgroup
  const long by_slab = std::max<long>(1, (long)(kBinSlabBytes / hist_bytes));
  const long by_blocks = std::max<long>(1, 2048 / (long)p.n_slice);
  p.n_seg = (uint32_t)std::min(std::min(by_size, by_slab), by_blocks);
  // the reservation grows with n_sample and n_bin only, so a later call that is not larger allocates nothing
  p.slab_alloc = std::max(hist_bytes, std::min(kBinSlabBytes, (size_t)by_size * hist_bytes));
  if (moments) {
    p.slab_alloc *= 2;                                                 // [segment][moment][bin][root]
    if ((size_t)n_bin * 16u <= (size_t)FDG_BIN_MAX * 8u) {             // both histograms of one root fit: kBoth, the same budget rule
      rs = 16;
      while (rs > 1 && (size_t)n_bin * rs * 16u > kBinLdsBudget) rs >>= 1;
      while (rs > 1 && rs / 2 >= R) rs >>= 1;
      p.mode = kBoth;
      p.lds = (size_t)n_bin * rs * 16u;
    } else {                                                           // n_bin > 8192: one root of one moment per workgroup
      rs = 1;
      p.mode = kSplit;
      p.lds = (size_t)n_bin * 8u;
    }
    p.rs = rs;
    p.n_slice = (R + rs - 1) / rs;
  }
  return p;
}

template <int RS, int MODE>
int launch_partials(const BinnedPlan &p, const double *roots, long n, const int32_t *bins, int32_t bin_base, uint32_t n_bin,
                    const double *weight, uint32_t R, double *partial, int first, hipStream_t st) {
  static std::once_flag lds_once;           // (histograms above 64 KiB: one root of up to FDG_BIN_MAX bins, 128 KiB of the CU's 160)
  std::call_once(lds_once, [] {
    (void)hipFuncSetAttribute((const void *)fdg_binned_partials<RS, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(FDG_BIN_MAX * 8));
    (void)hipGetLastError();
  });
  const long ntile = (n + 63) / 64, seg_tiles = (ntile + p.n_seg - 1) / p.n_seg;
  const uint32_t n_grp = MODE == kSplit ? 2 * p.n_slice : p.n_slice;
  hipLaunchKernelGGL((fdg_binned_partials<RS, MODE>), dim3(p.n_seg * n_grp), dim3(256), p.lds, st, roots, (long)p.Bc, n, bins, bin_base,
                     n_bin, weight, R, p.n_slice, seg_tiles, partial, first);
  HIP_TRY(hipGetLastError());
  return FDG_OK;
}

template <int MODE>
int binned_pass_rs(const BinnedPlan &p, const double *roots, long n, const int32_t *bins, int32_t bin_base, uint32_t n_bin,
                   const double *weight, uint32_t R, double *partial, int first, hipStream_t st) {
  switch (p.rs) {
    case 1: return launch_partials<1, MODE>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
    case 2: return launch_partials<2, MODE>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
    case 4: return launch_partials<4, MODE>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
    case 8: return launch_partials<8, MODE>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
    default: return launch_partials<16, MODE>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
  }
}

int binned_pass(const BinnedPlan &p, const double *roots, long n, const int32_t *bins, int32_t bin_base, uint32_t n_bin, const double *weight,
                uint32_t R, double *partial, int first, hipStream_t st) {
  if (p.mode == kBoth) return binned_pass_rs<kBoth>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
  if (p.mode == kSplit) return launch_partials<1, kSplit>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
  return binned_pass_rs<kFirst>(p, roots, n, bins, bin_base, n_bin, weight, R, partial, first, st);
}

// The checks every binned entry point makes before any device work.
int check_binned(const fdg_graph *g, const int32_t *d_bin, uint32_t n_bin, const double *d_acc, int64_t B) {
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  if (B < 0) { set_error("n_sample < 0"); return FDG_E_INVALID; }
  if (!d_bin || !d_acc) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (n_bin == 0) { set_error("n_bin == 0"); return FDG_E_INVALID; }
  if (n_bin > FDG_BIN_MAX) { set_error("n_bin > FDG_BIN_MAX"); return FDG_E_UNSUPPORTED; }
  return FDG_OK;
}

// ... and the moments entry points' (d_bin == NULL: every sample in bin 0, which needs n_bin == 1).
int check_moments(const fdg_graph *g, const int32_t *d_bin, uint32_t n_bin, const double *d_acc, const double *d_acc2, int64_t B) {
  if (!g) { set_error("null handle"); return FDG_E_INVALID; }
  if (B < 0) { set_error("n_sample < 0"); return FDG_E_INVALID; }
  if (!d_acc || !d_acc2) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (d_acc == d_acc2) { set_error("d_acc and d_acc2 are the same buffer"); return FDG_E_INVALID; }
  if (n_bin == 0) { set_error("n_bin == 0"); return FDG_E_INVALID; }
  if (!d_bin && n_bin != 1) { set_error("d_bin == NULL (one bin) needs n_bin == 1"); return FDG_E_INVALID; }
  if (n_bin > FDG_BIN_MAX) { set_error("n_bin > FDG_BIN_MAX"); return FDG_E_UNSUPPORTED; }
  return FDG_OK;
}

// The chunk loop shared by the entry points (caller holds g->mu, stream bound): eval(c0, n, roots, ld) writes the roots of samples
// c0 .. c0 + n - 1 column-major into roots (root k of sample c0 + b at roots[k * ld + b]).  d_acc2 != null: the second moment too.
template <class Eval>
int run_binned(fdg_graph *g, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin, const double *d_weight, double *d_acc, double *d_acc2,
               int64_t B, hipStream_t st, Eval eval) {
  const uint32_t R = g->prog.R;
  const BinnedPlan p = binned_plan(g, B, R, n_bin, d_acc2 != nullptr);
  const size_t root_bytes = ((size_t)p.Bc * R * sizeof(double) + 4095) & ~(size_t)4095;
  int rc = ensure_root_scratch(g, root_bytes + p.slab_alloc);
  if (rc) return rc;
  double *roots = (double *)g->d_ws2, *partial = (double *)((char *)g->d_ws2 + root_bytes);
  const uint8_t *live = nullptr;
  rc = root_live_mask(g, &live);
  if (rc) return rc;
  for (long c0 = 0; c0 < (long)B; c0 += p.Bc) {
    const long n = std::min<long>(p.Bc, (long)B - c0);
    rc = eval(c0, n, roots, p.Bc);
    if (rc) return rc;
    rc = binned_pass(p, roots, n, d_bin ? d_bin + c0 : nullptr, bin_base, n_bin, d_weight ? d_weight + c0 : nullptr, R, partial, c0 == 0, st);
    if (rc) return rc;
  }
  const long ncol = (long)n_bin * R;
  uint32_t C = 1;
  while (C < 64 && (long)C < ncol) C <<= 1;
  const uint32_t n_mom = d_acc2 ? 2 : 1;
  hipLaunchKernelGGL(fdg_binned_reduce, dim3((unsigned)((ncol + C - 1) / C), n_mom), dim3(256), 0, st, partial, p.n_seg, ncol * n_mom, ncol,
                     R, C, d_acc, d_acc2, live);
  HIP_TRY(hipGetLastError());
  return FDG_OK;
}

// fdg_accumulate_device_binned / _moments after their own checks
int accumulate_leaf(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin, int32_t bin_base,
                    uint32_t n_bin, const double *d_weight, double *d_acc, double *d_acc2, int64_t B, void *stream) {
  if (g->prog.L && !d_leaf) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (B == 0 || g->prog.R == 0) return FDG_OK;
  std::lock_guard<std::mutex> lk(g->mu);
  fdg::KnobScope knob_scope(&g->knobs);
  if (d_acc2 && lts && !(g->isa && !g->code_object.empty())) {     // (the binned call finds it in the first chunk's evaluation)
    set_error("tile-major batches need a handle specialised with FDG_SPEC_ISA"); return FDG_E_UNSUPPORTED;
  }
  int rc = ensure_device(g);
  if (rc) return rc;
  rc = fdg_bind_stream_ws(g, stream);
  if (rc) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return run_binned(g, d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, st, [&](long c0, long n, double *roots, long ld) {
    const double *lf = lts ? d_leaf + (size_t)(c0 / 64) * (size_t)lts : d_leaf + c0 * ss;
    return fdg_run_locked(g, 0, lf, ss, ls, roots, 1, ld, nullptr, nullptr, n, st, lts, 0);
  });
}

// fdg_mc_accumulate_device_binned / _moments after their own checks
int accumulate_mc(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc, double kF, double beta,
                  double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin, const double *d_weight, double *d_acc, double *d_acc2,
                  int64_t B, void *stream) {
  if (!d_K || !d_T) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (B == 0 || g->prog.R == 0) return FDG_OK;
  std::lock_guard<std::mutex> lk(g->mu);
  fdg::KnobScope knob_scope(&g->knobs);
  if (g->mc_route == 0) { set_error("fdg_graph_specialize_fused has not been called on this handle"); return FDG_E_INVALID; }
  int rc = ensure_device(g);
  if (rc) return rc;
  rc = fdg_bind_stream_ws(g, stream);
  if (rc) return rc;
  const hipStream_t st = (hipStream_t)stream;
  return run_binned(g, d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, st, [&](long c0, long n, double *roots, long ld) {
    return fdg_mc_run_locked(g, 0, d_K + c0 * ks, ks, kc, d_T + c0 * ts, ts, tc, kF, beta, lambda, roots, 1, ld, nullptr, nullptr, n, st);
  });
}

}  // namespace

extern "C" {

int fdg_accumulate_device_binned(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin, int32_t bin_base,
                                 uint32_t n_bin, const double *d_weight, double *d_acc, int64_t B, void *stream) {
  const int rc = check_binned(g, d_bin, n_bin, d_acc, B);
  if (rc) return rc;
  return accumulate_leaf(g, d_leaf, ss, ls, lts, d_bin, bin_base, n_bin, d_weight, d_acc, nullptr, B, stream);
}

int fdg_mc_accumulate_device_binned(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                    double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                    const double *d_weight, double *d_acc, int64_t B, void *stream) {
  const int rc = check_binned(g, d_bin, n_bin, d_acc, B);
  if (rc) return rc;
  return accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, d_bin, bin_base, n_bin, d_weight, d_acc, nullptr, B, stream);
}

int fdg_accumulate_device_moments(fdg_graph *g, const double *d_leaf, int64_t ss, int64_t ls, int64_t lts, const int32_t *d_bin,
                                  int32_t bin_base, uint32_t n_bin, const double *d_weight, double *d_acc, double *d_acc2, int64_t B,
                                  void *stream) {
  const int rc = check_moments(g, d_bin, n_bin, d_acc, d_acc2, B);
  if (rc) return rc;
  return accumulate_leaf(g, d_leaf, ss, ls, lts, d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream);
}

int fdg_mc_accumulate_device_moments(fdg_graph *g, const double *d_K, int64_t ks, int64_t kc, const double *d_T, int64_t ts, int64_t tc,
                                     double kF, double beta, double lambda, const int32_t *d_bin, int32_t bin_base, uint32_t n_bin,
                                     const double *d_weight, double *d_acc, double *d_acc2, int64_t B, void *stream) {
  const int rc = check_moments(g, d_bin, n_bin, d_acc, d_acc2, B);
  if (rc) return rc;
  return accumulate_mc(g, d_K, ks, kc, d_T, ts, tc, kF, beta, lambda, d_bin, bin_base, n_bin, d_weight, d_acc, d_acc2, B, stream);
}

}  // extern "C"
