// Observables of the Markov chain: sums of roots with their covariance (include/fdg.h: fdg_chain_reduce_device_observables; DESIGN.md
// 8s).  An observable is linear in the walkers' sums, so nothing here touches a step: one reduction behind the chain forms, per
// walker b, O_m(b) = sum_c coef[m][c] A_{col_base + c}(b) and the normalisation O_M(b), and adds up O_p and every product O_p O_q.
//
// Two kernels.  fdg_chain_obs_partial<NP> walks the walkers once: a lane reads every column that some row uses once per walker
// (stride 1 across the lanes), folds it into the rows that use it, and keeps S_p and P_pq of its walkers in registers -- NP slots,
// NP + NP (NP + 1) / 2 accumulators, three instances (5, 9, 17 slots) so that a call with few rows does not pay for 170 of them;
// the instance of 17 splits its pairs by rows over three workgroups (blockIdx.y), each of which reads the columns again.
// The table of the live columns (column, mask of the rows that use it, their factors) is wave-uniform: scalar loads, scalar branches
// on the mask's bits; a factor of zero is selected away, never multiplied.  The workgroup's 256 lane partials go through the LDS
// tree, eight accumulators at a time, into part [V][W].  fdg_chain_obs_final adds the W partials of every output by the scheme of
// fdg_chain_reduce (fdg_chain.hip) and adds the total to d_out.  The order of every sum is a function of n_walker alone: the
// instance, the rows and their factors change which sums are formed, not how.
//
// No kernel here holds a runtime-indexed per-lane array: every index into o[] and acc[] is a constant after unrolling.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#define FDG_RUNTIME_TU 1
#include "fdg_internal.h"

using namespace fdg;

namespace {

constexpr uint32_t OBS_BATCH = 8;                          // accumulators per trip through the LDS tree

constexpr size_t page_up(size_t bytes) { return (bytes + 4095) & ~(size_t)4095; }

// Slot 0 of the kernel is the normalisation (row M of the outputs), slot s >= 1 row s - 1: the live slots are 0 .. M, contiguous
// whatever the instance.  The output index of the pair of slots (sp <= sq), or of the sum of slot sp (pair = false).
__device__ inline uint32_t obs_out_index(uint32_t sp, uint32_t sq, bool pair, uint32_t M) {
  const uint32_t rp = sp ? sp - 1u : M, rq = sq ? sq - 1u : M;
  if (!pair) return rp;
  const uint32_t p = sp ? rp : rq, q = sp ? rq : M;        // (0, s): rows (s - 1, M); (0, 0): (M, M)
  return M + 1u + p * (M + 1u) - p * (p - 1u) / 2u + (q - p);
}

// Accumulator i of the rows P0 .. P1 - 1 of an instance of NP slots: per row p its sum S_p, then its products with the slots q = p
// .. NP - 1.  Constants after unrolling.
struct ObsSlot { int p, q; bool pair; };
constexpr int obs_n_acc(int NP, int P0, int P1) {
  int n = 0;
  for (int p = P0; p < P1; ++p) n += 1 + NP - p;
  return n;
}
constexpr ObsSlot obs_slot(int NP, int P0, int i) {
  int p = P0;
  while (i >= 1 + NP - p) { i -= 1 + NP - p; ++p; }
  return i == 0 ? ObsSlot{p, p, false} : ObsSlot{p, p + i - 1, true};
}

// The walk of one workgroup for the rows P0 .. P1 - 1 of the pairs: every slot's O is formed, the sums of these rows are kept.
template <int NP, int P0, int P1>
__device__ __forceinline__ void obs_walk(const double *__restrict__ sum, long n, const uint32_t *__restrict__ tcol,
                                         const uint32_t *__restrict__ tmask, const double *__restrict__ tcoef, uint32_t n_live, uint32_t M,
                                         uint32_t norm_col, double *__restrict__ part, double (*sh)[256]) {
  constexpr int NA = obs_n_acc(NP, P0, P1);
  const uint32_t t = threadIdx.x, w = blockIdx.x, W = gridDim.x;
  double acc[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) acc[i] = 0.0;
  const double *nrm = sum + (size_t)norm_col * (size_t)n;
  for (long b = 256l * (long)w + (long)t; b < n; b += 256l * (long)W) {
    double o[NP];
    // -0.0 is the identity of IEEE addition for every value, -0.0 and +0.0 included (round to nearest), so a fold begun from it
    // has the bits of the fold that its first product starts
#pragma unroll
    for (int s = 1; s < NP; ++s) o[s] = -0.0;
    for (uint32_t j = 0; j < n_live; ++j) {
      const double a = sum[(size_t)tcol[j] * (size_t)n + (size_t)b];
      const uint32_t mask = tmask[j];
      const double *cf = tcoef + (size_t)j * FDG_CHAIN_OBS_MAX;
#pragma unroll
      for (int s = 1; s < NP; ++s)
        if ((mask >> (s - 1)) & 1u) o[s] = o[s] + cf[s - 1] * a;
    }
    o[0] = nrm[b];
    int at = 0;
#pragma unroll
    for (int p = P0; p < P1; ++p) {
      if ((uint32_t)p <= M) {
        acc[at] = acc[at] + o[p];
#pragma unroll
        for (int q = p; q < NP; ++q) acc[at + 1 + q - p] = acc[at + 1 + q - p] + o[p] * o[q];
      }
      at += 1 + NP - p;
    }
  }
#pragma unroll
  for (int a0 = 0; a0 < NA; a0 += (int)OBS_BATCH) {
#pragma unroll
    for (int k = 0; k < (int)OBS_BATCH; ++k)
      if (a0 + k < NA) sh[k][t] = acc[a0 + k];
    __syncthreads();
    for (uint32_t h = 128; h; h >>= 1) {
      if (t < h) {
#pragma unroll
        for (int k = 0; k < (int)OBS_BATCH; ++k)
          if (a0 + k < NA) sh[k][t] = sh[k][t] + sh[k][t + h];
      }
      __syncthreads();
    }
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < (int)OBS_BATCH; ++k)
        if (a0 + k < NA) {
          constexpr int NPc = NP, P0c = P0;
          const ObsSlot s = obs_slot(NPc, P0c, a0 + k);
          if ((uint32_t)s.q <= M) part[(size_t)obs_out_index((uint32_t)s.p, (uint32_t)s.q, s.pair, M) * (size_t)W + w] = sh[k][0];
        }
    }
    __syncthreads();
  }
}

// The first stage.  NP = 5 and 9 keep every pair in one workgroup; NP = 17 would need 170 accumulators of two registers each, so
// its pairs are split by rows over blockIdx.y into three shares of 51, 54 and 65 accumulators (each share forms every O again).
template <int NP>
__global__ void __launch_bounds__(256)
fdg_chain_obs_partial(const double *__restrict__ sum, long n, const uint32_t *__restrict__ tcol, const uint32_t *__restrict__ tmask,
                      const double *__restrict__ tcoef, uint32_t n_live, uint32_t M, uint32_t norm_col, double *__restrict__ part) {
  __shared__ double sh[OBS_BATCH][256];
  if constexpr (NP == 17) {
    if (blockIdx.y == 0) obs_walk<NP, 0, 3>(sum, n, tcol, tmask, tcoef, n_live, M, norm_col, part, sh);
    else if (blockIdx.y == 1) obs_walk<NP, 3, 7>(sum, n, tcol, tmask, tcoef, n_live, M, norm_col, part, sh);
    else obs_walk<NP, 7, 17>(sum, n, tcol, tmask, tcoef, n_live, M, norm_col, part, sh);
  } else {
    obs_walk<NP, 0, NP>(sum, n, tcol, tmask, tcoef, n_live, M, norm_col, part, sh);
  }
}

// out[v] += the sum of the W workgroup partials of output v, for the outputs whose rows have a term; one workgroup per output.
__global__ void __launch_bounds__(256)
fdg_chain_obs_final(const double *__restrict__ part, uint32_t W, uint32_t M, uint32_t live, double *__restrict__ out) {
  __shared__ double sh[256];
  const uint32_t v = blockIdx.x;
  uint32_t p = v, q = v;
  if (v > M) {
    uint32_t r = v - (M + 1u);
    p = 0;
    while (r >= M + 1u - p) { r -= M + 1u - p; ++p; }
    q = p + r;
  }
  if (!((live >> p) & (live >> q) & 1u)) return;           // a row without a term: its outputs stay as they are
  const double *x = part + (size_t)v * (size_t)W;
  double s = 0.0;
  for (uint32_t w = threadIdx.x; w < W; w += 256) s = s + x[w];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (uint32_t h = 128; h; h >>= 1) {
    if (threadIdx.x < h) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[v] = out[v] + sh[0];
}

uint32_t obs_outputs(uint32_t M) { return (M + 1u) + (M + 1u) * (M + 2u) / 2u; }

bool obs_sizes_ok(uint32_t n_obs, uint32_t n_use) {
  return n_obs >= 1 && n_obs <= FDG_CHAIN_OBS_MAX && n_use >= 1 && n_use <= FDG_CHAIN_OBS_COL_MAX;
}

size_t obs_part_bytes(uint32_t n_obs) { return page_up((size_t)obs_outputs(n_obs) * FDG_CHAIN_OBS_GROUPS * sizeof(double)); }

// the table of the live columns behind the partials: factors [n_use][FDG_CHAIN_OBS_MAX], columns [n_use], masks [n_use]
size_t obs_table_bytes(uint32_t n_use) { return (size_t)n_use * (FDG_CHAIN_OBS_MAX * sizeof(double) + 2u * sizeof(uint32_t)); }

}  // namespace

extern "C" {

size_t fdg_chain_reduce_observables_work_bytes(uint32_t n_obs, uint32_t n_use) {
  if (!obs_sizes_ok(n_obs, n_use)) return 0;
  return obs_part_bytes(n_obs) + page_up(obs_table_bytes(n_use));
}

int fdg_chain_reduce_device_observables(const double *d_sum, int64_t B, uint32_t col_base, uint32_t n_use, uint32_t norm_col,
                                        const double *coef, uint32_t n_obs, double *d_out, void *d_work, void *stream) {
  if (!d_sum || !d_out || !d_work) { set_error("null device buffer"); return FDG_E_INVALID; }
  if (!coef) { set_error("null coef"); return FDG_E_INVALID; }
  if ((const void *)d_out == (const void *)d_sum || (const void *)d_work == (const void *)d_sum || (const void *)d_work == (const void *)d_out) {
    set_error("two of d_sum, d_out and d_work are the same buffer"); return FDG_E_INVALID;
  }
  if (B < 0) { set_error("n_walker < 0"); return FDG_E_INVALID; }
  if (n_obs == 0) { set_error("n_obs == 0"); return FDG_E_INVALID; }
  if (n_use == 0) { set_error("n_use == 0"); return FDG_E_INVALID; }
  if (n_obs > FDG_CHAIN_OBS_MAX) { set_error("n_obs > FDG_CHAIN_OBS_MAX"); return FDG_E_UNSUPPORTED; }
  if (n_use > FDG_CHAIN_OBS_COL_MAX) { set_error("n_use > FDG_CHAIN_OBS_COL_MAX"); return FDG_E_UNSUPPORTED; }
  for (size_t i = 0; i < (size_t)n_obs * n_use; ++i)
    if (!std::isfinite(coef[i])) { set_error("a coefficient is not finite"); return FDG_E_INVALID; }
  if ((uint64_t)norm_col >= (uint64_t)col_base && (uint64_t)norm_col < (uint64_t)col_base + n_use) {
    set_error("norm_col lies inside the window"); return FDG_E_INVALID;
  }
  if (B == 0) return FDG_OK;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t M = n_obs;
  // the columns some row uses, ascending, with the rows that use each and their factors; the rows that have a term
  std::vector<char> tab(obs_table_bytes(n_use), 0);
  double *hcoef = (double *)tab.data();
  uint32_t *hcol = (uint32_t *)(hcoef + (size_t)n_use * FDG_CHAIN_OBS_MAX), *hmask = hcol + n_use;
  uint32_t n_live = 0, live = 1u << M;
  for (uint32_t c = 0; c < n_use; ++c) {
    uint32_t mask = 0;
    for (uint32_t m = 0; m < M; ++m)
      if (coef[(size_t)m * n_use + c] != 0.0) {
        mask |= 1u << m;
        hcoef[(size_t)n_live * FDG_CHAIN_OBS_MAX + m] = coef[(size_t)m * n_use + c];
      }
    if (!mask) continue;
    hcol[n_live] = col_base + c;
    hmask[n_live] = mask;
    live |= mask;
    ++n_live;
  }
  double *part = (double *)d_work;
  char *d_tab = (char *)d_work + obs_part_bytes(n_obs);
  const double *d_coef = (const double *)d_tab;
  const uint32_t *d_col = (const uint32_t *)(d_coef + (size_t)n_use * FDG_CHAIN_OBS_MAX), *d_mask = d_col + n_use;
  // one small upload per call (pageable memory: staged before the call returns)
  if (n_live) HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  const uint32_t W = (uint32_t)std::min<int64_t>(std::max<int64_t>((B + 255) / 256, 1), FDG_CHAIN_OBS_GROUPS);
  const auto partial = M + 1u <= 5u ? fdg_chain_obs_partial<5> : M + 1u <= 9u ? fdg_chain_obs_partial<9> : fdg_chain_obs_partial<17>;
  hipLaunchKernelGGL(partial, dim3(W, M + 1u <= 9u ? 1u : 3u), dim3(256), 0, st, d_sum, (long)B, d_col, d_mask, d_coef, n_live, M, norm_col, part);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(fdg_chain_obs_final, dim3(obs_outputs(M)), dim3(256), 0, st, (const double *)part, W, M, live, d_out);
  HIP_TRY(hipGetLastError());
  return FDG_OK;
}

}  // extern "C"
