// The phase factor of the Matsubara projection (include/fdg.h: fdg_matsubara_phase, fdg_[mc_]accumulate_device_matsubara); one definition
// for host and device, like fdg_sincos.h, so that the projection pass, every checker and a numpy restatement give the same bits.
// No counterpart in the reference checkout: its Monte-Carlo callers form the factor with Julia's exp / sincos (test/ver4.jl:193), which
// are not bit-pinned.
//
// (s, c) = (sin, cos) of omega_n tau, omega_n = (2n+1) pi / beta (fermionic) or 2n pi / beta (bosonic), n of either sign.  Every line
// below is ONE rounded fp64 operation (no FMA: the library is built with -ffp-contract=off), in exactly this order:
//
//   x  = tau / beta
//   m  = x * (double)(fermionic ? 2n+1 : 2n)          (the multiplier is exact: |2n+1| < 2^33)
//   h  = m * 0.5;   fl = floor(h);   r = h - fl        (0 <= r <= 1: r = 1 when h lies just below an integer)
//   th = r * 6.283185307179586                         (0 <= th <= fl(2 pi): inside fdg_sincos' domain, its top end included)
//   (s, c) = fdg_sincos(th)
//
// The passes that project many frequencies of one time pair form x once and the multipliers on the host (matsubara_multiplier): the
// same operations on the same operands, the same bits.
#pragma once
#include <cmath>
#include <cstdint>

#include "fdg_sincos.h"

FDG_SINCOS_HD inline double matsubara_multiplier(int32_t n, int fermionic) {
  const int64_t k = 2 * (int64_t)n + (fermionic ? 1 : 0);
  return (double)k;
}

// (s, c) from x = tau / beta and the multiplier
FDG_SINCOS_HD inline void matsubara_phase_of(double x, double mult, double &s, double &c) {
  const double m = x * mult;
  const double h = m * 0.5;
  const double fl = floor(h);
  const double r = h - fl;
  const double th = r * 6.283185307179586;
  fdg_sincos_impl(th, s, c);
}

FDG_SINCOS_HD inline void fdg_matsubara_phase_impl(double tau, double beta, int32_t n, int fermionic, double &s, double &c) {
  const double x = tau / beta;
  matsubara_phase_of(x, matsubara_multiplier(n, fermionic), s, c);
}
