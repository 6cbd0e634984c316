// Sine and cosine for the polar variables of the VEGAS sampler (include/fdg.h: fdg_vegas_sample_device_polar, fdg_sincos); one
// definition for host and device so that the sampler, every checker and a numpy restatement run the same operations on the same
// constants and give the same bits.  The device library's sin / cos and the host libm's differ in the last place; this does not.
// No counterpart in the reference (its MCIntegration.FermiK calls Julia's sin / cos, which are not bit-pinned across versions either).
//
// Domain: 0 <= x <= 2 pi, the double nearest above 2 pi included.  Every line below is ONE rounded fp64 operation (no FMA: the
// library is built with -ffp-contract=off), in exactly this order:
//
//   reduce (Cody-Waite, pi/2 = P1 + P1T: P1 holds the first 33 bits, so q * P1 is exact for q <= 4 and x - q * P1 is exact too)
//     fn = x * TWO_OVER_PI;  fn = fn + 0.5;  q = (int)fn  (truncation; 0 <= q <= 4)
//     r  = x - q * P1;       t  = q * P1T;   r = r - t                              (|r| <= pi/4 up to rounding of fn)
//   two Horner polynomials in z = r * r (plain Taylor coefficients, each the double nearest to (-1)^n / (2n+1)! or (-1)^n / (2n)!)
//     ps = S8;  ps = ps * z;  ps = ps + S7;  ...  ps = ps * z;  ps = ps + S1
//     sn = r * z;  sn = sn * ps;  sn = r + sn                                       (r - r^3/3! + ... + r^17/17!)
//     pc = C8;  pc = pc * z;  pc = pc + C7;  ...  pc = pc * z;  pc = pc + C2
//     h  = 0.5 * z;  w = z * z;  w = w * pc;  h = h - w;  cs = 1.0 - h              (1 - r^2/2! + ... + r^16/16!)
//   quadrant by select, never by multiplying with 0 or +-1 (q & 3:  0 -> (sn, cs), 1 -> (cs, -sn), 2 -> (-sn, -cs), 3 -> (-cs, sn))
//     s = (q & 1) ? cs : sn;  if ((q & 2) != 0) s = -s
//     c = (q & 1) ? sn : cs;  if (((q + 1) & 2) != 0) c = -c
//
// Constants (decimal literals that round-trip; hex in brackets):
//   TWO_OVER_PI = 0.6366197723675814      [0x1.45f306dc9c883p-1]
//   P1  = 1.5707963267341256              [0x1.921fb544p+0]       P1T = 6.077100506506192e-11  [0x1.0b4611a626331p-34]
//   S1 .. S8 = -0.16666666666666666, 0.008333333333333333, -0.0001984126984126984, 2.7557319223985893e-06, -2.505210838544172e-08,
//              1.6059043836821613e-10, -7.647163731819816e-13, 2.8114572543455206e-15
//   C2 .. C8 = 0.041666666666666664, -0.001388888888888889, 2.48015873015873e-05, -2.755731922398589e-07, 2.08767569878681e-09,
//              -1.1470745597729725e-11, 4.779477332387385e-14
//
// Properties (tests/test_vegas_polar_host.py; DESIGN.md 8d has the measured error):
//  * |s - sin x|, |c - cos x| <= 4 * 2^-53 absolute: r is off by one rounding (the last subtraction, at most 2^-54) plus P1 + P1T - pi/2
//    (below 1e-26); each polynomial ends in one addition of a result below 1 (at most 2^-54) and the terms before it add a few 2^-57.
//  * s >= 0 on [0, fl(pi)]: q = 0 gives sn of r = x >= 0, q = 1 gives cs >= 0.7, and in q = 2 the reduction is exact up to the one
//    monotone rounding, r(fl(pi)) = fl(pi) - 2 (P1 + P1T) = -1.22e-16 < 0, so r <= 0 and s = -sn >= 0 (sn has the sign of r).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define FDG_SINCOS_HD __host__ __device__
#else
#define FDG_SINCOS_HD
#endif

FDG_SINCOS_HD inline void fdg_sincos_impl(double x, double &s, double &c) {
  double fn = x * 0.6366197723675814;
  fn = fn + 0.5;
  const int q = (int)fn;
  const double qd = (double)q;
  double r = x - qd * 1.5707963267341256;
  const double t = qd * 6.077100506506192e-11;
  r = r - t;
  const double z = r * r;
  double ps = 2.8114572543455206e-15;
  ps = ps * z; ps = ps + -7.647163731819816e-13;
  ps = ps * z; ps = ps + 1.6059043836821613e-10;
  ps = ps * z; ps = ps + -2.505210838544172e-08;
  ps = ps * z; ps = ps + 2.7557319223985893e-06;
  ps = ps * z; ps = ps + -0.0001984126984126984;
  ps = ps * z; ps = ps + 0.008333333333333333;
  ps = ps * z; ps = ps + -0.16666666666666666;
  double sn = r * z;
  sn = sn * ps;
  sn = r + sn;
  double pc = 4.779477332387385e-14;
  pc = pc * z; pc = pc + -1.1470745597729725e-11;
  pc = pc * z; pc = pc + 2.08767569878681e-09;
  pc = pc * z; pc = pc + -2.755731922398589e-07;
  pc = pc * z; pc = pc + 2.48015873015873e-05;
  pc = pc * z; pc = pc + -0.001388888888888889;
  pc = pc * z; pc = pc + 0.041666666666666664;
  double h = 0.5 * z;
  double w = z * z;
  w = w * pc;
  h = h - w;
  const double cs = 1.0 - h;
  double sv = (q & 1) ? cs : sn;
  double cv = (q & 1) ? sn : cs;
  if ((q & 2) != 0) sv = -sv;
  if (((q + 1) & 2) != 0) cv = -cv;
  s = sv;
  c = cv;
}
