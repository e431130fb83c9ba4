// droop.hpp — the Volt/VAR droop law of the reference's traditional controller (traditional_control/pf_droop_matpower_all.m:196-231)
// and the pieces of its fixed-point loop, compilable for the HOST as well: tests/test_droop_cpu.py builds this header with g++ and
// compares it bit for bit with the numpy restatement (tests/droop_ref.py).  No expression here may be contracted into a fused
// multiply-add (numpy rounds every product), hence the pragma.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define DROOP_FN __host__ __device__ __forceinline__
#else
#define DROOP_FN static inline
#endif

namespace mapdn {

// f(v) with the branches tested in the script's order: v <= va -> +1, v > vd -> -1, vb <= v <= vc -> 0, v < vb -> the rising
// slope, otherwise the falling one (va < vb <= vc < vd)
DROOP_FN double droop_law(double v, double va, double vb, double vc, double vd) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (v <= va) return 1.0;
  if (v > vd) return -1.0;
  if (vb <= v && v <= vc) return 0.0;
  if (v < vb) return (v - vb) / (va - vb);
  return -(v - vc) / (vd - vc);
}

// the action the law asks for, in units of lim = sqrt(s_max^2 - p^2): the script's q_max = min(lim, ratio s_max), so f is scaled by
// min(1, ratio s_max / lim) (exactly 1 with ratio = 1)
DROOP_FN double droop_target(double f, double ratio, double smax, double lim) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return f * fmin(1.0, ratio * smax / lim);
}

// the damped update a <- (1 - damping) a + damping target
DROOP_FN double droop_damped(double a, double target, double damping) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  return (1.0 - damping) * a + damping * target;
}

// ||v - v_last||_2^2 summed in sgen order: s + (v - v_last)^2, the square rounded on its own (droop_dv2_sum adds a squared term)
DROOP_FN double droop_dv2_sum(double s, double dv2) {
  return s + dv2;
}
DROOP_FN double droop_dv2_add(double s, double v, double v_last) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double dv = v - v_last;
  return droop_dv2_sum(s, dv * dv);
}

}  // namespace mapdn
