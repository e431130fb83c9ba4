// branch.hpp — the arithmetic of res_line / res_trafo, compilable for the HOST as well: tests/branch_check.cpp builds this
// header with g++ and runs it against the extended-precision reference (tests/test_branch_cpu.py).  The kernels of branch.hip call the
// same function per (env, branch).
//
// pandapower 2.7.0 results_branch.py::_get_line_results / _get_trafo_results (trafo_loading="current"), restated [PP-recalled]: with the pi
// constants of makeYbus (plan.cpp: yff, yft, ytf, ytt) and the bus voltages Vf, Vt in per unit
//     Sf = Vf conj(yff Vf + yft Vt),   St = Vt conj(ytf Vf + ytt Vt)
//     p_from_mw + j q_from_mvar = Sf sn_mva,   p_to_mw + j q_to_mvar = St sn_mva
//     pl_mw   = sn_mva [ gff |Vf|^2 + gtt |Vt|^2 + (gft + gtf) a + (bft - btf) b ],   a + jb = Vf conj(Vt)      (plan.hpp LineFlow: Re(Sf + St))
//     ql_mvar = sn_mva [-bff |Vf|^2 - btt |Vt|^2 - (bft + btf) a + (gft - gtf) b ]                                (Im(Sf + St))
//       (not formed as p_from + p_to; the four terms are regrouped around |Vf - Vt|^2, see branch_eval)
//     i_from_ka = |Sf| sn_mva / (sqrt(3) |Vf| bus_vn_kv[from]),  i_to_ka likewise,  i_ka = max of the two;  |S| == 0 gives 0
//     line:  loading_percent = 100 i_ka / (max_i_ka df parallel)
//     trafo: loading_percent = 100 sqrt(3) max(i_hv_ka vn_hv_kv, i_lv_ka vn_lv_kv) / (sn_mva_trafo parallel df)
// An out-of-service line reports 0 in every column; an unrated branch (no rating given) reports loading_percent = NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define BR_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define BR_FN static inline
#endif

namespace mapdn {

// One branch of either table, shared by all envs (wave-uniform reads): 128 bytes.
struct BranchRec {
  int32_t f, t;          // ORIGINAL bus ids (rows of res_bus): fused buses share their representative's voltage there
  int32_t live, trafo;   // in service; 0 = net.line row, 1 = per-unit pi branch (from = hv, to = lv)
  double y[8];           // gff bff | gft bft | gtf btf | gtt btt
  double vn_f, vn_t;     // bus_vn_kv of the two ends
  double rate;           // line: max_i_ka df parallel (kA); trafo: sn_mva parallel df (MVA); NaN = unrated
  double tv_f, tv_t;     // trafo: nameplate vn_hv_kv, vn_lv_kv (an unrated trafo has rate = NaN and 1 here)
  double parallel;       // line: net.line.parallel (folded into rate by mapdn_set_branch_ratings); trafo: 1 (its rating arrives folded)
};
static_assert(sizeof(BranchRec) == 128, "BranchRec must be 128 bytes");

// columns of mapdn_branch_out, in its order
enum { BC_PF = 0, BC_QF, BC_PT, BC_QT, BC_PL, BC_QL, BC_IF, BC_IT, BC_I, BC_LOAD, BC_N };
enum : uint32_t { BM_FLOW = (1u << BC_PF) | (1u << BC_QF) | (1u << BC_PT) | (1u << BC_QT) | (1u << BC_IF) | (1u << BC_IT) | (1u << BC_I) | (1u << BC_LOAD),
                  BM_LOSS = (1u << BC_PL) | (1u << BC_QL) };

#define BR_SQRT3 1.7320508075688772

// p, q in MW / MVAr, vm in per unit, vn in kV -> kA
BR_FN double br_current(double p, double q, double vm, double vn) {
  const double s = sqrt(p * p + q * q);
  return s == 0.0 ? 0.0 : s / (BR_SQRT3 * vm * vn);
}

// every column of one branch at |V| / angle (rad) of its two ends; `want` (BM_*) skips the flows or the losses when no column of the
// group is asked for (the skipped columns are left unset)
BR_FN void branch_eval(const BranchRec& r, double vmf, double vaf, double vmt, double vat, double sn, uint32_t want, double (&o)[BC_N]) {
  if (!r.live) {
    o[BC_PF] = o[BC_QF] = o[BC_PT] = o[BC_QT] = o[BC_PL] = o[BC_QL] = o[BC_IF] = o[BC_IT] = o[BC_I] = o[BC_LOAD] = 0.0;
    return;
  }
  const double ef = vmf * cos(vaf), ff = vmf * sin(vaf), et = vmt * cos(vat), ft = vmt * sin(vat);
  if (want & BM_FLOW) {
    const double ifr = r.y[0] * ef - r.y[1] * ff + r.y[2] * et - r.y[3] * ft;      // If = yff Vf + yft Vt
    const double ifi = r.y[0] * ff + r.y[1] * ef + r.y[2] * ft + r.y[3] * et;
    const double itr = r.y[4] * ef - r.y[5] * ff + r.y[6] * et - r.y[7] * ft;      // It = ytf Vf + ytt Vt
    const double iti = r.y[4] * ff + r.y[5] * ef + r.y[6] * ft + r.y[7] * et;
    o[BC_PF] = (ef * ifr + ff * ifi) * sn; o[BC_QF] = (ff * ifr - ef * ifi) * sn;  // S = V conj(I)
    o[BC_PT] = (et * itr + ft * iti) * sn; o[BC_QT] = (ft * itr - et * iti) * sn;
    o[BC_IF] = br_current(o[BC_PF], o[BC_QF], vmf, r.vn_f);
    o[BC_IT] = br_current(o[BC_PT], o[BC_QT], vmt, r.vn_t);
    o[BC_I] = o[BC_IF] > o[BC_IT] ? o[BC_IF] : o[BC_IT];
    if (r.trafo) {
      const double sf = o[BC_IF] * r.tv_f, st = o[BC_IT] * r.tv_t;
      o[BC_LOAD] = 100.0 * BR_SQRT3 * (sf > st ? sf : st) / r.rate;
    } else {
      o[BC_LOAD] = 100.0 * o[BC_I] / r.rate;
    }
  }
  if (want & BM_LOSS) {
    // The four terms, regrouped so that they do not cancel in floating point: a = (|Vf|^2 + |Vt|^2 - d) / 2 with d = |Vf - Vt|^2 formed
    // from the component differences, hence  gff |Vf|^2 + gtt |Vt|^2 + (gft + gtf) a = (gff + gs) |Vf|^2 + (gtt + gs) |Vt|^2 - gs d,
    // gs = (gft + gtf) / 2.  On a line gs = -g of the series admittance (some 10^2 p.u.) and gff + gs, gtt + gs are the shunt
    // conductance alone — exactly 0 without g_us_per_km — so the loss is g |Vf - Vt|^2 to its last digits, where the plain sum of four
    // terms of size g leaves 10^-16 g of rounding on a loss of 10^-4.  The same for Q with bs = (bft + btf) / 2.
    const double vf2 = ef * ef + ff * ff, vt2 = et * et + ft * ft, b = ff * et - ef * ft;      // b = Im(Vf conj(Vt))
    const double de = ef - et, df = ff - ft, d = de * de + df * df;
    const double gs = 0.5 * (r.y[2] + r.y[4]), bs = 0.5 * (r.y[3] + r.y[5]);
    o[BC_PL] = ((r.y[0] + gs) * vf2 + (r.y[6] + gs) * vt2 - gs * d + (r.y[3] - r.y[5]) * b) * sn;
    o[BC_QL] = (bs * d - (r.y[1] + bs) * vf2 - (r.y[7] + bs) * vt2 + (r.y[2] - r.y[4]) * b) * sn;
  }
}

}  // namespace mapdn
