// sparse.hip — k_nr_sparse: the Newton-Raphson power flow for MESHED nets of any size that fits a CU's LDS, gfx950 (MI355X).
//
// pandapower hands the Jacobian of any net to SuperLU at run time (pypower/newtonpf.py: dx = -spsolve(J, F); reference call
// site voltage_control_env.py:557).  Here the symbolic half of that factorisation is done once per topology on the host
// (plan.cpp: minimum-degree order, fill pattern, one slot per structurally non-zero 2x2 block) and compiled into a PROGRAM
// of block operations  B[c] = inv(B[a]) | B[c] = B[a] B[b] | B[c] -= B[a] B[b]  packed into phases of independent
// operations.  A workgroup is ONE wavefront serving L envs; its 64 lanes are S = 64 / L
// sub-lanes per env (lane = sub * L + env, as in k_nr_tree) and sub-lane s executes operation s of every phase for its L
// envs.  All blocks of those envs (diagonal, off-diagonal incl. fill, right-hand sides as [b | 0] blocks) live in LDS as
// [slot][env][2x2]; a phase is: operation record (prefetched, broadcast buffer load of a constant table) -> six
// ds_read_b128 -> 8 FMAs (+ the 2x2 inverse) -> two ds_write_b128.  One wavefront needs no barrier: LDS executes its
// instructions in order, so the reads of phase p+1 see the writes of phase p.
// sparse_prog.hpp owns that frame (SpWave), the prefetched block assembly (sp_assemble) and the interpreter (sp_run_program), shared
// with k_action_grad_sparse and k_opf_sens_sparse; this file holds what the power flow stores per entry and per row, and the Newton loop.
//
// Same Newton iteration as the other two solvers (flat start, scaled polar unknowns [dtheta, d|V|/|V|], full Jacobian every
// iteration, ||F||inf < tol, <= max_it iterations, V <- V (1 - z1) e^{-j z0}) and the same fused epilogue (nr_common.hpp).
// Voltage-dependent loads (d.zip, a run-time branch here): the mismatch after iteration 0 is formed against Sbus_k (cp + ci |V_k| +
// cz |V_k|^2), the Jacobian stays the constant-power one (pandapower 2.x newtonpf, as k_nr_tree).
// Radial feeders keep the specialised tree kernel; MAPDN_NR_SPARSE=1 runs this one on them too (cross-check).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gen_mask.hpp"
#include "kernels.hpp"
#include "nr_common.hpp"
#include "sparse_prog.hpp"

namespace mapdn {

// Generators (d.gen_start, a run-time branch like ZIP): every node starts at its own magnitude d.v0; at block assembly the Q row of every
// block in a gen node's block row and the |V| column of every block in its block column are zeroed, its diagonal block's (2, 2) is 1 and
// the Q entry of its right-hand side 0 (gen_mask.hpp) — the program is untouched, fill blocks inherit the zeros; the verdict skips its Fq.
// DC: runpp init="dc" (mapdn_env_config.nr_init = 2) — before the first iteration the same program solves Bbus theta = Pbus per env
// (the DC power flow of pandapower run_dc_pf) and the solve starts from V0 = vroot e^{j theta}; DC = false: the flat start.
template <int L, bool DC = false>
__global__ void __launch_bounds__(64)
k_nr_sparse(Dev d, int mode, double* __restrict__ reward, uint8_t* __restrict__ terminated, double* __restrict__ info) {
  extern __shared__ d2 lds2[];
  constexpr unsigned S = 64u / L;
  const SpWave<L> w(d, lds2);
  const unsigned s = w.s, e = w.e;
  const int n = d.n;
  const double vroot = d.vroot, tol = d.tol;
  d2* sV = w.sV;
  double* s_epi = (double*)(lds2 + (size_t)(n + 2) * L + (size_t)d.sp_blocks * 2u * L) + w.el;  // 10 * S * L doubles (epilogue), also the verdict scratch
  const bool gens = d.gen_start != 0;            // generators (run-time branch, wave-uniform): per-node start magnitudes, masked gen blocks
  auto v0_of = [&](unsigned k) { return gens ? d.v0[k] : vroot; };
  auto gen_at = [&](unsigned k) { return gens && d.is_gen[k] != 0; };
  for (unsigned k = s; k < (unsigned)n + 2u; k += S) sV[(size_t)k * L] = d2{v0_of(k), 0.0};     // runpp init="auto": flat start
  const bool act = d.active[e] != 0;
  const int bk_steps = d.steps[e];
  const uint32_t bk_draw = d.draw[e];
  const double bk_sum = d.sum_rewards[e];
  const auto nz = sp_stream(d.sp_nz, d.sp_nz_bytes, d.sp_rows_per_sub, d.sp_max_nnz);          // the Ybus entries of the assembly rows
  const int RPS = d.sp_rows_per_sub;
  const double2* gsb = (const double2*)((const char*)d.nrbuf + d.sb_off);
  const bool nothing_to_solve = __all(!act);
  bool done = !act, conv = false;
  int it = 0;
  if constexpr (DC) {
    // ---- DC-angle start (oracle/pp_restated.py dc_angles): blocks [[B_ij, 0], [0, 0]] off the diagonal, [[B_ii, 0], [0, 1]] on it and
    // the right-hand side [Pbus_i | 0], Pbus = Re(Sbus) + dc_pc; the program's solution is [theta_i, 0]
    if (!nothing_to_solve) {
      sp_zero_fill(w, d);
      const int MNZ = d.sp_max_nnz;
      for (int r = 0; r < RPS; ++r) {
        const unsigned i = (unsigned)r * S + s;
        if (i >= (unsigned)n) continue;
        const SpNz* z = d.sp_nz + ((size_t)s * RPS + r) * MNZ;
        double bii = 0.0;
        for (int q = 0; q < MNZ; ++q) {
          const SpNz zq = z[q];
          if ((zq.col & ~SP_COL_GEN) == i) bii = zq.bdc;
          else if (zq.slot >= 0) { d2* o = w.blk((unsigned)zq.slot); o[0] = d2{zq.bdc, 0.0}; o[1] = d2{0.0, 0.0}; }
        }
        d2* dg = w.blk(i);
        dg[0] = d2{bii, 0.0}; dg[1] = d2{0.0, 1.0};
        d2* rh = w.blk((unsigned)n + i);
        rh[0] = d2{gsb[(size_t)i * d.Bp + e].x + d.dc_pc[i], 0.0}; rh[1] = d2{0.0, 0.0};
      }
      sp_run_program(w, done);
      for (int r = 0; r < RPS; ++r) {
        const unsigned i = (unsigned)r * S + s;
        if (i < (unsigned)n && !done) {
          double sn, cs;
          sincos(w.blk((unsigned)n + i)[0].x, &sn, &cs);
          const double v0 = v0_of(i);
          sV[(size_t)i * L] = d2{v0 * cs, v0 * sn};
        }
      }
    }
  }
  while (!nothing_to_solve) {
    // ---- mismatch F = V conj(Ybus V) - Sbus and the Jacobian blocks, row by row (sub-lane s owns rows s, s + S, ...):
    //      dS_i/dtheta_j = -j A_ij, dS_i/dln|V_j| = A_ij (j != i); dS_i/dtheta_i = j (S_i - A_ii), dS_i/dln|V_i| = S_i + A_ii
    sp_zero_fill(w, d);
    bool ok = true;
    double2 sb;                                  // this row's Sbus entry
    bool gi;                                     // this row's node is a gen bus
    sp_assemble(
        w, nz,
        [&](unsigned i, bool live) { sb = gsb[(size_t)(live ? i : 0u) * d.Bp + e]; gi = live && gen_at(i); },
        [&](const SpRec<sizeof(SpNz)>& z, unsigned slot, d2, d2, double ar, double ai) {
          const Opf2x2 m = gs_offdiag(ar, ai);
          d2* o = w.blk(slot);
          if (gens) {                            // gen buses (gen_mask.hpp): no Q row in the block row of one, no |V| column in its block column
            const bool gj = (z.a.x & SP_COL_GEN) != 0;       // (rides in the prefetched record)
            o[0] = d2{m.m00, gj ? 0.0 : m.m01}; o[1] = gi ? d2{0.0, 0.0} : d2{m.m10, gj ? 0.0 : m.m11};
          } else { o[0] = d2{m.m00, m.m01}; o[1] = d2{m.m10, m.m11}; }
        },
        [&](unsigned i, bool live, d2 vi, double sr, double si, double aii_r, double aii_i) {   // diagonal block, right-hand side, verdict
          double sbr = sb.x, sbi = sb.y;
          if (d.zip && it > 0) {                 // voltage-dependent loads: makeSbus(vm = |V|) after the first voltage update (as k_nr_tree)
            const double2 zc = ((const double2*)d.zip_c)[live ? i : (unsigned)n + 1u];
            const double v2 = vi.x * vi.x + vi.y * vi.y;
            const double vd = fma(zc.y, v2, fma(zc.x, sqrt(v2), 1.0 - (zc.x + zc.y)));
            sbr *= vd; sbi *= vd;
          }
          const double Fp = sr - sbr, Fq = gen_mask_fq(gi, si - sbi);
          if (live) {
            Opf2x2 m = gs_diag(sr, si, aii_r, aii_i);
            double r1 = Fq;
            gen_mask_pivot(gi, m.m01, m.m10, m.m11, r1);
            d2* dg = w.blk(i);
            dg[0] = d2{m.m00, m.m01}; dg[1] = d2{m.m10, m.m11};
            d2* rh = w.blk((unsigned)n + i);
            rh[0] = d2{Fp, 0.0}; rh[1] = d2{r1, 0.0};
            ok = ok && (fabs(Fp) < tol) && (fabs(Fq) < tol);
          }
        });
    {                                                              // AND over the sub-lanes of an env
      s_epi[(size_t)s * L] = ok ? 1.0 : 0.0;
      bool all = true;
#pragma unroll 4
      for (unsigned t = 0; t < S; ++t) all = all && (s_epi[(size_t)t * L] != 0.0);
      ok = all;
    }
    if (!done) {
      conv = ok;
      if (conv || it == d.max_it) done = true;
    }
    if (__all(done)) break;
    sp_run_program(w, done);                     // numeric factorisation + forward / backward substitution; a finished env takes no writes
    // ---- newtonpf update: Va -= z0, Vm -= |V| z1, V = Vm e^{jVa}   =>   V <- V (1 - z1) e^{-j z0}
    for (int r = 0; r < RPS; ++r) {
      const unsigned i = (unsigned)r * S + s;
      if (i < (unsigned)n && !done) {
        const d2* x = w.blk((unsigned)n + i);
        const double y0 = x[0].x, y1 = x[1].x;
        const d2 vi = sV[(size_t)i * L];
        double sn, cs;
        sincos(-y0, &sn, &cs);
        sV[(size_t)i * L] = nr_rotate(vi, sn, cs, y1);
      }
    }
    if (!done) ++it;
  }
  if (s == 0) { d.iters[e] = it; d.conv[e] = conv ? 1 : 0; }
  nr_epilogue<(unsigned)L, S>(d, mode, reward, terminated, info, sV, s, e, act, conv, bk_steps, bk_draw, bk_sum, s_epi,
                              (const double*)nullptr, [](int) {});
}

size_t nr_sparse_lds_bytes(int n, int n_blocks, int L) {
  return ((size_t)(n + 2) * L + (size_t)n_blocks * 2 * L) * 16 + (size_t)10 * 64 * sizeof(double);
}

int nr_sparse_prepare(int L) {
  const int rc = sp_prepare(L, [](auto l) { return k_nr_sparse<decltype(l)::value, false>; });
  return rc ? rc : sp_prepare(L, [](auto l) { return k_nr_sparse<decltype(l)::value, true>; });
}

void launch_nr_sparse(const Dev& d, int mode, double* reward, uint8_t* term, double* info, hipStream_t st) {
  if (d.nr_init == 2) sp_launch(d, d.Bp, st, [](auto l) { return k_nr_sparse<decltype(l)::value, true>; }, d, mode, reward, term, info);
  else sp_launch(d, d.Bp, st, [](auto l) { return k_nr_sparse<decltype(l)::value, false>; }, d, mode, reward, term, info);
}

}  // namespace mapdn
