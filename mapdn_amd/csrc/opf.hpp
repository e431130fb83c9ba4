// opf.hpp — the arithmetic of the OPF baseline (reduced-space SQP), compilable for the HOST as well: tests/opf_check.cpp
// builds this header with g++ and runs the tree elimination against a dense solve and the QP routine against stored optima
// (tests/test_opf_cpu.py).  The kernels of opf.hip call the same functions on env-minor global memory (OpfVec with stride Bp).
//
// Linearisation at a converged power flow.  Unknowns per node k: x_k = (dtheta_k, u_k), u = d|V| / |V|.  With T_km = V_k conj(Y_km V_m)
// = a + jb the polar Jacobian has the 2x2 blocks
//     J_km = [[ b, a], [-a, b]]  (m != k),     J_kk = [[-(Q_k - Im T_kk), P_k + Re T_kk], [P_k - Re T_kk, Q_k + Im T_kk]],
// S_k = P_k + jQ_k = sum_m T_km.  On the radial plan (children before parents) the block LU has no fill:
//     forward   D_k = J_kk - sum_children C_c,   L_k = J_pk D_k^-1,   C_k = L_k J_kp,   r_p -= L_k r_k
//     backward  x_k = D_k^-1 (r_k - J_kp x_p)
// The right-hand side of column j is w_j e_Q at the node of sgen j, so its forward pass is the path from that node to its root.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define OPF_FN __host__ __device__ inline
#define OPF_MEM __host__ __device__
#else
#define OPF_FN static inline
#define OPF_MEM
#endif

namespace mapdn {

// element i of a per-env array lives at p[i * s]: s = Bp on the device (env-minor), 1 on the host
struct OpfVec {
  double* p; size_t s;
  OPF_MEM double& operator[](size_t i) const { return p[i * s]; }
};

// per-node constants (shared by all envs), OPF_YT doubles each: Y_kk, Y_k,parent, Y_parent,k, Y_k,slack V_slack (Plan::yc), then the
// Hermitian part M = (Y + Y^H) / 2 of Ybus that the loss V^H M V sees: M_k,parent and M_k,slack V_slack
enum { OY_KK = 0, OY_KP = 2, OY_PK = 4, OY_KS = 6, OY_MKP = 8, OY_MSV = 10, OPF_YT = 12 };
// per-node factors of one env, OPF_FAC doubles each
enum { OF_DINV = 0, OF_L = 4, OF_JKP = 8, OF_C = 12, OPF_FAC = 16 };

struct Opf2x2 { double m00, m01, m10, m11; };

OPF_FN Opf2x2 opf_mul(const Opf2x2& a, const Opf2x2& b) {
  return {a.m00 * b.m00 + a.m01 * b.m10, a.m00 * b.m01 + a.m01 * b.m11, a.m10 * b.m00 + a.m11 * b.m10, a.m10 * b.m01 + a.m11 * b.m11};
}
OPF_FN Opf2x2 opf_inv(const Opf2x2& a) {
  const double id = 1.0 / (a.m00 * a.m11 - a.m01 * a.m10);
  return {a.m11 * id, -a.m01 * id, -a.m10 * id, a.m00 * id};
}
// the off-diagonal block of T = V_k conj(Y_km V_m)
OPF_FN Opf2x2 opf_offdiag(double ek, double fk, double yr, double yi, double em, double fm, double* tr, double* ti) {
  const double cr = yr * em - yi * fm, ci = yr * fm + yi * em;       // Y_km V_m
  const double a = ek * cr + fk * ci, b = fk * cr - ek * ci;         // V_k conj(.)
  *tr = a; *ti = b;
  return {b, a, -a, b};
}
OPF_FN Opf2x2 opf_diag(double P, double Q, double tkk_r, double tkk_i) {
  return {-(Q - tkk_i), P + tkk_r, P - tkk_r, Q + tkk_i};
}
OPF_FN void opf_load4(const OpfVec& f, size_t o, Opf2x2* m) { m->m00 = f[o]; m->m01 = f[o + 1]; m->m10 = f[o + 2]; m->m11 = f[o + 3]; }
OPF_FN void opf_store4(const OpfVec& f, size_t o, const Opf2x2& m) { f[o] = m.m00; f[o + 1] = m.m01; f[o + 2] = m.m10; f[o + 3] = m.m11; }

// The elimination step of node k (leaf -> root): D = J_kk - sum of the children's C (canonical child order), its inverse, L_k, J_kp and
// C_k into fac.  e, f: Re / Im V by node position (the slack is not read: its terms are the constants OY_KS).  Returns S_k in *P, *Q.
OPF_FN void opf_elim_step(int k, int n, const int32_t* par, const int32_t* cptr, const int32_t* cidx, const double* yt, const OpfVec& e,
                          const OpfVec& f, const OpfVec& fac, double* P, double* Q) {
  const double* y = yt + (size_t)k * OPF_YT;
  const double ek = e[k], fk = f[k];
  const double m2 = ek * ek + fk * fk;
  const double tkr = y[OY_KK] * m2, tki = -y[OY_KK + 1] * m2;       // T_kk = conj(Y_kk) |V_k|^2
  double sr = tkr + (ek * y[OY_KS] + fk * y[OY_KS + 1]), si = tki + (fk * y[OY_KS] - ek * y[OY_KS + 1]);   // + V_k conj(Y_ks V_s)
  const int p = par[k];
  Opf2x2 jkp = {0, 0, 0, 0}, jpk = {0, 0, 0, 0};
  double tr, ti;
  if (p < n) {
    jkp = opf_offdiag(ek, fk, y[OY_KP], y[OY_KP + 1], e[p], f[p], &tr, &ti);
    sr += tr; si += ti;
    jpk = opf_offdiag(e[p], f[p], y[OY_PK], y[OY_PK + 1], ek, fk, &tr, &ti);
  }
  double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0;
  for (int i = cptr[k]; i < cptr[k + 1]; ++i) {
    const int c = cidx[i];
    const double* yc = yt + (size_t)c * OPF_YT;
    (void)opf_offdiag(ek, fk, yc[OY_PK], yc[OY_PK + 1], e[c], f[c], &tr, &ti);     // Y_kc = Y_parent,child of c
    sr += tr; si += ti;
    Opf2x2 C; opf_load4(fac, (size_t)c * OPF_FAC + OF_C, &C);
    c00 += C.m00; c01 += C.m01; c10 += C.m10; c11 += C.m11;
  }
  Opf2x2 D = opf_diag(sr, si, tkr, tki);
  D.m00 -= c00; D.m01 -= c01; D.m10 -= c10; D.m11 -= c11;
  const Opf2x2 Di = opf_inv(D);
  const Opf2x2 L = opf_mul(jpk, Di);
  const size_t o = (size_t)k * OPF_FAC;
  opf_store4(fac, o + OF_DINV, Di); opf_store4(fac, o + OF_L, L); opf_store4(fac, o + OF_JKP, jkp); opf_store4(fac, o + OF_C, opf_mul(L, jkp));
  *P = sr; *Q = si;
}

// One column of J X = E: the right-hand side w e_Q at node kj (kj >= n: the slack, a zero column).  x holds 2 values per node at
// x[(k * xs + c)]: (dtheta, u).  The forward pass walks the path kj -> root (r_p = -L_k r_k: every other r is 0); the
// back-substitution step is x_k = D_k^-1 (r_k - J_kp x_p).
OPF_FN void opf_back_step(int k, int p, int n, const OpfVec& fac, const OpfVec& x, size_t xs) {
  double r0 = x[(size_t)k * xs], r1 = x[(size_t)k * xs + 1];
  const size_t o = (size_t)k * OPF_FAC;
  if (p < n) {
    Opf2x2 J; opf_load4(fac, o + OF_JKP, &J);
    const double x0 = x[(size_t)p * xs], x1 = x[(size_t)p * xs + 1];
    r0 -= J.m00 * x0 + J.m01 * x1; r1 -= J.m10 * x0 + J.m11 * x1;
  }
  Opf2x2 Di; opf_load4(fac, o + OF_DINV, &Di);
  x[(size_t)k * xs] = Di.m00 * r0 + Di.m01 * r1; x[(size_t)k * xs + 1] = Di.m10 * r0 + Di.m11 * r1;
}
OPF_FN void opf_solve_column(int kj, double w, int n, const int32_t* par, const OpfVec& fac, const OpfVec& x, size_t xs) {
  for (int k = 0; k < n; ++k) { x[(size_t)k * xs] = 0.0; x[(size_t)k * xs + 1] = 0.0; }
  if (kj >= n) return;
  double r0 = 0.0, r1 = w;
  for (int k = kj;;) {
    x[(size_t)k * xs] = r0; x[(size_t)k * xs + 1] = r1;
    const int p = par[k];
    if (p >= n) break;
    Opf2x2 L; opf_load4(fac, (size_t)k * OPF_FAC + OF_L, &L);
    const double t0 = -(L.m00 * r0 + L.m01 * r1), t1 = -(L.m10 * r0 + L.m11 * r1);
    r0 = t0; r1 = t1; k = p;
  }
  for (int k = n - 1; k >= 0; --k) opf_back_step(k, par[k], n, fac, x, xs);
}

// ---- the QP of one SQP iteration:  min g'd + d'Hd / 2  s.t.  lo_r <= (A d)_r <= hi_r,  A = [I; S]: the box rows -1 - a <= d <= 1 - a
// first, then one row per node, vl - v <= S d <= vu - v.  Augmented Lagrangian on every row with a semismooth Newton inner solve:
//     phi(d) = g'd + d'Hd / 2 + sum_r (z_r^2 - y_r^2) / (2 rho_r),   z_r = the AL multiplier of row r at c_r = (A d)_r
//     Newton: (H + sum over z_r != 0 of rho_r a_r a_r' + ridge) p = -grad phi  (Cholesky), backtracking on phi;  then y <- z.
// rho_r = OPF_QP_RHO max(H_ii) / |a_r|^2 (a stiffer penalty would put its rounding, rho_r ulp(c_r), into the stationarity).  Rows that
// share (nearly) one normal — two buses with the same sensitivity row — keep multipliers that decay by only rho x slack per outer
// iteration, so when an outer iteration fails to quarter the violation, the multiplier of every row strictly inside its bound is
// dropped (the AL rebuilds it if it is needed).  y may come in warm: the multipliers of the previous SQP iteration's QP.
// It stops on the KKT residual of the QP — stationarity <= eps |g|inf, violation <= eps, complementarity <= eps |g|inf — or reports
// that it hit its cap: OPF_QP_MAX_OUTER outer iterations, or OPF_QP_MAX_STALL in a row that did not halve the violation (an infeasible QP).  Needs S d, S' z, H d and rank-one updates with the rows of S only.
#define OPF_QP_RHO 1e4
#define OPF_QP_EPS 1e-10
#define OPF_QP_RIDGE 1e-8
#define OPF_QP_SHRINK 0.25
#define OPF_QP_STALL 0.5
enum { OPF_QP_MAX_OUTER = 60, OPF_QP_MAX_STALL = 4, OPF_QP_MAX_NEWTON = 60, OPF_QP_MAX_BACKTRACK = 30, OPF_MAX_NS = 64 };

OPF_FN double opf_qp_mult(double y, double rho, double c, double lo, double hi) {
  const double t = y + rho * (c - hi);
  if (t > 0.0) return t;
  const double u = y + rho * (c - lo);
  return u < 0.0 ? u : 0.0;
}

// The lanes that work on one env's QP together.  Every lane runs the same control flow: what decides a branch is either read from memory
// that all of them see or comes out of max() / sum(), which return the same bits in every lane.  sync() orders the team's stores
// before its later loads.  The host, and a caller that has one lane per env, use OpfSolo; opf.hip has the team of sub-lanes of a wave.
struct OpfSolo {
  OPF_MEM int lane() const { return 0; }
  OPF_MEM int lanes() const { return 1; }
  OPF_MEM void sync() const {}
  OPF_MEM double sum(double x) const { return x; }
  OPF_MEM double max(double x) const { return x; }
};

// the rows: c[0 .. ns) the box rows, c[ns .. ns + n) the voltage rows.  Row r, column i and row i of H belong to lane r (or i) % lanes.
struct OpfQp {
  int ns, n;
  OpfVec g, H, S;          // [ns], [ns][ns], [n][ns]
  OpfVec a, v; double vl, vu;   // a [ns]; v [n] = |V| by node
  OPF_MEM double lo(int r) const { return r < ns ? -1.0 - a[r] : vl - v[r - ns]; }
  OPF_MEM double hi(int r) const { return r < ns ? 1.0 - a[r] : vu - v[r - ns]; }
  template <class T> OPF_MEM void rows_times(const T& tm, const OpfVec& d, const OpfVec& c) const {              // c = A d
    for (int r = tm.lane(); r < ns + n; r += tm.lanes()) {
      if (r < ns) { c[r] = d[r]; continue; }
      double s = 0.0;
      for (int j = 0; j < ns; ++j) s += S[(size_t)(r - ns) * ns + j] * d[j];
      c[r] = s;
    }
  }
  template <class T> OPF_MEM void h_times(const T& tm, const OpfVec& d, const OpfVec& out) const {
    for (int i = tm.lane(); i < ns; i += tm.lanes()) { double s = 0.0; for (int j = 0; j < ns; ++j) s += H[(size_t)i * ns + j] * d[j]; out[i] = s; }
  }
};

// the KKT residual of the QP at (d, y): stationarity |g + H d + A' y|inf, violation, complementarity max |y_r| x distance to its bound.
// c, t: workspaces of ns + n and ns.  d and y are in place for every lane (synced by the caller).
template <class T>
OPF_FN void opf_qp_kkt(const T& tm, const OpfQp& q, const OpfVec& d, const OpfVec& y, const OpfVec& c, const OpfVec& t, double* st, double* vi,
                       double* co) {
  const int ns = q.ns, n = q.n, L = tm.lane(), NL = tm.lanes();
  q.rows_times(tm, d, c);
  q.h_times(tm, d, t);
  for (int i = L; i < ns; i += NL) t[i] += q.g[i] + y[i];
  for (int r = 0; r < n; ++r) { const double yr = y[ns + r]; if (yr != 0.0) for (int j = L; j < ns; j += NL) t[j] += q.S[(size_t)r * ns + j] * yr; }
  double s = 0.0, v = 0.0, m = 0.0;
  for (int i = L; i < ns; i += NL) s = fmax(s, fabs(t[i]));
  for (int r = L; r < ns + n; r += NL) {
    const double lo = q.lo(r), hi = q.hi(r), cr = c[r], yr = y[r];
    v = fmax(v, fmax(cr - hi, lo - cr));
    if (yr > 0.0) m = fmax(m, yr * fabs(hi - cr)); else if (yr < 0.0) m = fmax(m, -yr * fabs(cr - lo));
  }
  *st = tm.max(s); *vi = tm.max(fmax(v, 0.0)); *co = tm.max(m);
  tm.sync();
}
OPF_FN void opf_qp_kkt(const OpfQp& q, const OpfVec& d, const OpfVec& y, const OpfVec& c, const OpfVec& t, double* st, double* vi, double* co) {
  opf_qp_kkt(OpfSolo{}, q, d, y, c, t, st, vi, co);
}

struct OpfQpOut { int newton, capped; double kkt; };
// doubles of workspace: K | Hd Hp grad p | c Ap rho
OPF_FN size_t opf_qp_work(int ns, int n) { return (size_t)ns * ns + 4 * (size_t)ns + 3 * (size_t)(ns + n); }

template <class T>
OPF_FN OpfQpOut opf_qp_solve(const T& tm, const OpfQp& q, const OpfVec& d, const OpfVec& y, const OpfVec& w, int warm) {
  const int ns = q.ns, n = q.n, m = ns + n, L = tm.lane(), NL = tm.lanes();
  const size_t s = w.s;
  const OpfVec K{w.p, s}, Hd{K.p + (size_t)ns * ns * s, s}, Hp{Hd.p + ns * s, s}, gr{Hp.p + ns * s, s}, p{gr.p + ns * s, s},
      c{p.p + ns * s, s}, Ap{c.p + m * s, s}, rho{Ap.p + m * s, s};
  const OpfVec dg = Hp;                                  // the diagonal of the Cholesky factor, until Hp is formed
  double hmax = 1e-300, gs = 1e-300;
  for (int i = L; i < ns; i += NL) { hmax = fmax(hmax, fabs(q.H[(size_t)i * ns + i])); gs = fmax(gs, fabs(q.g[i])); d[i] = 0.0; }
  hmax = tm.max(hmax); gs = tm.max(gs);
  for (int r = L; r < m; r += NL) {
    double t = 1.0;
    if (r >= ns) { t = 0.0; for (int j = 0; j < ns; ++j) { const double x = q.S[(size_t)(r - ns) * ns + j]; t += x * x; } }
    rho[r] = OPF_QP_RHO * hmax / fmax(t, 1e-300);
    if (!warm) y[r] = 0.0;
  }
  tm.sync();
  OpfQpOut out{0, 1, 0.0};
  double vi_last = INFINITY;
  int stall = 0;
  for (int outer = 0; outer < OPF_QP_MAX_OUTER; ++outer) {
    q.rows_times(tm, d, c);
    tm.sync();
    for (int it = 0; it < OPF_QP_MAX_NEWTON; ++it) {
      // grad = g + H d + A' z
      q.h_times(tm, d, Hd);
      for (int i = L; i < ns; i += NL) gr[i] = q.g[i] + Hd[i] + opf_qp_mult(y[i], rho[i], c[i], q.lo(i), q.hi(i));
      for (int r = 0; r < n; ++r) {
        const double z = opf_qp_mult(y[ns + r], rho[ns + r], c[ns + r], q.lo(ns + r), q.hi(ns + r));
        if (z != 0.0) for (int j = L; j < ns; j += NL) gr[j] += q.S[(size_t)r * ns + j] * z;
      }
      double gmax = 0.0;
      for (int i = L; i < ns; i += NL) gmax = fmax(gmax, fabs(gr[i]));
      gmax = tm.max(gmax);
      if (gmax <= OPF_QP_EPS * gs) break;
      // K = H + sum over the penalised rows of rho_r a_r a_r' (lower triangle), + ridge
      double kmax = 1e-300;
      for (int i = L; i < ns; i += NL) {
        for (int j = 0; j <= i; ++j) K[(size_t)i * ns + j] = q.H[(size_t)i * ns + j];
        if (opf_qp_mult(y[i], rho[i], c[i], q.lo(i), q.hi(i)) != 0.0) K[(size_t)i * ns + i] += rho[i];
      }
      for (int r = 0; r < n; ++r)
        if (opf_qp_mult(y[ns + r], rho[ns + r], c[ns + r], q.lo(ns + r), q.hi(ns + r)) != 0.0) {
          const double rr = rho[ns + r];
          for (int i = L; i < ns; i += NL) {
            const double si = rr * q.S[(size_t)r * ns + i];
            for (int j = 0; j <= i; ++j) K[(size_t)i * ns + j] += si * q.S[(size_t)r * ns + j];
          }
        }
      for (int i = L; i < ns; i += NL) kmax = fmax(kmax, K[(size_t)i * ns + i]);
      kmax = tm.max(kmax);
      const double ridge = OPF_QP_RIDGE * kmax;
      for (int i = L; i < ns; i += NL) K[(size_t)i * ns + i] += ridge;
      tm.sync();
      // Cholesky K = C C' in place (the diagonal of C in dg), column by column: every lane forms the pivot, the rows below it are shared
      for (int j = 0; j < ns; ++j) {
        double dj = K[(size_t)j * ns + j];
        for (int k = 0; k < j; ++k) { const double x = K[(size_t)j * ns + k]; dj -= x * x; }
        dj = sqrt(fmax(dj, 1e-3 * ridge));
        if (j % NL == L) dg[j] = dj;
        for (int i = j + 1 + (L + NL - (j + 1) % NL) % NL; i < ns; i += NL) {
          double x = K[(size_t)i * ns + j];
          for (int k = 0; k < j; ++k) x -= K[(size_t)i * ns + k] * K[(size_t)j * ns + k];
          K[(size_t)i * ns + j] = x / dj;
        }
        tm.sync();
      }
      // p = -K^-1 grad: the two triangular solves are one lane's (ns^2 against the ns^3 above; gr is whole after the sync above)
      if (L == 0) {
        for (int i = 0; i < ns; ++i) {
          double x = -gr[i];
          for (int k = 0; k < i; ++k) x -= K[(size_t)i * ns + k] * p[k];
          p[i] = x / dg[i];
        }
        for (int i = ns - 1; i >= 0; --i) {
          double x = p[i];
          for (int k = i + 1; k < ns; ++k) x -= K[(size_t)k * ns + i] * p[k];
          p[i] = x / dg[i];
        }
      }
      tm.sync();
      out.newton++;
      // backtracking on phi along p: c(t) = c + t A p
      q.rows_times(tm, p, Ap);
      q.h_times(tm, p, Hp);
      double gd = 0.0, gp = 0.0, dHd = 0.0, dHp = 0.0, pHp = 0.0, slope = 0.0;
      for (int i = L; i < ns; i += NL) {
        gd += q.g[i] * d[i]; gp += q.g[i] * p[i]; dHd += d[i] * Hd[i]; dHp += p[i] * Hd[i]; pHp += p[i] * Hp[i]; slope += gr[i] * p[i];
      }
      gd = tm.sum(gd); gp = tm.sum(gp); dHd = tm.sum(dHd); dHp = tm.sum(dHp); pHp = tm.sum(pHp); slope = tm.sum(slope);
      double f0 = 0.0, t = 1.0;
      for (int bt = -1; bt < OPF_QP_MAX_BACKTRACK; ++bt) {       // bt == -1: phi at t = 0
        const double tt = bt < 0 ? 0.0 : t;
        double pen = 0.0;
        for (int r = L; r < m; r += NL) {
          const double z = opf_qp_mult(y[r], rho[r], c[r] + tt * Ap[r], q.lo(r), q.hi(r));
          pen += (z * z - y[r] * y[r]) / (2.0 * rho[r]);
        }
        pen = tm.sum(pen);
        const double ft = gd + tt * gp + 0.5 * (dHd + 2.0 * tt * dHp + tt * tt * pHp) + pen;
        if (bt < 0) { f0 = ft; continue; }
        if (ft <= f0 + 1e-4 * t * slope) break;
        t *= 0.5;
      }
      for (int i = L; i < ns; i += NL) d[i] += t * p[i];
      for (int r = L; r < m; r += NL) c[r] += t * Ap[r];
      tm.sync();
    }
    tm.sync();
    q.rows_times(tm, d, c);
    for (int r = L; r < m; r += NL) y[r] = opf_qp_mult(y[r], rho[r], c[r], q.lo(r), q.hi(r));
    tm.sync();
    double st, vi, co;
    opf_qp_kkt(tm, q, d, y, c, gr, &st, &vi, &co);
    out.kkt = fmax(fmax(st / gs, vi), co / gs);
    if (st <= OPF_QP_EPS * gs && vi <= OPF_QP_EPS && co <= OPF_QP_EPS * gs) { out.capped = 0; return out; }
    if (vi > OPF_QP_EPS && vi > OPF_QP_SHRINK * vi_last)
      for (int r = L; r < m; r += NL) {
        const double yr = y[r];
        if ((yr > 0.0 && c[r] < q.hi(r)) || (yr < 0.0 && c[r] > q.lo(r))) y[r] = 0.0;
      }
    tm.sync();
    stall = vi > OPF_QP_STALL * vi_last ? stall + 1 : 0;
    if (stall >= OPF_QP_MAX_STALL) break;          // the rows cannot be met inside the box: the least-violation compromise, reported as capped
    vi_last = vi;
  }
  return out;
}
OPF_FN OpfQpOut opf_qp_solve(const OpfQp& q, const OpfVec& d, const OpfVec& y, const OpfVec& w, int warm) {
  return opf_qp_solve(OpfSolo{}, q, d, y, w, warm);
}

// ---- the decision of k_opf_update for one env after its iter-th power flow (iter >= 1), as tests/opf_ref.py's loop takes it.
// run: 1 the point solved, go on from it; 2 it solved and the env stops there (status 0 or 1); 3 the power flow failed and the env
// stops at the last action that solved (status 2); 4 it failed: retry from the last solved action with half the step.
enum { OPF_CONVERGED = 0, OPF_MAX_ITER = 1, OPF_PF_FAILED = 2, OPF_STOPPED = 3, OPF_RUNNING = 255 };
enum { OPF_GO_NEXT = 1, OPF_GO_STOP = 2, OPF_GO_FAILED = 3, OPF_GO_RETRY = 4 };
struct OpfLimits { double step_tol, v_tol; int max_iter, max_backtrack; };
struct OpfDecision { int run, status, nback; double t; };
// solved: the power flow converged.  nback, t: failed power flows in a row and the step length so far.  dn = |d|inf of the QP at this
// point, capped: that QP hit its cap; viol, prev_viol: the violation here and at the last solved point before (NaN: there is none).
OPF_FN OpfDecision opf_decide(int iter, int solved, int nback, double t, double dn, double viol, double prev_viol, int capped, const OpfLimits& c) {
  if (!solved) {
    const int nb = nback + 1;
    if (iter == 1 || nb > c.max_backtrack || iter >= c.max_iter) return {OPF_GO_FAILED, OPF_PF_FAILED, nb, t};
    return {OPF_GO_RETRY, OPF_RUNNING, nb, 0.5 * t};
  }
  if (!capped && dn < c.step_tol && viol <= c.v_tol) return {OPF_GO_STOP, OPF_CONVERGED, 0, 1.0};
  // a capped QP: the linearised bounds cannot be met inside the box.  With a step below step_tol, or a violation that came down by less
  // than v_tol since the last solved point (false for NaN), the env stands at a least-violation point: it stops there, as at max_iter
  if (iter >= c.max_iter || (capped && (dn < c.step_tol || prev_viol - viol < c.v_tol))) return {OPF_GO_STOP, OPF_MAX_ITER, 0, 1.0};
  return {OPF_GO_NEXT, OPF_RUNNING, 0, 1.0};
}
// the action of the next power flow: from the last solved action along the last QP's step
OPF_FN double opf_trial(double a_sol, double t, double d) { return fmin(1.0, fmax(-1.0, a_sol + t * d)); }

}  // namespace mapdn
