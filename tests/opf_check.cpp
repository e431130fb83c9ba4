// Host build of mapdn_amd/csrc/opf.hpp for tests/test_opf_cpu.py: reads a file of doubles, writes a file of doubles.
//   tree: 0, n, ns, nc | par[n] | cptr[n + 1] | cidx[nc] | yt[n][OPF_YT] | e[n] | f[n] | sg_node[ns] | w[ns]
//         -> x[n][ns][2] = (dtheta, u = d|V| / |V|) of J X = E by the tree elimination
//   qp:   1, n, ns, vl, vu | g[ns] | H[ns][ns] | S[n][ns] | v[n] | a[ns]
//         -> d[ns] | y[ns + n] | newton, capped, kkt | stationarity, violation, complementarity (opf_qp_kkt at (d, y))
//   linearise: 4, n, ns, nc | as tree | vm[n] | loss_slack
//         -> S[n][ns] | g[ns] | H[ns][ns] | loss: the elimination of opf.hpp, then k_opf_linearise's sums (M V, dV, W = M dV, g, H, the
//            loss) restated for the host in the kernel's order — what float64 without pivoting gives on that net at that V
//   decide: 3, step_tol, v_tol, max_iter, max_backtrack | rows of (iter, solved, nback, t, dn, viol, prev_viol, capped)
//         -> rows of (run, status, nback, t) by opf_decide
//   qp by a team: 2, lanes, then as qp — the same routine shared by `lanes` threads, as the sub-lanes of the kernel share it
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

#include "opf.hpp"

using namespace mapdn;

static std::vector<double> read_all(const char* path) {
  std::vector<double> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  double x;
  while (fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
  fclose(f);
  return v;
}

// a team of host threads: sync() is a barrier, sum() and max() go over the lanes' values in lane order, the same in every lane
struct TeamShared {
  int nl, waiting = 0; long phase = 0;
  std::mutex m; std::condition_variable cv;
  std::vector<double> buf;
  explicit TeamShared(int n) : nl(n), buf((size_t)n) {}
  void barrier() {
    std::unique_lock<std::mutex> lk(m);
    const long ph = phase;
    if (++waiting == nl) { waiting = 0; ++phase; cv.notify_all(); }
    else cv.wait(lk, [&] { return phase != ph; });
  }
};
struct ThreadTeam {
  int l; TeamShared* sh;
  int lane() const { return l; }
  int lanes() const { return sh->nl; }
  void sync() const { sh->barrier(); }
  template <class F> double reduce(double x, F f) const {
    sh->buf[(size_t)l] = x;
    sh->barrier();
    double r = sh->buf[0];
    for (int i = 1; i < sh->nl; ++i) r = f(r, sh->buf[(size_t)i]);
    sh->barrier();
    return r;
  }
  double sum(double x) const { return reduce(x, [](double a, double b) { return a + b; }); }
  double max(double x) const { return reduce(x, [](double a, double b) { return fmax(a, b); }); }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::vector<double> in = read_all(argv[1]);
  if (in.size() < 4) return 3;
  std::vector<double> out;
  size_t o = 0;
  const int mode = (int)in[o++];
  if (mode == 0) {
    const int n = (int)in[o++], ns = (int)in[o++], nc = (int)in[o++];
    if (in.size() != (size_t)4 + n + (n + 1) + nc + (size_t)n * OPF_YT + 2 * n + 2 * ns) return 4;
    std::vector<int32_t> par(n), cptr(n + 1), cidx(nc), sg(ns);
    for (int& p : par) p = (int)in[o++];
    for (int& p : cptr) p = (int)in[o++];
    for (int& p : cidx) p = (int)in[o++];
    const double* yt = &in[o]; o += (size_t)n * OPF_YT;
    OpfVec e{&in[o], 1}; o += n;
    OpfVec f{&in[o], 1}; o += n;
    for (int& p : sg) p = (int)in[o++];
    const double* w = &in[o];
    std::vector<double> fac((size_t)n * OPF_FAC);
    OpfVec F{fac.data(), 1};
    double P, Q;
    for (int k = 0; k < n; ++k) opf_elim_step(k, n, par.data(), cptr.data(), cidx.data(), yt, e, f, F, &P, &Q);
    out.assign((size_t)n * ns * 2, 0.0);
    for (int j = 0; j < ns; ++j) opf_solve_column(sg[j], w[j], n, par.data(), F, OpfVec{out.data() + (size_t)j * 2, 1}, (size_t)ns * 2);
  } else if (mode == 4) {
    const int n = (int)in[o++], ns = (int)in[o++], nc = (int)in[o++];
    if (in.size() != (size_t)4 + n + (n + 1) + nc + (size_t)n * OPF_YT + 2 * n + 2 * ns + n + 1) return 4;
    std::vector<int32_t> par(n), cptr(n + 1), cidx(nc), sg(ns);
    for (int& p : par) p = (int)in[o++];
    for (int& p : cptr) p = (int)in[o++];
    for (int& p : cidx) p = (int)in[o++];
    const double* yt = &in[o]; o += (size_t)n * OPF_YT;
    const double* E = &in[o]; o += n;
    const double* F = &in[o]; o += n;
    for (int& p : sg) p = (int)in[o++];
    const double* w = &in[o]; o += ns;
    const double* VM = &in[o]; o += n;
    const double loss_slack = in[o];
    std::vector<double> fac((size_t)n * OPF_FAC), mv((size_t)n * 2), X((size_t)n * ns * 2), W((size_t)n * ns * 2);
    OpfVec Fc{fac.data(), 1}, e{const_cast<double*>(E), 1}, f{const_cast<double*>(F), 1};
    const size_t xs = (size_t)ns * 2;
    for (int k = 0; k < n; ++k) {
      const double* y = yt + (size_t)k * OPF_YT;
      double mr = y[OY_KK] * E[k] + y[OY_MSV], mi = y[OY_KK] * F[k] + y[OY_MSV + 1];
      const int p = par[k];
      if (p < n) { mr += y[OY_MKP] * E[p] - y[OY_MKP + 1] * F[p]; mi += y[OY_MKP] * F[p] + y[OY_MKP + 1] * E[p]; }
      for (int i = cptr[k]; i < cptr[k + 1]; ++i) {
        const int c = cidx[i];
        const double* yc = yt + (size_t)c * OPF_YT;
        mr += yc[OY_MKP] * E[c] + yc[OY_MKP + 1] * F[c]; mi += yc[OY_MKP] * F[c] - yc[OY_MKP + 1] * E[c];
      }
      mv[(size_t)k * 2] = mr; mv[(size_t)k * 2 + 1] = mi;
    }
    double P, Q;
    for (int k = 0; k < n; ++k) opf_elim_step(k, n, par.data(), cptr.data(), cidx.data(), yt, e, f, Fc, &P, &Q);
    double loss = loss_slack;
    for (int k = 0; k < n; ++k) {
      const double* y = yt + (size_t)k * OPF_YT;
      loss += E[k] * mv[(size_t)k * 2] + F[k] * mv[(size_t)k * 2 + 1] + (y[OY_MSV] * E[k] + y[OY_MSV + 1] * F[k]);
    }
    out.assign((size_t)n * ns + ns + (size_t)ns * ns + 1, 0.0);
    double *S = out.data(), *g = S + (size_t)n * ns, *H = g + ns;
    for (int j = 0; j < ns; ++j) {
      double* x = X.data() + (size_t)j * 2; double* wv = W.data() + (size_t)j * 2;
      opf_solve_column(sg[j], w[j], n, par.data(), Fc, OpfVec{x, 1}, xs);
      for (int k = 0; k < n; ++k) {
        const double th = x[(size_t)k * xs], u = x[(size_t)k * xs + 1];
        S[(size_t)k * ns + j] = u * VM[k];
        x[(size_t)k * xs] = u * E[k] - th * F[k]; x[(size_t)k * xs + 1] = u * F[k] + th * E[k];
      }
      double gj = 0.0;
      for (int k = 0; k < n; ++k) {
        const double* y = yt + (size_t)k * OPF_YT;
        const double de = x[(size_t)k * xs], df = x[(size_t)k * xs + 1];
        double wr = y[OY_KK] * de, wi = y[OY_KK] * df;
        const int pk = par[k];
        if (pk < n) {
          const double pe = x[(size_t)pk * xs], pf = x[(size_t)pk * xs + 1];
          wr += y[OY_MKP] * pe - y[OY_MKP + 1] * pf; wi += y[OY_MKP] * pf + y[OY_MKP + 1] * pe;
        }
        for (int i = cptr[k]; i < cptr[k + 1]; ++i) {
          const int c = cidx[i];
          const double* yc = yt + (size_t)c * OPF_YT;
          const double ce = x[(size_t)c * xs], cf = x[(size_t)c * xs + 1];
          wr += yc[OY_MKP] * ce + yc[OY_MKP + 1] * cf; wi += yc[OY_MKP] * cf - yc[OY_MKP + 1] * ce;
        }
        wv[(size_t)k * xs] = wr; wv[(size_t)k * xs + 1] = wi;
        gj += de * mv[(size_t)k * 2] + df * mv[(size_t)k * 2 + 1];
      }
      g[j] = 2.0 * gj;
    }
    for (int j = 0; j < ns; ++j)
      for (int i = 0; i <= j; ++i) {
        const double* x = X.data() + (size_t)i * 2; const double* wv = W.data() + (size_t)j * 2;
        double h = 0.0;
        for (int k = 0; k < n; ++k) h += x[(size_t)k * xs] * wv[(size_t)k * xs] + x[(size_t)k * xs + 1] * wv[(size_t)k * xs + 1];
        H[(size_t)i * ns + j] = H[(size_t)j * ns + i] = 2.0 * h;
      }
    out.back() = loss;
  } else if (mode == 1 || mode == 2) {
    const int lanes = mode == 2 ? (int)in[o++] : 1;
    if (lanes < 1 || lanes > 64) return 4;
    const size_t o0 = o;
    const int n = (int)in[o++], ns = (int)in[o++];
    if (ns > OPF_MAX_NS || in.size() != o0 + 4 + ns + (size_t)ns * ns + (size_t)n * ns + n + ns) return 4;
    OpfQp q;
    q.ns = ns; q.n = n; q.vl = in[o++]; q.vu = in[o++];
    q.g = OpfVec{&in[o], 1}; o += ns;
    q.H = OpfVec{&in[o], 1}; o += (size_t)ns * ns;
    q.S = OpfVec{&in[o], 1}; o += (size_t)n * ns;
    q.v = OpfVec{&in[o], 1}; o += n;
    q.a = OpfVec{&in[o], 1};
    std::vector<double> d(ns), y(ns + n), w(opf_qp_work(ns, n)), c(ns + n), t(ns);
    OpfQpOut r{};
    if (mode == 1) r = opf_qp_solve(q, OpfVec{d.data(), 1}, OpfVec{y.data(), 1}, OpfVec{w.data(), 1}, 0);
    else {
      TeamShared sh(lanes);
      std::vector<OpfQpOut> rs((size_t)lanes);
      std::vector<std::thread> th;
      for (int l = 0; l < lanes; ++l)
        th.emplace_back([&, l] { rs[(size_t)l] = opf_qp_solve(ThreadTeam{l, &sh}, q, OpfVec{d.data(), 1}, OpfVec{y.data(), 1}, OpfVec{w.data(), 1}, 0); });
      for (auto& t : th) t.join();
      r = rs[0];
      for (const OpfQpOut& x : rs) if (x.newton != r.newton || x.capped != r.capped || x.kkt != r.kkt) return 7;   // the lanes took one path
    }
    double st, vi, co;
    opf_qp_kkt(q, OpfVec{d.data(), 1}, OpfVec{y.data(), 1}, OpfVec{c.data(), 1}, OpfVec{t.data(), 1}, &st, &vi, &co);
    out = d;
    out.insert(out.end(), y.begin(), y.end());
    for (double x : {(double)r.newton, (double)r.capped, r.kkt, st, vi, co}) out.push_back(x);
  } else if (mode == 3) {
    if (in.size() < 5 || (in.size() - 5) % 8 != 0) return 4;
    const OpfLimits c{in[1], in[2], (int)in[3], (int)in[4]};
    for (o = 5; o < in.size(); o += 8) {
      const OpfDecision d = opf_decide((int)in[o], (int)in[o + 1], (int)in[o + 2], in[o + 3], in[o + 4], in[o + 5], in[o + 6], (int)in[o + 7], c);
      for (double x : {(double)d.run, (double)d.status, (double)d.nback, d.t}) out.push_back(x);
    }
  } else return 5;
  FILE* g = fopen(argv[2], "wb");
  if (!g) return 6;
  fwrite(out.data(), sizeof(double), out.size(), g);
  fclose(g);
  return 0;
}
