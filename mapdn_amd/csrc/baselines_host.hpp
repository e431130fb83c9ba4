// baselines_host.hpp — the host side of the traditional baselines (mapdn_droop_actions, mapdn_opf_actions, mapdn_opf_probe): their
// configs' defaults and refusals, their workspaces, and the one loop driver both run in (the device side of that frame: ctlloop.hpp);
// and of mapdn_evaluate_actions, which scores candidate actions in the same frame (whatif_prepare, whatif_run at the end).
// Included by capi.hip after mapdn_handle and its helpers (dalloc, dupload, nr_launch, transpose_out), outside its extern "C" block;
// the entry points stay there.
#pragma once

// ---- the frame.  Before the first solve: nobody counted yet in n_active[0 .. solves]; an Sbus that holds
// mapdn_solve_only's inputs rebuilt from the env's loads (q = 0; sbus_stale is read, not cleared: the next step() rebuilds Sbus as
// well); and in *dd the handle's Dev with the loop's own active / iters / conv arrays: its solves skip the envs that stopped and leave
// the env's flags alone.
static int ctl_begin(mapdn_handle* h, const CtlLoop& s, int solves, hipStream_t st, Dev* dd) {
  const Dev& d = h->d;
  HIPCHK(h, hipMemsetAsync(s.n_active, 0, ((size_t)solves + 1) * sizeof(int32_t), st));
  if (h->sbus_stale) {
    HIPCHK(h, hipMemsetAsync(s.a, 0, (size_t)d.ns * d.Bp * sizeof(double), st));
    launch_inject(d, MODE_SOLVE, nullptr, MAPDN_F64, d.cur_pl, d.cur_ql, d.cur_pv, s.a, 0, st);
  }
  *dd = d;
  dd->active = s.act; dd->iters = const_cast<int32_t*>(s.nr_iters); dd->conv = const_cast<uint8_t*>(s.nr_conv);
  return MAPDN_OK;
}

// The loop for every env at once: launch(dd, 0) is the start launch, then per iteration the solve (MODE_SOLVE on dd) and launch(dd, i)
// after the i-th solve, at most s.max_iter times.  The host reads the number of envs still iterating every `poll` iterations only, so at
// most poll - 1 solves run after the last env stopped.  Then the exports every loop has: a_sol, iters, status.  Writes only what the
// next step() overwrites before it reads it: the PV-bus and several-load-bus entries of the Sbus buffer that solve reads (d.sb_off;
// all of it when Sbus is stale, as the next step() rebuilds it then anyway) and the solver's Vout rows.
template <class Launch>
static int ctl_drive(mapdn_handle* h, const CtlLoop& s, int poll, double* actions, int32_t* iterations, uint8_t* status, hipStream_t st,
                     Launch launch) {
  Dev dd;
  if (const int rc = ctl_begin(h, s, s.max_iter, st, &dd)) return rc;
  launch(dd, 0);
  for (int i = 0; i < s.max_iter; ++i) {         // i power flows solved so far
    if (i % poll == 0) {
      int32_t left = 0;
      HIPCHK(h, hipMemcpyAsync(&left, s.n_active + i, sizeof(left), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
      if (left == 0) break;
    }
    nr_launch(h, MODE_SOLVE, nullptr, nullptr, nullptr, st, nullptr, 0, &dd);
    launch(dd, i + 1);
  }
  transpose_out(h, s.a_sol, 1.0, h->iota_idx, actions, dd.ns, st);
  launch_copy_i32(s.iters, iterations, dd.B, st);
  launch_copy_u8(s.status, status, dd.B, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
}

// ---- droop baseline (droop.hip): the script's defaults for the fields left 0, and its refusals
static const char* droop_resolve(const mapdn_droop_config* in, mapdn_droop_config& c) {
  if (in) c = *in; else std::memset(&c, 0, sizeof(c));
  if (c.va == 0.0) c.va = 0.95;                  // pf_droop_matpower_all.m: the law's breakpoints, damping, stopping rule,
  if (c.vb == 0.0) c.vb = 1.0;                   // reactive_ratio of q_max = min(sqrt(S^2 - p^2), ratio S)
  if (c.vc == 0.0) c.vc = 1.0;
  if (c.vd == 0.0) c.vd = 1.05;
  if (c.damping == 0.0) c.damping = 0.1;
  if (c.max_iter == 0) c.max_iter = 100;
  if (c.v_tol == 0.0) c.v_tol = 1e-4;
  if (c.reactive_ratio == 0.0) c.reactive_ratio = 1.0;
  if (!(c.va < c.vb && c.vb <= c.vc && c.vc < c.vd)) return "droop: the breakpoints must satisfy va < vb <= vc < vd";
  if (!(c.damping > 0.0 && c.damping <= 1.0)) return "droop: damping must lie in (0, 1]";
  if (c.max_iter < 1 || c.max_iter > DROOP_MAX_ITER_CAP) return "droop: max_iter must lie in 1 ... 10000";
  if (!(c.v_tol > 0.0)) return "droop: v_tol must be > 0";
  if (!(c.reactive_ratio > 0.0)) return "droop: reactive_ratio must be > 0";
  return nullptr;
}

// the workspace of the droop loop (DroopState), once per handle
static int droop_prepare(mapdn_handle* h) {
  if (h->droop_ready) return MAPDN_OK;
  const Plan& P = h->plan;
  DroopState& s = h->droop;
  const size_t Bp = h->d.Bp, ns = (size_t)P.ns;
  int32_t *iters = nullptr, *nr_iters = nullptr, *n_active = nullptr; uint8_t *status = nullptr, *act = nullptr, *nr_conv = nullptr;
  int rc;
  if ((rc = dalloc(h, &s.a, ns * Bp)) || (rc = dalloc(h, &s.a_sol, ns * Bp)) || (rc = dalloc(h, &s.v_last, ns * Bp)) ||
      (rc = dalloc(h, &s.dv2, ns * Bp)) ||
      (rc = dalloc(h, &iters, Bp)) || (rc = dalloc(h, &nr_iters, Bp)) || (rc = dalloc(h, &status, Bp)) || (rc = dalloc(h, &act, Bp)) ||
      (rc = dalloc(h, &nr_conv, Bp)) || (rc = dalloc(h, &n_active, (size_t)DROOP_MAX_ITER_CAP + 1)))
    return rc;
  s.iters = iters; s.nr_iters = nr_iters; s.status = status; s.act = act; s.nr_conv = nr_conv; s.n_active = n_active;
  std::vector<int32_t> vrow(std::max<size_t>(ns, 1), 0);           // |V| of sgen j's bus: the Vout row of its node (alloc_nrbuf)
  for (size_t j = 0; j < ns; ++j) vrow[j] = (int32_t)h->d.r_vout + VOF * P.pos_of_obus[P.sgen_bus[j]] + VO_VM;
  const int32_t* vr = nullptr;
  if ((rc = dupload(h, &vr, vrow))) return rc;
  s.sg_vrow = vr; s.vm_row = h->vm_row;
  h->droop_ready = true;
  return MAPDN_OK;
}

// The loop of pf_droop_matpower_all.m:84-162: between the solves, k_droop_update.
static int droop_run(mapdn_handle* h, const mapdn_droop_config& c, double* actions, double* vm_pu, int32_t* iterations,
                     uint8_t* status, hipStream_t st) {
  constexpr int DROOP_POLL = 4;
  if (const int rc = droop_prepare(h)) return rc;
  const Dev& d = h->d;
  DroopState s = h->droop;
  s.va = c.va; s.vb = c.vb; s.vc = c.vc; s.vd = c.vd; s.damping = c.damping; s.v_tol = c.v_tol; s.ratio = c.reactive_ratio;
  s.max_iter = c.max_iter; s.vm_out = vm_pu;
  return ctl_drive(h, s, DROOP_POLL, actions, iterations, status, st, [&](const Dev&, int iter) { launch_droop_update(d, s, iter, st); });
}

// ---- shared by the OPF baseline and mapdn_action_gradients.
// The solver gate: the tree solver on a radial net answers; with the entry point's knob at 1 a k_nr_sparse handle answers too; nothing
// else does.  nullptr, or the refusal under the entry point's prefix.
static const char* solver_gate(const mapdn_handle* h, const char* prefix, const char* knob, bool knob_on) {
  if ((h->plan.radial && h->solver == 0) || (knob_on && h->solver == 1)) return nullptr;
  static thread_local std::string why;
  why = std::string(prefix) +
        (knob_on ? ": meshed nets and radial ones on the dense solver (nr_solver = dense, k_nr_dense) are not supported (" + std::string(knob) +
                       " = 1 covers the sparse solver)"
                 : std::string(": meshed nets and handles on another solver than the tree solver are not supported"));
  return why.c_str();
}
// the node of every sgen (position; n: the slack)
static std::vector<int32_t> sgen_nodes(const Plan& P) {
  std::vector<int32_t> sgn(std::max<size_t>((size_t)P.ns, 1), 0);
  for (size_t j = 0; j < (size_t)P.ns; ++j) sgn[j] = P.pos_of_obus[P.sgen_bus[j]];
  return sgn;
}
// the result of a *_sparse_prepare(sp_lanes) of sparse_prog.hpp's sp_prepare as a return code
static int sparse_prepared(mapdn_handle* h, int rc, const char* kernel) {
  if (rc == 0) return MAPDN_OK;
  (void)hipGetLastError();
  h->err = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for ") + kernel;
  return MAPDN_E_HIP;
}

// ---- OPF baseline (opf.hip, opf.hpp; opf_sparse.hip): the defaults for the fields left 0, the config's ranges and what the
// linearisation does not cover.  meshed = 1 lets a k_nr_sparse handle answer (the elimination program in place of the tree sweeps);
// 0 keeps the tree solver alone.
static const char* opf_resolve(const mapdn_handle* h, const mapdn_opf_config* in, mapdn_opf_config& c) {
  if (in) c = *in; else std::memset(&c, 0, sizeof(c));
  if (c.v_lower == 0.0) c.v_lower = h->cfg.v_lower;
  if (c.v_upper == 0.0) c.v_upper = h->cfg.v_upper;
  if (c.v_tol == 0.0) c.v_tol = 5e-6;             // MATPOWER's opf.violation
  if (c.step_tol == 0.0) c.step_tol = 1e-6;
  if (c.max_iter == 0) c.max_iter = 50;
  if (c.max_backtrack == 0) c.max_backtrack = 8;
  if (!(c.v_lower > 0.0 && c.v_lower < c.v_upper)) return "opf: the bounds must satisfy 0 < v_lower < v_upper";
  if (!(c.v_tol > 0.0)) return "opf: v_tol must be > 0";
  if (!(c.step_tol > 0.0)) return "opf: step_tol must be > 0";
  if (c.max_iter < 1 || c.max_iter > OPF_MAX_ITER_CAP) return "opf: max_iter must lie in 1 ... 1000";
  if (c.max_backtrack < 1 || c.max_backtrack > 60) return "opf: max_backtrack must lie in 1 ... 60";
  if (c.meshed != 0 && c.meshed != 1) return "opf: meshed must be 0 or 1";
  const Plan& P = h->plan;
  if (const char* why = solver_gate(h, "opf", "meshed", c.meshed == 1)) return why;
  if (P.zip) return "opf: voltage-dependent (ZIP) loads are not supported";
  if (P.n_gen) return "opf_actions: nets with generators (net.gen, gen buses) are not supported (k_opf_linearise takes every non-slack bus as a PQ bus)";
  if (P.gen_start) return "opf_actions: a start other than ext_grid_vm_pu (vm_init_pu: out-of-service net.gen rows) is not supported (the loop's solves start at the ext_grid set-point)";
  if (P.nbo != P.nb || !P.fused_obus.empty() || !P.alias_pos.empty()) return "opf: fused buses are not supported";
  if (P.ns > OPF_MAX_NS) return "opf: more than 64 sgens are not supported";
  return nullptr;
}

// the topology tables of the tree elimination (OpfState: par, cptr, cidx, sg_node, yt, loss_slack), once per handle; grad_prepare
// takes them as well
static int opf_tables(mapdn_handle* h) {
  if (h->opf_tables_ready) return MAPDN_OK;
  const Plan& P = h->plan;
  OpfState& s = h->opf;
  const size_t n = (size_t)P.n;
  // children of every node in the canonical order of the sweeps: the chain child k - 1 first, then ascending positions
  std::vector<int32_t> cptr(n + 1, 0), cidx;
  {
    std::vector<std::vector<int32_t>> ch(n);
    for (int k = 0; k < P.n; ++k) if (P.par[k] < P.n) ch[(size_t)P.par[k]].push_back(k);     // ascending k
    for (size_t k = 0; k < n; ++k) {
      auto& c = ch[k];
      if (!c.empty() && c.back() == (int32_t)k - 1) { c.pop_back(); c.insert(c.begin(), (int32_t)k - 1); }
      cidx.insert(cidx.end(), c.begin(), c.end());
      cptr[k + 1] = (int32_t)cidx.size();
    }
  }
  // Y constants of Plan::yc, then M = (Y + Y^H) / 2: M_k,parent and M_k,slack V_slack (Y_slack,k from root_children / root_y)
  std::vector<double> yt(std::max<size_t>(n, 1) * OPF_YT, 0.0);
  std::vector<cplx> ysk(n, cplx(0, 0));
  for (size_t i = 0; i < P.root_children.size(); ++i) ysk[(size_t)P.root_children[i]] = cplx(P.root_y[2 * i], P.root_y[2 * i + 1]);
  for (size_t k = 0; k < n; ++k) {
    const double* c = &P.yc[k * 8];
    double* y = &yt[k * OPF_YT];
    for (int i = 0; i < 8; ++i) y[i] = c[i];
    const cplx mkp = 0.5 * (cplx(c[2], c[3]) + std::conj(cplx(c[4], c[5])));
    const cplx msv = 0.5 * (cplx(c[6], c[7]) + std::conj(ysk[k]) * P.vroot);
    y[OY_MKP] = mkp.real(); y[OY_MKP + 1] = mkp.imag(); y[OY_MSV] = msv.real(); y[OY_MSV + 1] = msv.imag();
  }
  std::vector<int32_t> par(std::max<size_t>(n, 1), 0);
  for (size_t k = 0; k < n; ++k) par[k] = P.par[k];
  int rc;
  if ((rc = dupload(h, &s.par, par)) || (rc = dupload(h, &s.cptr, cptr)) || (rc = dupload(h, &s.cidx, cidx)) ||
      (rc = dupload(h, &s.sg_node, sgen_nodes(P))) || (rc = dupload(h, &s.yt, yt)))
    return rc;
  s.loss_slack = P.yrr[0] * P.vroot * P.vroot;
  h->opf_tables_ready = true;
  return MAPDN_OK;
}

// the tables of the sparse path (opf_sparse.hip), once per handle: the node of every sgen, the rows of M (plan.cpp opf_sparse_table),
// the slack's own term of the loss
static int opf_tables_sparse(mapdn_handle* h) {
  const Plan& P = h->plan;
  OpfState& s = h->opf;
  OsM& m = h->opf_m;
  std::vector<int32_t> ptr, col;
  std::vector<double> val, msv;
  opf_sparse_table(P, ptr, col, val, msv);
  if (col.empty()) { col.push_back(0); val.assign(2, 0.0); }
  int rc;
  if ((rc = dupload(h, &s.sg_node, sgen_nodes(P))) || (rc = dupload(h, &m.ptr, ptr)) || (rc = dupload(h, &m.col, col)) ||
      (rc = dupload(h, &m.val, val)) || (rc = dupload(h, &m.msv, msv)))
    return rc;
  s.loss_slack = P.yrr[0] * P.vroot * P.vroot;
  return sparse_prepared(h, opf_sparse_prepare(h->sp_lanes), "k_opf_sens_sparse");
}

// the tables and the workspace of the OPF loop (OpfState), once per handle; a k_nr_sparse handle has no factors in global memory
static int opf_prepare(mapdn_handle* h) {
  if (h->opf_ready) return MAPDN_OK;
  int rc;
  const bool sparse = h->solver == 1;
  if ((rc = sparse ? opf_tables_sparse(h) : opf_tables(h))) return rc;
  const Plan& P = h->plan;
  OpfState& s = h->opf;
  const size_t Bp = h->d.Bp, ns = (size_t)P.ns, n = (size_t)P.n;
  s.vm_row = h->vm_row;
  int32_t *nr_iters = nullptr; uint8_t* nr_conv = nullptr;
  if ((rc = sparse ? MAPDN_OK : dalloc(h, &s.fac, n * OPF_FAC * Bp)) || (rc = dalloc(h, &s.mv, n * 2 * Bp)) || (rc = dalloc(h, &s.X, n * ns * 2 * Bp)) ||
      (rc = dalloc(h, &s.W, n * ns * 2 * Bp)) || (rc = dalloc(h, &s.S, n * ns * Bp)) || (rc = dalloc(h, &s.H, ns * ns * Bp)) ||
      (rc = dalloc(h, &s.g, ns * Bp)) || (rc = dalloc(h, &s.qd, ns * Bp)) || (rc = dalloc(h, &s.qy, (ns + n) * Bp)) ||
      (rc = dalloc(h, &s.qw, opf_qp_work((int)ns, (int)n) * Bp)) || (rc = dalloc(h, &s.a, ns * Bp)) || (rc = dalloc(h, &s.a_sol, ns * Bp)) ||
      (rc = dalloc(h, &s.t, Bp)) || (rc = dalloc(h, &s.loss, Bp)) || (rc = dalloc(h, &s.viol, Bp)) || (rc = dalloc(h, &s.loss_out, Bp)) ||
      (rc = dalloc(h, &s.viol_out, Bp)) || (rc = dalloc(h, &s.iters, Bp)) || (rc = dalloc(h, &s.nback, Bp)) ||
      (rc = dalloc(h, &s.status, Bp)) || (rc = dalloc(h, &s.act, Bp)) || (rc = dalloc(h, &s.lin, Bp)) ||
      (rc = dalloc(h, &s.qp_capped, Bp)) || (rc = dalloc(h, &nr_iters, Bp)) || (rc = dalloc(h, &nr_conv, Bp)) ||
      (rc = dalloc(h, &s.n_active, (size_t)OPF_MAX_ITER_CAP + 1)))
    return rc;
  s.nr_iters = nr_iters; s.nr_conv = nr_conv;
  h->opf_ready = true;
  return MAPDN_OK;
}

// the handle's OpfState with the config's limits, where the caller wants |V| and the set-points the start launch begins from (nullptr: a = 0)
static OpfState opf_state(const mapdn_handle* h, const mapdn_opf_config& c, double* vm_out, const double* a0) {
  OpfState s = h->opf;
  s.v_lower = c.v_lower; s.v_upper = c.v_upper; s.v_tol = c.v_tol; s.step_tol = c.step_tol;
  s.max_iter = c.max_iter; s.max_backtrack = c.max_backtrack; s.vm_out = vm_out; s.a0 = a0;
  return s;
}

// The linearisation launch of the handle's solver: k_opf_linearise on the tree, k_opf_sens_sparse and k_opf_reduce_sparse on k_nr_sparse.
static void opf_linearise(const mapdn_handle* h, const Dev& dd, const OpfState& s, hipStream_t st) {
  if (h->solver == 1) launch_opf_linearise_sparse(dd, s, h->opf_m, st);
  else launch_opf_linearise(dd, s, st);
}

// The SQP loop: after every solve the linearisation and k_opf_qp on the solver's Dev (the OPF's own active set), then k_opf_update.
static int opf_run(mapdn_handle* h, const mapdn_opf_config& c, double* actions, double* vm_pu, double* loss_mw, double* violation,
                   int32_t* iterations, uint8_t* status, hipStream_t st) {
  constexpr int OPF_POLL = 2;
  if (const int rc = opf_prepare(h)) return rc;
  const Dev& d = h->d;
  const OpfState s = opf_state(h, c, vm_pu, nullptr);
  const int rc = ctl_drive(h, s, OPF_POLL, actions, iterations, status, st, [&](const Dev& dd, int iter) {
    if (iter > 0) { opf_linearise(h, dd, s, st); launch_opf_qp(dd, s, st); }
    launch_opf_update(d, s, iter, st);
  });
  if (rc) return rc;
  if (loss_mw) transpose_out(h, s.loss_out, d.sn, h->iota_idx, loss_mw, 1, st);
  if (violation) transpose_out(h, s.viol_out, 1.0, h->iota_idx, violation, 1, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
}

// mapdn_opf_probe: the frame stopped after one solve — the start launch from the caller's a (it writes the Sbus of that a), the solve,
// k_opf_linearise, k_opf_qp, no k_opf_update after them — then the workspace as it stands, env-major.
static int opf_probe(mapdn_handle* h, const mapdn_opf_config& c, const double* a, int32_t ns, double* v_re, double* v_im, double* vm, double* S,
                     double* g, double* H, double* loss_mw, double* violation, double* d, double* y, uint8_t* linearised,
                     uint8_t* qp_capped, hipStream_t st) {
  if (const int rc = opf_prepare(h)) return rc;
  const Dev& dv = h->d;
  const int n = dv.n;
  const int io = std::max(std::max(n * ns, ns * ns), ns + n);      // identity rows for the widest export
  if (!h->opf_probe_a) { if (const int rc = dalloc(h, &h->opf_probe_a, (size_t)ns * dv.Bp)) return rc; }
  if (!h->opf_probe_rows) {
    std::vector<int32_t> rows((size_t)io + 3 * (size_t)n);
    for (int i = 0; i < io; ++i) rows[(size_t)i] = i;
    for (int k = 0; k < n; ++k) {
      rows[(size_t)io + k] = (int32_t)dv.r_vout + VOF * k + VO_E; rows[(size_t)io + n + k] = (int32_t)dv.r_vout + VOF * k + VO_F;
      rows[(size_t)io + 2 * n + k] = (int32_t)dv.r_vout + VOF * k + VO_VM;
    }
    if (const int rc = dupload(h, &h->opf_probe_rows, rows)) return rc;
  }
  const int32_t* iota = h->opf_probe_rows;
  const int32_t* erow = iota + io;
  const OpfState s = opf_state(h, c, nullptr, h->opf_probe_a);
  launch_to_envminor(dv, a, h->opf_probe_a, ns, st);
  Dev dd;
  if (const int rc = ctl_begin(h, s, 0, st, &dd)) return rc;
  launch_opf_update(dv, s, 0, st);
  nr_launch(h, MODE_SOLVE, nullptr, nullptr, nullptr, st, nullptr, 0, &dd);
  opf_linearise(h, dd, s, st);
  launch_opf_qp(dd, s, st);
  if (v_re) transpose_out(h, dv.nrbuf, 1.0, erow, v_re, n, st);
  if (v_im) transpose_out(h, dv.nrbuf, 1.0, erow + n, v_im, n, st);
  if (vm) transpose_out(h, dv.nrbuf, 1.0, erow + 2 * n, vm, n, st);
  if (S) transpose_out(h, s.S, 1.0, iota, S, n * ns, st);
  if (g) transpose_out(h, s.g, 1.0, iota, g, ns, st);
  if (H) transpose_out(h, s.H, 1.0, iota, H, ns * ns, st);
  if (loss_mw) transpose_out(h, s.loss, dv.sn, iota, loss_mw, 1, st);
  if (violation) transpose_out(h, s.viol, 1.0, iota, violation, 1, st);
  if (d) transpose_out(h, s.qd, 1.0, iota, d, ns, st);
  if (y) transpose_out(h, s.qy, 1.0, iota, y, ns + n, st);
  if (linearised) launch_copy_u8(s.lin, linearised, dv.B, st);
  if (qp_capped) launch_copy_u8(s.qp_capped, qp_capped, dv.B, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
}

// ---- mapdn_evaluate_actions (whatif.hip): the workspace of the frame (the CtlLoop arrays, sized like droop's), once per handle.
// Nothing in it grows with the number of candidates: only the caller's outputs do.
static int whatif_prepare(mapdn_handle* h) {
  if (h->whatif_ready) return MAPDN_OK;
  WhatifState& s = h->whatif;
  const size_t Bp = h->d.Bp, ns = (size_t)h->plan.ns;
  int32_t *iters = nullptr, *nr_iters = nullptr, *n_active = nullptr; uint8_t *status = nullptr, *act = nullptr, *nr_conv = nullptr;
  int rc;
  if ((rc = dalloc(h, &s.a, ns * Bp)) || (rc = dalloc(h, &iters, Bp)) || (rc = dalloc(h, &nr_iters, Bp)) || (rc = dalloc(h, &status, Bp)) ||
      (rc = dalloc(h, &act, Bp)) || (rc = dalloc(h, &nr_conv, Bp)) || (rc = dalloc(h, &n_active, 1)))
    return rc;
  s.a_sol = nullptr; s.iters = iters; s.nr_iters = nr_iters; s.status = status; s.act = act; s.nr_conv = nr_conv; s.n_active = n_active;
  s.vm_row = h->vm_row; s.max_iter = 0;
  h->whatif_ready = true;
  return MAPDN_OK;
}

// The frame without a stop test, so without a poll: ctl_begin, then per candidate the start launch (the candidate's Sbus rows), the
// solve on the frame's active set, between(k) — what the caller reads off the solved candidate — and k_whatif_score.  Only enqueues.
// Writes what ctl_drive writes (the PV-bus and several-load-bus entries of the Sbus buffer the next solve reads, all of it when Sbus is
// stale; the solver's Vout rows) and the caller's outputs.  After whatif_prepare.
template <class Between>
static int whatif_drive(mapdn_handle* h, const void* actions, int dtype, int K, double* reward, double* info, uint8_t* status,
                        int32_t* iterations, double* vm_pu, hipStream_t st, Between between) {
  const Dev& d = h->d;
  WhatifState s = h->whatif;
  s.K = K; s.reward = reward; s.info = info; s.status_out = status; s.iters_out = iterations; s.vm_out = vm_pu;
  Dev dd;
  if (const int rc = ctl_begin(h, s, 0, st, &dd)) return rc;
  for (int k = 0; k < K; ++k) {
    launch_whatif_start(d, s, actions, dtype, k, st);
    nr_launch(h, MODE_SOLVE, nullptr, nullptr, nullptr, st, nullptr, 0, &dd);
    between(k);
    launch_whatif_score(d, s, k, st);
  }
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
}
static int whatif_run(mapdn_handle* h, const void* actions, int dtype, int K, double* reward, double* info, uint8_t* status,
                      int32_t* iterations, double* vm_pu, hipStream_t st) {
  if (const int rc = whatif_prepare(h)) return rc;
  return whatif_drive(h, actions, dtype, K, reward, info, status, iterations, vm_pu, st, [](int) {});
}

// ---- mapdn_action_gradients (grad.hip, grad.hpp; grad_sparse.hip): what the adjoint solve does not cover, by name.  grad_meshed = 1
// (mapdn_env_config) lets a k_nr_sparse handle answer by the elimination program on transposed blocks; 0 keeps the tree solver alone.
static bool grad_on_sparse(const mapdn_handle* h) { return h->knobs.grad_meshed == 1 && h->solver == 1; }
static const char* grad_refusal(const mapdn_handle* h) {
  const Plan& P = h->plan;
  if (const char* why = solver_gate(h, "action_gradients", "grad_meshed", h->knobs.grad_meshed == 1)) return why;
  if (P.zip) return "action_gradients: voltage-dependent (ZIP) loads are not supported";
  if (P.n_gen) return "action_gradients: nets with generators (net.gen, gen buses) are not supported (k_action_grad takes every non-slack bus as a PQ bus)";
  if (P.gen_start && grad_on_sparse(h))
    return "action_gradients: a start other than ext_grid_vm_pu (vm_init_pu: out-of-service net.gen rows) is not supported on the sparse solver";
  if (P.nbo != P.nb || !P.fused_obus.empty() || !P.alias_pos.empty()) return "action_gradients: fused buses are not supported";
  return nullptr;
}

// k_action_grad_sparse (grad_sparse.hip), once per handle: the node of every sgen and the transposed assembly stream beside Dev::sp_nz
// (plan.cpp grad_sparse_table).  No workspace: fac and lam stay unallocated, every block of an env lives in LDS.
static int grad_prepare_sparse(mapdn_handle* h) {
  int rc;
  if ((rc = whatif_prepare(h))) return rc;
  const Plan& P = h->plan;
  GradState& g = h->grad;
  GradSparseState& t = h->grad_sparse;
  std::vector<GsNz> nz;
  grad_sparse_table(P, h->sprog, nz, t.rows_per_sub, t.max_nnz);
  if ((rc = dupload(h, &g.sg_node, sgen_nodes(P))) || (rc = dupload(h, &t.nz, nz))) return rc;
  t.nz_bytes = (uint32_t)(nz.size() * sizeof(GsNz));
  if ((rc = sparse_prepared(h, grad_sparse_prepare(h->sp_lanes), "k_action_grad_sparse"))) return rc;
  g.act = h->whatif.act; g.nr_conv = h->whatif.nr_conv; g.a = h->whatif.a;
  h->grad_ready = true;
  return MAPDN_OK;
}

// the tree tables (opf_tables) and the workspace of k_action_grad, once per handle: the factors and lambda of ONE candidate, env-minor.
// Nothing in it grows with the number of candidates.
static int grad_prepare(mapdn_handle* h) {
  if (h->grad_ready) return MAPDN_OK;
  if (h->solver == 1) return grad_prepare_sparse(h);
  int rc;
  if ((rc = opf_tables(h)) || (rc = whatif_prepare(h))) return rc;
  GradState& g = h->grad;
  const size_t Bp = h->d.Bp, n = (size_t)h->plan.n;
  if ((rc = dalloc(h, &g.fac, n * OPF_FAC * Bp)) || (rc = dalloc(h, &g.lam, n * 2 * Bp))) return rc;
  const OpfState& o = h->opf;
  g.par = o.par; g.cptr = o.cptr; g.cidx = o.cidx; g.sg_node = o.sg_node; g.yt = o.yt;
  g.act = h->whatif.act; g.nr_conv = h->whatif.nr_conv; g.a = h->whatif.a;
  h->grad_ready = true;
  return MAPDN_OK;
}

// whatif_drive with k_action_grad (a k_nr_sparse handle: k_action_grad_sparse) between the solve and the scoring of every candidate.
// Only enqueues; writes what whatif_run writes, the gradient workspace and the caller's grad.
static int grad_run(mapdn_handle* h, const void* actions, int dtype, int K, double* grad, double* reward, double* info, uint8_t* status,
                    int32_t* iterations, double* vm_pu, hipStream_t st) {
  if (const int rc = grad_prepare(h)) return rc;
  const Dev& d = h->d;
  GradState g = h->grad;
  g.K = K; g.grad = grad;
  return whatif_drive(h, actions, dtype, K, reward, info, status, iterations, vm_pu, st, [&](int k) {
    if (h->solver == 1) launch_action_grad_sparse(d, g, h->grad_sparse, k, st);
    else launch_action_grad(d, g, k, st);
  });
}

// ---- mapdn_voltage_vjp (vjp.hip, vjp.hpp): grad_refusal's list under its own prefix.  The tree solver on a radial net answers; a handle
// of the sparse or of the dense solver is refused by name whatever grad_meshed says.
static const char* vjp_refusal(const mapdn_handle* h) {
  const Plan& P = h->plan;
  if (h->solver == 1)
    return "voltage_vjp: handles of the sparse solver (k_nr_sparse: meshed nets and radial ones pinned to it, with grad_meshed = 1 too) are not supported";
  if (h->solver != 0) return "voltage_vjp: handles of the dense solver (nr_solver = dense, k_nr_dense) are not supported";
  if (!P.radial) return "voltage_vjp: meshed nets are not supported";
  if (P.zip) return "voltage_vjp: voltage-dependent (ZIP) loads are not supported";
  if (P.n_gen) return "voltage_vjp: nets with generators (net.gen, gen buses: k_voltage_vjp takes every non-slack bus as a PQ bus) are not supported";
  if (P.nbo != P.nb || !P.fused_obus.empty() || !P.alias_pos.empty()) return "voltage_vjp: fused buses are not supported";
  return nullptr;
}

// whatif_drive with k_voltage_vjp between the solve and the scoring of every candidate (M = 0 and no angles wanted: nothing between
// them), on the tables and the workspace of grad_prepare: nothing grows with K or M.  The frame's reward and info are not written.
// Only enqueues; writes what whatif_run writes, the gradient workspace and the caller's outputs.
static int vjp_run(mapdn_handle* h, const void* actions, int dtype, int K, int M, const double* cot_vm, const double* cot_va, double* grad,
                   double* vm_pu, double* va_degree, uint8_t* status, int32_t* iterations, hipStream_t st) {
  if (const int rc = grad_prepare(h)) return rc;
  const Dev& d = h->d;
  const GradState g = h->grad;
  const VjpState v = {K, M, cot_vm, cot_va, grad, va_degree};
  const bool between = M > 0 || va_degree;
  if (const int rc = whatif_drive(h, actions, dtype, K, nullptr, nullptr, status, iterations, vm_pu, st, [&](int k) {
        if (between) launch_voltage_vjp(d, g, v, k, st);
      }))
    return rc;
  if (vm_pu) launch_vjp_mask(d, K, actions, dtype, status, vm_pu, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
}
