// capi.hip — C ABI of libmapdn_hip.so (declared in include/mapdn.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.hpp"
#include "ppo.hip"            // MAPPO / IPPO: the strided GAE and the clipped losses (k_ppo_*), compiled inside this unit; entry points below
#include "branch.hip"         // res_line / res_trafo: k_branch_results, k_loading_summary, compiled inside this unit like ppo.hip; entry points below
#include "nr_inst_list.hpp"
#include "colstats.hpp"
#include "opf.hpp"
#include "plan.hpp"

using namespace mapdn;

static constexpr size_t CU_LDS = 160 * 1024;    // LDS of one CU: what one workgroup of any NR kernel may use
static constexpr int DROOP_MAX_ITER_CAP = 10000;   // mapdn_droop_config.max_iter at most
static constexpr int OPF_MAX_ITER_CAP = 1000;      // mapdn_opf_config.max_iter at most

// ---- tuning knobs: a field of mapdn_env_config (0 = automatic), overridden by an environment variable when one is set (tools,
// A/B runs).  resolve_knobs reads them all once, at the top of mapdn_create, into the handle; nothing else reads the environment.
struct Knobs {
  int solver;                                    // nr_solver; MAPDN_NR_SPARSE=1 -> 1, MAPDN_NR_DENSE=1 -> 2
  int waves, lanes;                              // k_nr_tree geometry pins
  // tri-state residency / mode switches: 0 auto | 1 on | 2 off (nr_lean: 1 lean | 2 fat)
  int lean, h_lds, g_lds, rec_lds, flat_lds, line_lds, mm_pass, fuse_inject;
  int sp_lanes;
  int grad_meshed;                               // mapdn_action_gradients on k_nr_sparse handles: 0 refused (as before) | 1 answered
  bool inject_full, debug_geometry;
  double check_dx, check_quad;
};

static Knobs resolve_knobs(const mapdn_env_config& c) {
  auto num = [](int v, const char* env) { const char* s = getenv(env); return s ? atoi(s) : v; };
  auto tri = [](int v, const char* env) { const char* s = getenv(env); return s ? (atoi(s) ? 1 : 2) : v; };   // env NAME=1 on, NAME=0 off
  auto f64 = [](double v, const char* env, double dflt) { const char* s = getenv(env); return s ? atof(s) : (v != 0.0 ? v : dflt); };
  Knobs k;
  k.solver = num(0, "MAPDN_NR_DENSE") ? 2 : (num(0, "MAPDN_NR_SPARSE") ? 1 : c.nr_solver);
  k.waves = num(c.nr_waves, "MAPDN_NR_WAVES"); k.lanes = num(c.nr_lanes, "MAPDN_NR_LANES"); k.lean = tri(c.nr_lean, "MAPDN_NR_LEAN");
  k.h_lds = tri(c.nr_h_lds, "MAPDN_NR_H_LDS"); k.g_lds = tri(c.nr_g_lds, "MAPDN_NR_G_LDS"); k.rec_lds = tri(c.nr_rec_lds, "MAPDN_NR_REC_LDS");
  k.flat_lds = tri(c.nr_flat_lds, "MAPDN_NR_FLAT_LDS"); k.line_lds = tri(c.nr_line_lds, "MAPDN_NR_LINE_LDS");
  k.mm_pass = tri(c.nr_mm_pass, "MAPDN_NR_MM_PASS");
  k.fuse_inject = tri(c.fuse_inject, "MAPDN_FUSE_INJECT");
  k.sp_lanes = num(c.sp_lanes, "MAPDN_SP_LANES");
  k.grad_meshed = num(c.grad_meshed, "MAPDN_GRAD_MESHED");
  k.inject_full = num(c.inject_full, "MAPDN_INJECT_FULL") != 0;
  k.debug_geometry = num(c.debug_geometry, "MAPDN_DEBUG_GEOMETRY") != 0;
  // 1e-7: with quadratic convergence the mismatch after such a step is ~|Y| dx^2 << tol, so a wrong prediction
  // (which costs one extra mismatch-only sweep for that workgroup) practically never happens
  k.check_dx = f64(c.nr_check_dx, "MAPDN_NR_CHECK_DX", 1e-7);
  // quadratic extrapolation of the mismatch norm, no safety margin: in 4096-env samples of all three cases it
  // predicts the last sweep of 95-100 % of the workgroups and never a non-final one (tools/predictor_study.py)
  k.check_quad = f64(c.nr_check_quad, "MAPDN_NR_CHECK_QUAD", 1.0);
  return k;
}

struct mapdn_handle {
  Plan plan;
  Schedule sched;
  SparseProg sprog;
  Knobs knobs;
  int solver = 0;                 // 0 tree (radial), 1 general sparse (k_nr_sparse), 2 general dense (k_nr_dense)
  int sp_lanes = 0;
  int nr_var = 0;                 // k_nr_tree variant: NR_VAR_DC | NR_VAR_ZIP | NR_VAR_GEN
  mapdn_env_config cfg;
  Dev d;
  int device = 0;
  std::string err;
  std::vector<void*> allocs;
  bool have_profiles = false, was_reset = false, host_only = false;
  bool sbus_stale = true;         // Sbus / bus_ld do not reflect cur_pl / cur_ql (fresh handle, after mapdn_solve_only): the next
                                  // injection runs the all-bus kernel; knobs.inject_full keeps it that way (A/B, tests)
  bool fuse_inject = false;       // step(): the PV-bus injection runs in the prologue of k_nr_tree instead of as k_inject_sgen (tree solver, no auto_reset)
  size_t lds_bytes = 0;
  // what mapdn_create settled on (mapdn_get_nr_geometry); tree solver only: W .. mm_pass
  struct Geo { int W = 0, L = 0, lean = 0, rows = 0, h_lds = 0, g_lds = 0, rec_lds = 0, flat_lds = 0, line_lds = 0, mm_pass = 0, ncl = 0;
               size_t lds = 0; long wgs = 0; int resident = 0, rounds = 0; double model_ns = 0.0; } geo;
  int32_t *obs_rows = nullptr, *state_rows = nullptr, *iota_idx = nullptr, *vm_row = nullptr, *va_row = nullptr;
  int32_t *obs_xptr = nullptr, *obs_xrow = nullptr, *gen_bus_rows = nullptr;
  double *obs_scale = nullptr, *state_scale = nullptr, *gen_p_rows = nullptr;
  double *t_pl = nullptr, *t_ql = nullptr, *t_pv = nullptr, *t_q = nullptr;
  double* table = nullptr; double* stdv = nullptr; double* smax = nullptr;
  std::vector<double> stdv_host, smax_host;     // what set_profiles computed (mapdn_get_profile_stats)
  long long* stats_dev = nullptr;
  // NR kernel timing
  bool timing = false;
  std::vector<hipEvent_t> ev;   // pairs
  size_t ev_used = 0;
  double acc_ms = 0.0;
  int64_t acc_launches = 0;
  // droop baseline (mapdn_droop_actions): its workspace, allocated on the first call
  DroopState droop{};
  bool droop_ready = false;
  // OPF baseline (mapdn_opf_actions): likewise
  OpfState opf{};
  bool opf_ready = false, opf_tables_ready = false;
  OsM opf_m{};                                   // ... of k_opf_reduce_sparse (meshed = 1, k_nr_sparse handles): the rows of M
  // mapdn_evaluate_actions: the frame's workspace, likewise
  WhatifState whatif{};
  bool whatif_ready = false;
  // mapdn_action_gradients: the workspace of k_action_grad, likewise
  GradState grad{};
  bool grad_ready = false;
  GradSparseState grad_sparse{};                 // ... of k_action_grad_sparse (grad_meshed = 1, k_nr_sparse handles): the transposed assembly stream
  // res_line / res_trafo (mapdn_get_branch_results, mapdn_get_loading_summary): the plan's branch records with the ratings of
  // mapdn_set_branch_ratings folded in, and their device copy
  std::vector<BranchRec> branches;
  BranchRec* branches_dev = nullptr;
  double* opf_probe_a = nullptr;                 // mapdn_opf_probe: its set-points env-minor [ns][Bp], and the rows of its exports
  const int32_t* opf_probe_rows = nullptr;       // identity rows | the Re V, the Im V, the |V| row of every node
};

static std::string g_create_err;

// Nothing may leave an extern "C" entry point by exception: every one of them is a function-try-block ending in
// MAPDN_CATCH, which turns std::bad_alloc into MAPDN_E_NOMEM and anything else into MAPDN_E_INTERNAL, with the text in mapdn_last_error.
static int api_fail(const mapdn_handle* h, int code, const char* what) noexcept {
  try { (h ? const_cast<mapdn_handle*>(h)->err : g_create_err) = what; } catch (...) {}      // (the message itself may not fit any more)
  return code;
}
#define MAPDN_CATCH(h)                                                                                       \
  catch (const std::bad_alloc&) { return api_fail((h), MAPDN_E_NOMEM, "out of host memory (std::bad_alloc)"); } \
  catch (const std::exception& e) { return api_fail((h), MAPDN_E_INTERNAL, e.what()); }                      \
  catch (...) { return api_fail((h), MAPDN_E_INTERNAL, "unknown C++ exception"); }

#define NEEDDEV(h) do { if ((h)->host_only) { (h)->err = "host-only handle (device == -1): no device entry points"; return MAPDN_E_STATE; } } while (0)
#define HIPCHK(h, call)                                                                         \
  do {                                                                                          \
    hipError_t _e = (call);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(_e);                             \
      return MAPDN_E_HIP;                                                                       \
    }                                                                                           \
  } while (0)

template <typename T>
static int dalloc(mapdn_handle* h, T** p, size_t count) {
  void* q = nullptr;
  size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  HIPCHK(h, hipMalloc(&q, bytes));
  h->allocs.push_back(q);
  HIPCHK(h, hipMemset(q, 0, bytes));
  *p = (T*)q;
  return MAPDN_OK;
}

template <typename Q, typename T>                // Q: T or const T
static int dupload(mapdn_handle* h, Q** p, const std::vector<T>& v) {
  static_assert(std::is_same<std::remove_const_t<Q>, T>::value, "dupload: element type mismatch");
  T* q = nullptr;
  int rc = dalloc(h, &q, v.size());
  if (rc) return rc;
  if (!v.empty()) HIPCHK(h, hipMemcpy(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  *p = q;
  return MAPDN_OK;
}

// ---- k_nr_tree launch geometry.
// A workgroup = W waves serving L envs; each wave carries 64/L lane-group workers, so Wt = W*64/L workers eliminate independent
// subtrees of every env concurrently (schedule rows R(Wt) >= the radius of the feeder).  Small batches are latency-bound: spread
// each env over many workers and keep everything the solve touches in LDS ("fat", one workgroup per CU); batches that would need
// several ROUNDS of such workgroups take fewer workers / less LDS per env instead so that more envs are resident ("lean", or 16
// instead of 8 envs per workgroup on the 322-bus class).  The choice is the minimum of a launch-time model over the candidate
// (W, L, lean) triples, each with its own schedule and LDS residency settled first:
//     t = rounds x [ c0 + b n/Wt + row(W) R (1 + p [h not in LDS]) ] x load x share
//   rounds = ceil(workgroups / (CUs x resident));  resident = workgroups per CU by LDS (160 KB) and registers (one wave per SIMD:
//            every instantiation uses more than half of the register file)
//   row(W) = 2.37 / 2.90 / 3.00 us per schedule row (all sweeps of one solve together) with 1 / 2 / 4 waves: the row barrier
//            spans the workgroup;  c0 = 26 us, b = 0.36 us per node and worker (passes, epilogue)
//   load   = 1 + 0.21 [h not in LDS] x min(1, workgroups / CUs): factors through L2 / HBM slow down as the chip fills
//   share  = 1 + 0.5 x max(0, waves per SIMD - 1)
// Least-squares fit (relative error, 25 points, residuals <= 10 %, tools/nr_geometry_fit.py) to the launch times measured for
// case33 / case141 / case141_deep / case322 at 1024 ... 16384 envs in fat and lean layouts (profiles/r02_nr_geometry_case141.txt,
// profiles/r03_geometry_case322.txt, profiles/r03_final_*_kernel_stats.txt); it ranks every measured pair in the measured order.
// mapdn_env_config.nr_waves / nr_lanes / nr_lean pin a choice.
static double nr_model_ns(int W, int L, int n, int R, int h_lds, long wgs, int resident, int n_cu) {
  const double Wt = (double)W * (64 / L);
  const long per_round = (long)n_cu * std::max(resident, 1);
  const double rounds = (double)((wgs + per_round - 1) / per_round);
  const double row = W == 1 ? 2374.0 : (W == 2 ? 2903.0 : 3001.0);
  const double fill = (double)wgs / (double)n_cu;                           // workgroups per CU wanted
  const double conc = std::min((double)std::max(resident, 1), std::max(1.0, fill));   // ... sharing a CU
  const double base = 26032.0 + 363.0 * (double)n / Wt + row * (double)R * (h_lds ? 1.0 : 1.023);
  const double load = 1.0 + (h_lds ? 0.0 : 0.21) * std::min(1.0, fill);
  const double share = 1.0 + 0.5 * std::max(0.0, conc * W / 4.0 - 1.0);
  return rounds * base * load * share;
}

// Settles the k_nr_tree geometry of a handle: (W, L, lean) — pinned by the knobs or chosen by the model above — then the
// schedule for Wt workers and the LDS residents.  Works without a device (host-only handles assume n_cu CUs).
static int settle_tree_geometry(mapdn_handle* h, int Bp, int n_cu) {
  const Plan& P = h->plan;
  const Knobs& k = h->knobs;
  if (P.n + 1 > 0xffff) { h->err = "networks with more than 65534 buses are not supported (16-bit node positions in the NR step records)"; return MAPDN_E_INVALID; }
  auto tri = [](int forced, bool dflt) { return forced == 1 ? 1 : (forced == 2 ? 0 : (dflt ? 1 : 0)); };
  // Optional LDS residents, in order of benefit: the h factors, the step records, the flat-start constants, the net.line
  // constants of the fused res_line epilogue, then the G factors (with everything resident the solve state never leaves
  // the chip; what does not fit stays in / goes to L2-resident global memory).  In lean mode only the voltages and hand-off
  // slots are resident, so that several workgroups share a CU.
  // The kernel peels the first rows of its full sweeps (their G — and h, when h is not in LDS — stay in registers): a schedule
  // shorter than that is rebuilt with idle rows appended; one that needs no peeled rows (G in LDS) is left alone.
  auto settle = [&](int W, int L, int lean, Schedule& S, mapdn_handle::Geo& g) -> int {   // 0 ok, 1 does not fit / not compiled, <0 error
    const int Wt = W * (64 / L);
    int min_rows = 0;
    for (int pass = 0; pass < 4; ++pass) {
      build_schedule(P, Wt, S, nr_min_cslots(W, L), 64 / L, min_rows);
      if (S.n_cslots > 1023 || S.n_xslots > 1023) { h->err = "NR schedule needs more than 1023 LDS slots"; return MAPDN_E_INVALID; }
      g.ncl = (int)S.clist.size();
      if (g.ncl > 4095) { h->err = "NR schedule: more than 4095 overflow children (junctions with > 3 non-chain children)"; return MAPDN_E_INVALID; }
      if ((long)S.R * Wt > 0xffff) { h->err = "NR schedule has more than 65535 steps"; return MAPDN_E_INVALID; }
      const int R_ = S.R;
      auto lds_for = [&](int hl, int gl, int ll, int rl, int fl) {
        return nr_lds_bytes(W, L, P.n, S.n_cslots, S.n_xslots, g.ncl, hl, gl, ll ? P.n_line : 0, rl ? R_ : 0, fl ? R_ : 0); };
      g.h_lds = tri(k.h_lds, !lean && lds_for(1, 0, 0, 0, 0) <= CU_LDS);
      g.rec_lds = tri(k.rec_lds, !lean && lds_for(g.h_lds, 0, 0, 1, 0) <= CU_LDS);
      g.flat_lds = tri(k.flat_lds, !lean && lds_for(g.h_lds, 0, 0, g.rec_lds, 1) <= CU_LDS);
      g.line_lds = (tri(k.line_lds, !lean && P.n_line > 0 && lds_for(g.h_lds, 0, 1, g.rec_lds, g.flat_lds) <= CU_LDS) && P.n_line > 0) ? 1 : 0;
      g.g_lds = (tri(k.g_lds, !lean && g.h_lds && lds_for(1, 1, g.line_lds, g.rec_lds, g.flat_lds) <= CU_LDS) && g.h_lds) ? 1 : 0;
      g.lds = lds_for(g.h_lds, g.g_lds, g.line_lds, g.rec_lds, g.flat_lds);
      if (g.lds > CU_LDS) return 1;
      const int need = g.g_lds ? 0 : (g.h_lds ? NR_G_REG_ROWS : NR_HG_REG_ROWS);
      if (R_ >= need) { min_rows = -1; break; }
      min_rows = need;
    }
    if (min_rows >= 0) { h->err = "NR schedule: could not settle the number of peeled rows"; return MAPDN_E_INVALID; }
    const int compiled = nr_geometry_compiled(W, L, g.h_lds, g.g_lds, g.rec_lds, g.flat_lds, h->nr_var);
    if (!compiled) return 1;
    g.W = W; g.L = L; g.lean = lean; g.rows = S.R;
    g.wgs = Bp / L;
    // workgroups resident per CU: LDS, and the register file — every k_nr_tree instantiation keeps factors of its peeled rows in
    // AGPRs and uses 284 ... 452 of a SIMD's 512 registers per lane: one wave per SIMD, i.e. 4 / W workgroups per CU
    g.resident = (int)std::max<size_t>(1, std::min<size_t>(CU_LDS / std::max<size_t>(g.lds, 1), (size_t)std::max(4 / W, 1)));
    const long per_round = (long)n_cu * g.resident;
    g.rounds = (int)((g.wgs + per_round - 1) / per_round);
    g.model_ns = nr_model_ns(W, L, P.n, S.R, g.h_lds, g.wgs, g.resident, n_cu) * (compiled == 2 ? 1.0 : 1.05);   // generic body: the
                                                                   // per-row residency branches cost ~6 %
    return 0;
  };
  const int W = k.waves, L = k.lanes, lean_k = k.lean;          // lean_k: 0 auto, 1 lean, 2 fat
  if ((W != 0 && W != 1 && W != 2 && W != 4 && W != 8) || (L != 0 && L != 4 && L != 8 && L != 16 && L != 32)) {
    h->err = "nr_waves (MAPDN_NR_WAVES) must be 1/2/4/8 and nr_lanes (MAPDN_NR_LANES) 4/8/16/32 (0 = automatic)"; return MAPDN_E_INVALID; }
  mapdn_handle::Geo best; Schedule bestS; bool have = false;
  const bool forced = W != 0 && L != 0 && lean_k != 0;
  // automatic candidates: the pairs the model was fitted on; the other compiled pairs (nr_inst_list.hpp) only when pinned
  static const int cand[][2] = {{1, 16}, {2, 16}, {4, 16}, {4, 8}};
  for (const auto& wl : cand) {
    if ((W && wl[0] != W) || (L && wl[1] != L)) continue;
    for (int lean = 0; lean < 2; ++lean) {
      if ((lean_k == 1 && !lean) || (lean_k == 2 && lean)) continue;
      mapdn_handle::Geo g; Schedule S;
      const int r = settle(wl[0], wl[1], lean, S, g);
      if (r < 0) return r;
      if (r > 0) continue;
      if (!have || g.model_ns < best.model_ns) { best = g; bestS = std::move(S); have = true; }
    }
  }
  if (!have && W && L) {          // a pinned pair outside the candidate list (e.g. tests): no model, just settle it
    mapdn_handle::Geo g; Schedule S;
    const int r = settle(W, L, lean_k == 1 ? 1 : 0, S, g);
    if (r < 0) return r;
    if (r == 0) { best = g; bestS = std::move(S); have = true; }
    else if (g.lds > CU_LDS) { h->err = "NR schedule needs more LDS than one CU has (160 KB); use fewer envs per workgroup (nr_lanes / MAPDN_NR_LANES) or fewer waves"; return MAPDN_E_INVALID; }
  }
  if (!have) {
    h->err = (W || L) ? "this (nr_waves, nr_lanes) combination is not compiled in or does not fit the 160 KB LDS of a CU (csrc/nr_inst_list.hpp)"
                      : "no compiled k_nr_tree geometry fits this network into the 160 KB LDS of a CU";
    return MAPDN_E_INVALID; }
  if (forced) best.model_ns = 0.0;
  best.mm_pass = (best.h_lds && k.mm_pass != 2) ? 1 : 0;    // the pass needs the h array in LDS
  h->geo = best; h->sched = std::move(bestS); h->lds_bytes = best.lds;
  if (k.debug_geometry)
    fprintf(stderr, "[mapdn] k_nr_tree geometry: W %d L %d lean %d rows %d cslots %d | LDS: h %d rec %d flat %d line %d G %d = %zu B | "
                    "%ld workgroups, %d per CU, %d round(s), model %.1f us\n",
            best.W, best.L, best.lean, best.rows, h->sched.n_cslots, best.h_lds, best.rec_lds, best.flat_lds, best.line_lds, best.g_lds,
            best.lds, best.wgs, best.resident, best.rounds, best.model_ns * 1e-3);
  return MAPDN_OK;
}

// ---- mapdn_create, stage by stage: create_impl below calls them in order.

// Solver choice.  pp.runpp (voltage_control_env.py:557) solves any connected net: radial feeders take the fill-free
// tree kernel; meshed nets the general sparse kernel (host symbolic factorisation with fill + a block program, all
// blocks of L envs in LDS); MAPDN_NR_DENSE=1 selects the dense LDS-resident LU with f64 MFMA (<= 65 buses),
// MAPDN_NR_SPARSE=1 the sparse kernel on a radial net (cross-checks).
static int choose_solver(mapdn_handle* h) {
  const Plan& P = h->plan;
  const int pick = h->knobs.solver;
  if (pick < 0 || pick > 2) { h->err = "nr_solver must be 0 (auto), 1 (sparse) or 2 (dense)"; return MAPDN_E_INVALID; }
  if (pick == 2) {
    if (2 * P.n > 1024) { h->err = "nr_solver = dense (MAPDN_NR_DENSE): the dense general-topology solver handles at most 513 buses (one thread per Jacobian row)"; return MAPDN_E_TOPOLOGY; }
    h->solver = 2;
  } else if (pick == 1 || !P.radial) {
    SparseProg g0;
    sparse_symbolic(P, g0);
    int Lc = 0;
    for (int l : {16, 8, 4, 2}) if (nr_sparse_lds_bytes(P.n, g0.n_blocks, l) <= CU_LDS) { Lc = l; break; }
    if (!Lc) {
      h->err = "topology: meshed network with " + std::to_string(P.nb) + " buses needs " + std::to_string(g0.n_blocks) +
               " Jacobian blocks after fill; two envs of it do not fit the 160 KB LDS of a CU";
      return MAPDN_E_TOPOLOGY; }
    h->solver = 1; h->sp_lanes = Lc;
  }
  return MAPDN_OK;
}

// Every refusal of a config that build_plan and the solver choice accepted, for host-only and device handles alike (mapdn.h: a
// pinned switch that cannot take effect is MAPDN_E_INVALID, never silently ignored).
static int validate(mapdn_handle* h, const mapdn_env_config& c) {
  const Plan& P = h->plan;
  const Knobs& k = h->knobs;
  if (c.nr_init == 1)   // reserved: see include/mapdn.h (the gating study found the warm start safe but without effect on the launch time)
    return api_fail(h, MAPDN_E_INVALID, "nr_init != 0 (warm start, runpp init=\"results\") is not built: tools/warm_start_study.py / "
                                        "profiles/r04_warm_start_study_*.json show no iteration saved per 16-env workgroup; every solve "
                                        "starts flat like the reference's");
  if (c.nr_init != 0 && c.nr_init != 2) return api_fail(h, MAPDN_E_INVALID, "nr_init must be 0 (flat start) or 2 (runpp init=\"dc\"); 1 (init=\"results\") is reserved");
  if (c.nr_init == 2 && !P.dc_ok)
    return api_fail(h, MAPDN_E_INVALID, !P.fused_obus.empty()
                        ? "nr_init = 2 (runpp init=\"dc\") on a net with fused buses (bus_alias) is not supported (the DC-angle start is defined on unfused nets only)"
                        : "nr_init = 2 (runpp init=\"dc\"): the DC power flow matrix Bbus of this net is singular or not finite (a branch with x = 0?)");
  if (h->solver == 2 && c.nr_init == 2)
    return api_fail(h, MAPDN_E_INVALID, "nr_init = 2 (runpp init=\"dc\") is not built for nr_solver = dense (k_nr_dense starts flat only): use the tree or the sparse solver");
  if (h->solver == 2 && P.zip)
    return api_fail(h, MAPDN_E_INVALID, "voltage-dependent loads (load_const_z / load_const_i) are not built for nr_solver = dense (k_nr_dense solves "
                                        "constant-power loads only): use the tree or the sparse solver");
  if (h->solver == 2 && P.gen_start)
    return api_fail(h, MAPDN_E_INVALID, P.n_gen ? "generators (net.gen, gen buses) are not built for nr_solver = dense (k_nr_dense solves PQ buses from the "
                                                  "flat start only): use the tree or the sparse solver"
                                                : "vm_init_pu other than ext_grid_vm_pu (out-of-service net.gen rows move runpp's start) is not built for "
                                                  "nr_solver = dense (k_nr_dense starts every bus at the ext_grid set-point): use the tree or the sparse solver");
  if (c.overlap_advance) return api_fail(h, MAPDN_E_INVALID, "overlap_advance was removed (measured slower than the single stream): it must be 0");
  if (c.xcd_map) return api_fail(h, MAPDN_E_INVALID, "xcd_map was removed (the XCD-aligned env order measured a wash): it must be 0");
  if (k.fuse_inject == 1 && h->solver != 0)
    return api_fail(h, MAPDN_E_INVALID, "fuse_inject = 1 exists on the tree solver only (this handle runs the general sparse / dense solver)");
  if (k.fuse_inject == 1 && (c.auto_reset || k.inject_full))
    return api_fail(h, MAPDN_E_INVALID, "fuse_inject = 1 needs a handle without auto_reset and without inject_full");
  if (k.grad_meshed != 0 && k.grad_meshed != 1)
    return api_fail(h, MAPDN_E_INVALID, "grad_meshed (MAPDN_GRAD_MESHED) must be 0 (action_gradients on the tree solver only) or 1 (also on the sparse solver)");
  if (h->solver == 1 && k.sp_lanes != 0 && k.sp_lanes != 16 && k.sp_lanes != 8 && k.sp_lanes != 4 && k.sp_lanes != 2)
    return api_fail(h, MAPDN_E_INVALID, "sp_lanes (MAPDN_SP_LANES) must be 16, 8, 4 or 2 (0 = automatic)");
  return MAPDN_OK;
}

// The host part of the general solvers' set-up, for host-only and device handles alike (no device calls): k_nr_sparse's envs per
// workgroup and its elimination program, k_nr_dense's Jacobian order.  What it settles is what mapdn_get_nr_kernel reports.
static int settle_general_solver(mapdn_handle* h) {
  const Plan& P = h->plan;
  Dev& d = h->d;
  if (h->solver == 2) {
    d.dn_N = (2 * P.n + 15) / 16 * 16; d.dn_lda = d.dn_N + 2;
    h->lds_bytes = nr_dense_lds_bytes(d.dn_N, d.dn_lda, P.n);   // (setup_dense finds the same once the slab exists)
    return MAPDN_OK;
  }
  if (h->solver != 1) return MAPDN_OK;
  if (h->knobs.sp_lanes) h->sp_lanes = h->knobs.sp_lanes;      // pinned envs per workgroup (16 / 8 / 4 / 2)
  else {
    // Envs per (one-wave) workgroup: fewer envs = more sub-lanes per env = fewer phases, and a smaller LDS tile = more
    // resident waves per CU to hide each other's LDS latency.  Score = envs in flight per CU / length of the per-iteration
    // instruction stream (phases + assembly entries); measured on case33 / case141 / case322 with tie lines closed
    // (profiles/r02_sparse_lanes_sweep.txt): the score ranks the four geometries in the measured order.
    double best = -1.0;
    for (int l : {16, 8, 4, 2}) {
      SparseProg g;
      sparse_program(P, 64 / l, g);
      const size_t lds = nr_sparse_lds_bytes(P.n, g.n_blocks, l);
      if (lds > CU_LDS) continue;
      const double waves = (double)std::min<size_t>(CU_LDS / lds, 8);
      const double score = waves * l / ((double)g.n_phases + 0.5 * g.rows_per_sub * g.max_nnz);
      if (score > best) { best = score; h->sp_lanes = l; }
    }
  }
  sparse_program(P, 64 / h->sp_lanes, h->sprog);
  h->lds_bytes = nr_sparse_lds_bytes(P.n, h->sprog.n_blocks, h->sp_lanes);
  if (h->lds_bytes > CU_LDS) { h->err = "sp_lanes (MAPDN_SP_LANES): does not fit in LDS"; return MAPDN_E_INVALID; }
  return MAPDN_OK;
}

#define UP(field, vec) do { if (const int rc_ = dupload(h, &d.field, vec)) return rc_; } while (0)
#define AL(field, rows) do { if (const int rc_ = dalloc(h, &d.field, (size_t)(rows) * d.Bp)) return rc_; } while (0)

// the scalars of Dev and the topology plan
static int upload_topology(mapdn_handle* h) {
  const Plan& P = h->plan;
  const mapdn_env_config& c = h->cfg;
  Dev& d = h->d;
  d.nb = P.nb; d.n = P.n; d.nl = P.nl; d.ns = P.ns; d.n_line = P.n_line;
  d.nbo = P.nbo;                                 // original buses (> nb with fused buses): the rows of res_bus / obs / state
  d.ncol = P.ns + 2 * P.nl;
  d.vroot = P.vroot; d.sn = P.sn_mva; d.tol = P.tol; d.max_it = 10;   // runpp max_iteration="auto" -> 10
  d.yrr0 = P.yrr[0]; d.yrr1 = P.yrr[1];
  d.barrier_type = c.barrier_type; d.use_line_weight = c.use_line_weight; d.episode_limit = c.episode_limit;
  d.reset_action = c.reset_action; d.auto_reset = c.auto_reset ? 1 : 0; d.voltage_weight = c.voltage_weight; d.q_weight = c.q_weight;
  d.line_weight = c.line_weight; d.v_lower = c.v_lower; d.v_upper = c.v_upper;
  d.action_low = c.action_low; d.action_high = c.action_high;
  d.seed_lo = (uint32_t)(c.seed & 0xffffffffull); d.seed_hi = (uint32_t)(c.seed >> 32);
  d.env_id_offset = c.env_id_offset;
  d.nr_init = c.nr_init;
  if (d.nr_init == 2) UP(dc_pc, P.dc_pc);
  d.zip = P.zip ? 1 : 0;
  if (d.zip) { UP(zip_c, P.zip_c); d.zip_c_bytes = (uint32_t)(P.zip_c.size() * sizeof(double)); }
  d.n_gen = P.n_gen; d.gen_start = P.gen_start ? 1 : 0;
  if (d.gen_start) {                              // generators: plan.hpp Plan::n_gen ...
    UP(is_gen, P.is_gen); UP(gen_p_pos, P.gen_p_pos); UP(v0, P.v0); d.v0_bytes = (uint32_t)(P.v0.size() * sizeof(double));
    UP(gen_of_pos, P.gen_of_pos); UP(gq_ptr, P.gq_ptr);
    { std::vector<int32_t> gc(P.gq_col); if (gc.empty()) gc.push_back(0); UP(gq_col, gc); }
    { std::vector<double> gv(P.gq_val); if (gv.empty()) gv.push_back(0.0); UP(gq_val, gv); }
  }
  UP(bus_of_pos, P.bus_of_pos); UP(root_children, P.root_children); UP(root_y, P.root_y);
  UP(pos_of_obus, P.pos_of_obus); UP(cm_kind, P.cm_kind);
  d.n_fused = (int32_t)P.fused_obus.size(); d.n_alias = (int32_t)P.alias_pos.size(); d.n_slack_group = (int32_t)P.slack_group.size();
  if (d.n_fused) {
    UP(fused_obus, P.fused_obus); UP(ob_load_ptr, P.ob_load_ptr); UP(ob_load_idx, P.ob_load_idx); UP(ob_sgen_ptr, P.ob_sgen_ptr);
    UP(ob_sgen_idx, P.ob_sgen_idx); UP(ob_shunt_p, P.ob_shunt_p); UP(ob_shunt_q, P.ob_shunt_q);
    { std::vector<int32_t> sg(P.slack_group); if (sg.empty()) sg.push_back(0); UP(slack_group, sg); }
    { std::vector<int32_t> ap(P.alias_pos); if (ap.empty()) ap.push_back(0); UP(alias_pos, ap); }
  }
  d.n_root_children = (int32_t)P.root_children.size();
  UP(load_ptr, P.load_ptr); UP(load_idx, P.load_idx); UP(sgen_ptr, P.sgen_ptr); UP(sgen_idx, P.sgen_idx);
  UP(shunt_p, P.shunt_p); UP(shunt_q, P.shunt_q); UP(load_scale, P.load_scale); UP(sgen_scale, P.sgen_scale);
  std::vector<LineFlow> padded(P.lines);         // read 16 bytes at a time by the NR kernel's LDS staging
  if (padded.size() % 2) padded.push_back(LineFlow{});
  UP(lines, padded);
  return MAPDN_OK;
}

// The tables of the step()/reset() injection: buses with sgens (PV buses), load-only buses, load-only buses with several loads, the
// 16-byte records of the fused prologue of k_nr_tree, and where k_advance puts a load that is alone on its bus (ld_dest).
static int setup_pv_buses(mapdn_handle* h) {
  const Plan& P = h->plan;
  Dev& d = h->d;
  std::vector<int32_t> sgb, sgb_of(P.nb, -1), lb, mlo;
  for (int k = 0; k < P.nb; ++k) {
    if (P.sgen_ptr[k + 1] > P.sgen_ptr[k]) { sgb_of[k] = (int32_t)sgb.size(); sgb.push_back(k); }
    else if (P.load_ptr[k + 1] > P.load_ptr[k]) {
      lb.push_back(k);
      if (P.load_ptr[k + 1] - P.load_ptr[k] > 1 && k < P.n) mlo.push_back(k);
    }
  }
  d.n_sgb = (int32_t)sgb.size(); d.n_lb = (int32_t)lb.size(); d.n_mlo = (int32_t)mlo.size();
  if (lb.empty()) lb.push_back(0);
  if (mlo.empty()) mlo.push_back(0);
  {   // per (PV bus | load-only bus with several loads) row of the injection: what the fused prologue of k_nr_tree needs in one 16-byte load
    std::vector<int32_t> rec;
    auto put = [&](int k, bool pv) {
      const int nsg = pv ? P.sgen_ptr[k + 1] - P.sgen_ptr[k] : 0, nld = P.load_ptr[k + 1] - P.load_ptr[k];
      rec.push_back(k < P.n ? k : -1);            // Sbus is stored by node position
      rec.push_back(k);
      rec.push_back(pv ? P.sgen_idx[P.sgen_ptr[k]] : -1);
      rec.push_back((nsg << 8) | std::min(nld, 2));
      rec.push_back(nld > 0 ? P.load_idx[P.load_ptr[k]] : -1);        // the first two loads of the bus (CSR order)
      rec.push_back(nld > 1 ? P.load_idx[P.load_ptr[k] + 1] : -1);
      rec.push_back(0); rec.push_back(0);
    };
    for (int i = 0; i < d.n_sgb; ++i) put(sgb[i], true);
    for (int i = 0; i < d.n_mlo; ++i) put(mlo[i], false);
    UP(sgb_rec, rec);
  }
  UP(sgb_pos, sgb); UP(sgb_of_pos, sgb_of); UP(lb_pos, lb); UP(mlo_pos, mlo);
  // ld_dest: a load alone on its bus goes straight to the Sbus entry (kind 0) / bus_ld row (kind 1) of that bus; 2: neither
  std::vector<int32_t> ld_dest(std::max(P.nl, 1), 2);
  for (int k = 0; k < P.nb; ++k) {
    if (P.load_ptr[k + 1] - P.load_ptr[k] != 1) continue;
    const int li = P.load_idx[P.load_ptr[k]];
    if (sgb_of[k] >= 0) ld_dest[li] = (sgb_of[k] << 2) | 1;
    else if (k < P.n) ld_dest[li] = (k << 2) | 0;
  }
  UP(ld_dest, ld_dest);
  return dalloc(h, &d.bus_ld, (size_t)2 * d.n_sgb * d.Bp);
}

// gatherable state block gbuf (rows of Bp doubles): cur_pv cur_q [ns] | vm va res_p res_q [nbo]
struct GbufRows { int pv, q, vm, va, rp, rq, n; };
static GbufRows gbuf_rows(const Dev& d) {
  const int vm = 2 * d.ns;
  return {0, d.ns, vm, vm + d.nbo, vm + 2 * d.nbo, vm + 3 * d.nbo, vm + 4 * d.nbo};
}

// env state: element tables, gbuf, per-env bookkeeping, the staging of mapdn_solve_only and mapdn_stats
static int setup_env_state(mapdn_handle* h) {
  Dev& d = h->d;
  const size_t Bp = d.Bp;
  AL(q_new, d.ns); AL(cur_pl, d.nl); AL(cur_ql, d.nl); AL(pl, d.n_line);
  if (d.n_gen) {
    AL(res_gen_q, d.n_gen);
    std::vector<double> gp((size_t)d.n_gen * Bp);                // res_gen.p_mw, env-minor like every result row: the same constant per env
    for (int g = 0; g < d.n_gen; ++g) std::fill_n(gp.begin() + (size_t)g * Bp, Bp, h->plan.gen_p[g]);
    if (const int rc_ = dupload(h, &h->gen_p_rows, gp)) return rc_;
  }
  const GbufRows r = gbuf_rows(d);
  AL(gbuf, r.n);
  d.cur_pv = d.gbuf + (size_t)r.pv * Bp;
  d.cur_q = d.gbuf + (size_t)r.q * Bp; d.vm = d.gbuf + (size_t)r.vm * Bp; d.va = d.gbuf + (size_t)r.va * Bp;
  d.res_p = d.gbuf + (size_t)r.rp * Bp; d.res_q = d.gbuf + (size_t)r.rq * Bp;
  AL(sum_rewards, 1); AL(steps, 1); AL(start_row, 1); AL(draw, 1); AL(done, 1); AL(pending, 1);
  AL(active, 1); AL(commit, 1); AL(bad_start, 1); AL(resetting, 1); AL(adv_row, 1); AL(adv_draw, 1); AL(iters, 1); AL(conv, 1);
  std::vector<uint8_t> ones(Bp, 1);
  HIPCHK(h, hipMemcpy(d.done, ones.data(), Bp, hipMemcpyHostToDevice));   // nothing is steppable before reset
  int rc;
  if ((rc = dalloc(h, &h->t_pl, (size_t)d.nl * Bp)) || (rc = dalloc(h, &h->t_ql, (size_t)d.nl * Bp)) ||
      (rc = dalloc(h, &h->t_pv, (size_t)d.ns * Bp)) || (rc = dalloc(h, &h->t_q, (size_t)d.ns * Bp)))
    return rc;
  return dalloc(h, &h->stats_dev, 4);
}

// obs / state columns -> (source row of gbuf, scale, extra rows to add); -1 = zero padding.  P/Q columns with the effective PV
// add-back (voltage_control_env.py:238-244) = res_bus row + the sgen.p_mw / q_mvar rows of the sgens on that bus.
static int setup_gather_tables(mapdn_handle* h) {
  const Plan& P = h->plan;
  const Dev& d = h->d;
  const GbufRows g = gbuf_rows(d);
  std::vector<std::vector<int>> sgens_at(P.nbo);
  for (int j = 0; j < P.ns; ++j) sgens_at[P.sgen_bus[j]].push_back(j);
  auto tables = [&](const std::vector<int32_t>& kind, const std::vector<int32_t>& idx, std::vector<int32_t>& rows,
                    std::vector<double>& scale, std::vector<int32_t>& xptr, std::vector<int32_t>& xrow) {
    rows.resize(kind.size()); scale.assign(kind.size(), 1.0); xptr.assign(kind.size() + 1, 0); xrow.clear();
    for (size_t c = 0; c < kind.size(); ++c) {
      switch (kind[c]) {
        case G_P_ADDBACK: rows[c] = g.rp + idx[c]; for (int j : sgens_at[idx[c]]) xrow.push_back(g.pv + j); break;
        case G_Q_ADDBACK: rows[c] = g.rq + idx[c]; for (int j : sgens_at[idx[c]]) xrow.push_back(g.q + j); break;
        case G_SGEN_P: rows[c] = g.pv + idx[c]; break;
        case G_SGEN_Q: rows[c] = g.q + idx[c]; break;
        case G_VM: rows[c] = g.vm + idx[c]; break;
        case G_VA_RAD: rows[c] = g.va + idx[c]; break;
        case G_P: rows[c] = g.rp + idx[c]; break;
        case G_Q: rows[c] = g.rq + idx[c]; break;
        case G_VA_DEG: rows[c] = g.va + idx[c]; scale[c] = 180.0 / M_PI; break;
        default: rows[c] = -1; break;
      }
      xptr[c + 1] = (int32_t)xrow.size();
      if (xptr[c + 1] > xptr[c]) rows[c] |= 0x40000000;   // GATHER_HAS_EXTRA
    }
    if (xrow.empty()) xrow.push_back(0);
  };
  std::vector<int32_t> rows, xptr, xrow; std::vector<double> scale;
  int rc;
  tables(P.obs_kind, P.obs_idx, rows, scale, xptr, xrow);
  if ((rc = dupload(h, &h->obs_rows, rows)) || (rc = dupload(h, &h->obs_scale, scale)) || (rc = dupload(h, &h->obs_xptr, xptr)) ||
      (rc = dupload(h, &h->obs_xrow, xrow)))
    return rc;
  tables(P.state_kind, P.state_idx, rows, scale, xptr, xrow);     // get_state has no add-back
  if ((rc = dupload(h, &h->state_rows, rows)) || (rc = dupload(h, &h->state_scale, scale))) return rc;
  std::vector<int32_t> io(std::max(std::max(std::max(d.nbo, d.n_line), std::max(d.nl, d.ns)), d.n_gen));   // identity rows of the result exports
  for (size_t i = 0; i < io.size(); ++i) io[i] = (int32_t)i;
  if (d.n_gen) {                                 // res_gen vm_pu / va_degree: the res_bus rows of the gens' buses (no fused buses with generators)
    std::vector<int32_t> gb(P.n_gen);
    for (int g = 0; g < P.n_gen; ++g) gb[g] = P.bus_of_pos[P.gen_pos[g]];
    if ((rc = dupload(h, &h->gen_bus_rows, gb))) return rc;
  }
  return dupload(h, &h->iota_idx, io);
}

// NR scratch `nrbuf` (kernels.hpp): factor blocks (fb_rows pair rows) | 2 x Sbus (nblk pair rows each, entry k for position k) | Vout;
// a single buffer resource addresses it.  Also the rows of |V| / angle in Vout that mapdn_solve_only exports.
static int alloc_nrbuf(mapdn_handle* h, size_t fb_rows, size_t nblk) {
  const Plan& P = h->plan;
  Dev& d = h->d;
  const size_t Bp = d.Bp;
  const size_t sb_off = fb_rows * Bp * 16;
  const size_t vout_off = sb_off + 2 * nblk * Bp * 16;        // two Sbus buffers
  const size_t bytes = vout_off + (size_t)VOF * (P.n + 1) * Bp * sizeof(double);
  if (bytes >= (size_t)0xFFFFFFFFu) { h->err = "env batch too large: NR scratch exceeds the 4 GiB one buffer resource addresses; use fewer envs per handle"; return MAPDN_E_INVALID; }
  if (const int rc = dalloc(h, &d.nrbuf, bytes / sizeof(double))) return rc;
  d.nrbuf_bytes = (uint32_t)bytes;
  d.sb_off = (uint32_t)sb_off; d.sb_off_alt = (uint32_t)(sb_off + nblk * Bp * 16);
  d.r_vout = (uint32_t)(vout_off / (Bp * sizeof(double)));
  std::vector<double> row(Bp, d.vroot);   // slack entry of Vout: V = vroot + 0j (angle 0 from the memset)
  double* rootv = d.nrbuf + ((size_t)d.r_vout + (size_t)VOF * P.n) * Bp;
  HIPCHK(h, hipMemcpy(rootv + (size_t)VO_E * Bp, row.data(), Bp * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(rootv + (size_t)VO_VM * Bp, row.data(), Bp * sizeof(double), hipMemcpyHostToDevice));
  std::vector<int32_t> vmrow(P.nbo), varow(P.nbo);
  for (int b = 0; b < P.nbo; ++b) { const int k = P.pos_of_obus[b]; vmrow[b] = (int)d.r_vout + VOF * k + VO_VM; varow[b] = (int)d.r_vout + VOF * k + VO_VA; }
  int rc;
  if ((rc = dupload(h, &h->vm_row, vmrow)) || (rc = dupload(h, &h->va_row, varow))) return rc;
  return MAPDN_OK;
}

// k_nr_dense (dense.hip): one env per workgroup, dense Jacobian in LDS, f64 MFMA
static int setup_dense(mapdn_handle* h) {
  const Plan& P = h->plan;
  Dev& d = h->d;
  d.dense = 1;                                   // (dn_N, dn_lda: settle_general_solver)
  if (nr_dense_ga(d.dn_N)) {                     // beyond 65 buses the Jacobian of every env lives in a slab of global memory
    const size_t per_env = (size_t)d.dn_N * d.dn_lda;
    if (const int rc = dalloc(h, &d.dn_A, per_env * d.Bp)) return rc;
  }
  UP(gy_ptr, P.gy_ptr); UP(gy_col, P.gy_col); UP(gy_val, P.gy_val);
  if (const int rc = alloc_nrbuf(h, 0, (size_t)P.n)) return rc;
  if (nr_dense_prepare(d) != 0) { (void)hipGetLastError(); h->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for k_nr_dense"; return MAPDN_E_HIP; }
  h->lds_bytes = nr_dense_lds_bytes(d);
  return MAPDN_OK;
}

// k_nr_sparse (sparse.hip): host-compiled block elimination program (settle_general_solver)
static int setup_sparse(mapdn_handle* h) {
  const Plan& P = h->plan;
  Dev& d = h->d;
  const SparseProg& G = h->sprog;
  d.sparse = 1; d.sp_lanes = h->sp_lanes; d.sp_blocks = G.n_blocks; d.sp_fill = (int32_t)G.fill_slots.size();
  d.sp_phases = G.n_phases; d.sp_rows_per_sub = G.rows_per_sub; d.sp_max_nnz = G.max_nnz;
  UP(sp_ops, G.ops); d.sp_ops_bytes = (uint32_t)(G.ops.size() * sizeof(SpOp));
  UP(sp_nz, G.nz); d.sp_nz_bytes = (uint32_t)(G.nz.size() * sizeof(SpNz));
  { std::vector<int32_t> fs(G.fill_slots); if (fs.empty()) fs.push_back(G.n_blocks - 1); UP(sp_fill_slots, fs); }
  if (const int rc = alloc_nrbuf(h, 0, (size_t)P.n)) return rc;
  if (nr_sparse_prepare(h->sp_lanes) != 0) { (void)hipGetLastError(); h->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for k_nr_sparse"; return MAPDN_E_HIP; }
  return MAPDN_OK;
}

// k_nr_tree (nr_tree.hpp): the launch geometry (settle_tree_geometry), its schedule and the NR scratch
static int setup_tree(mapdn_handle* h) {
  const Plan& P = h->plan;
  Dev& d = h->d;
  hipDeviceProp_t prop;
  HIPCHK(h, hipGetDeviceProperties(&prop, h->device));
  if (const int rc = settle_tree_geometry(h, d.Bp, prop.multiProcessorCount)) return rc;
  const mapdn_handle::Geo& G_ = h->geo;
  const Schedule& S = h->sched;
  d.nr_waves = G_.W; d.nr_lanes = G_.L; d.nr_h_lds = G_.h_lds; d.nr_g_lds = G_.g_lds; d.nr_line_lds = G_.line_lds; d.nr_rec_lds = G_.rec_lds; d.nr_flat_lds = G_.flat_lds;
  d.nr_check_dx = h->knobs.check_dx; d.nr_check_quad = h->knobs.check_quad;
  d.nr_rows = S.R; d.nr_cslots = S.n_cslots; d.nr_xslots = S.n_xslots; d.nr_nclist = G_.ncl;
  {
    // the attribute is per kernel function, not per handle: always raise it to the full 160 KB so that
    // handles with different LDS needs can share an instantiation
    const int lr = nr_set_lds_limit(G_.W, G_.L, G_.h_lds, G_.g_lds, G_.rec_lds, G_.flat_lds, CU_LDS, h->nr_var);
    if (lr == -2) { h->err = "this (nr_waves, nr_lanes) combination is not compiled in (csrc/nr_inst_list.hpp)"; return MAPDN_E_INVALID; }
    if (lr != 0) { (void)hipGetLastError(); h->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"; return MAPDN_E_HIP; }
  }
  UP(sched, S.steps); d.sched_bytes = (uint32_t)(S.steps.size() * sizeof(StepRec));
  UP(clist, S.clist);
  UP(mm_ptr, S.mm_ptr); UP(mm_child, S.mm_child);
  UP(mm_recs, S.mm_recs); d.mm_recs_bytes = (uint32_t)(S.mm_recs.size() * sizeof(StepRec)); d.mm_np = S.mm_np;
  d.nr_mm_pass = G_.mm_pass;   // the predicted-final mismatch evaluation as a barrier-free pass over all nodes instead of a tree sweep
  UP(flat, S.flat); d.flat_bytes = (uint32_t)(S.flat.size() * sizeof(double));
  if (d.nr_init == 2) { UP(dc_recs, S.dc_recs); d.dc_recs_bytes = (uint32_t)(S.dc_recs.size() * sizeof(DcRec)); }
  // NR scratch: factor blocks (one per node) | 2 x Sbus (one entry per node) | Vout
  const size_t nblk = (size_t)P.n + 2;           // Sbus by node position (+ slack, + the trash node of idle steps: stays 0)
  const size_t fb_rows = (G_.h_lds && G_.g_lds) ? 0 : (size_t)(P.n + 2) * NBP;   // pair rows of Bp x 16 bytes: one block per node (+ slack, trash)
  return alloc_nrbuf(h, fb_rows, nblk);
}

#undef UP
#undef AL

static int create_impl(mapdn_handle* h, const mapdn_netspec* net, const mapdn_env_config* cfg, int32_t B, int32_t device) {
  if (!net || !cfg) { h->err = "null netspec/config"; return MAPDN_E_INVALID; }
  if (B < 1) { h->err = "n_envs must be >= 1"; return MAPDN_E_INVALID; }
  if (cfg->barrier_type < 0 || cfg->barrier_type > MAPDN_BARRIER_BUMP) { h->err = "unknown voltage_barrier_type"; return MAPDN_E_INVALID; }
  if (!cfg->use_line_weight && !cfg->use_q_weight) {   // voltage_control_env.py:616-617
    h->err = "NotImplementedError: Please at least give one weight, either q_weight or line_weight."; return MAPDN_E_INVALID; }
  if (cfg->episode_limit < 2) { h->err = "episode_limit must be >= 2"; return MAPDN_E_INVALID; }
  h->cfg = *cfg;
  h->knobs = resolve_knobs(*cfg);
  int rc = build_plan(*net, *cfg, h->plan, h->err);
  if (!rc) rc = choose_solver(h);
  if (!rc) rc = validate(h, *cfg);
  if (rc) return rc;
  h->nr_var = (cfg->nr_init == 2 ? NR_VAR_DC : 0) | (h->plan.zip ? NR_VAR_ZIP : 0) | (h->plan.gen_start ? NR_VAR_GEN : 0);
  // composition of the step() launches: the PV-bus injection runs in the prologue of k_nr_tree unless the handle auto-resets (its
  // restarting envs refresh all their loads in the injection launch), rebuilds all of Sbus on every call, or pins fuse_inject = 2
  h->fuse_inject = h->solver == 0 && !cfg->auto_reset && !h->knobs.inject_full && h->knobs.fuse_inject != 2;
  h->device = device;
  std::memset(&h->d, 0, sizeof(h->d));
  h->d.B = B; h->d.Bp = (B + 63) / 64 * 64;
  if ((rc = settle_general_solver(h))) return rc;
  h->branches = h->plan.branches;
  if (device == -1) {                                            // plan only (CPU tests): no device work
    h->host_only = true;
    return h->solver == 0 ? settle_tree_geometry(h, h->d.Bp, 256) : MAPDN_OK;   // (an MI355X has 256 CUs)
  }
  int ndev = 0;
  HIPCHK(h, hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) { h->err = "device index out of range"; return MAPDN_E_HIP; }
  HIPCHK(h, hipSetDevice(device));
  if ((rc = upload_topology(h)) || (rc = setup_pv_buses(h)) || (rc = setup_env_state(h)) || (rc = setup_gather_tables(h))) return rc;
  if ((rc = dupload(h, &h->branches_dev, h->branches))) return rc;
  return h->solver == 2 ? setup_dense(h) : h->solver == 1 ? setup_sparse(h) : setup_tree(h);
}

extern "C" {

const char* mapdn_last_error(const mapdn_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

#ifndef MAPDN_SRC_HASH
#define MAPDN_SRC_HASH "unknown"
#endif
// "MAPDN_SRC_HASH=<sha256 of the sources and flags this library was built from>" (mapdn_amd/build.py): the loader compares it with the
// sources on disk, so that a prebuilt library can never silently disagree with them
const char* mapdn_build_info(void) { return "MAPDN_SRC_HASH=" MAPDN_SRC_HASH; }

int mapdn_create(const mapdn_netspec* net, const mapdn_env_config* cfg, int32_t n_envs, int32_t device, mapdn_handle** out) {
  if (!out) { g_create_err = "null out pointer"; return MAPDN_E_INVALID; }
  *out = nullptr;
  mapdn_handle* h = nullptr;
  try {
    h = new mapdn_handle();
    const int rc = create_impl(h, net, cfg, n_envs, device);        // plan.cpp: dozens of std::vector / std::string allocations
    if (rc) { g_create_err = h->err; mapdn_destroy(h); return rc; }
    *out = h;
    return MAPDN_OK;
  } catch (...) {
    mapdn_destroy(h);                                                // (frees whatever the half-built handle owns; null is fine)
    try { throw; } MAPDN_CATCH(nullptr)
  }
}

void mapdn_destroy(mapdn_handle* h) {
  if (!h) return;
  for (void* p : h->allocs) (void)hipFree(p);
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  delete h;
}

int mapdn_dims(const mapdn_handle* h, mapdn_dims_t* out) try {
  if (!h || !out) return MAPDN_E_INVALID;
  const Plan& P = h->plan;
  out->n_envs = h->d.B; out->n_bus = P.nbo; out->n_line = P.n_line; out->n_load = P.nl; out->n_sgen = P.ns;
  out->n_agents = P.n_agents; out->n_actions = 1; out->obs_size = P.obs_size; out->state_size = P.state_size;
  out->n_info = MAPDN_N_INFO; out->is_radial = P.radial ? 1 : 0; out->max_zone_size = P.max_zone; out->n_gen = P.n_gen;
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_set_profiles(mapdn_handle* h, const double* pv, const double* load_p, const double* load_q,
                       int64_t T, int32_t time_delta_min, int32_t days) try {
  if (!h) return MAPDN_E_INVALID;
  if (!pv || !load_p || !load_q || T < 2) { h->err = "set_profiles: null table or too few rows"; return MAPDN_E_INVALID; }
  if (time_delta_min <= 0 || 60 % time_delta_min) { h->err = "set_profiles: time_delta_min must divide 60"; return MAPDN_E_INVALID; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  Dev& d = h->d;
  const int ns = d.ns, nl = d.nl, ncol = d.ncol;
  d.per_hour = 60 / time_delta_min; d.per_day = 24 * d.per_hour;
  const int episode_days = d.episode_limit / d.per_day + 1;          // voltage_control_env.py:397
  d.n_start_days = days - episode_days;                              // :398
  if (d.n_start_days < 1) { h->err = "set_profiles: table too short for one episode (pv_days - episode_days < 1)"; return MAPDN_E_INVALID; }
  const int64_t max_start = (d.per_hour - 1) + 23 * d.per_hour + (int64_t)(d.n_start_days - 1) * d.per_day;
  if (max_start + d.episode_limit + 1 >= T) { h->err = "set_profiles: sampled episodes could run past the end of the table"; return MAPDN_E_INVALID; }
  std::vector<double> tab((size_t)T * ncol), stdv(ncol), smax(ns);
  for (int64_t t = 0; t < T; ++t) {
    double* r = &tab[(size_t)t * ncol];
    std::memcpy(r, pv + (size_t)t * ns, ns * sizeof(double));
    std::memcpy(r + ns, load_p + (size_t)t * nl, nl * sizeof(double));
    std::memcpy(r + ns + nl, load_q + (size_t)t * nl, nl * sizeof(double));
  }
  // population std over the whole table / 100 (:70-72) in numpy's own summation order (colstats.hpp: pairwise along every column, as
  // `DataFrame.values.std(axis=0)` does on its F-ordered block), read row-major; s_max = 1.2 * max_t pv (:518-520)
  column_std(tab.data(), T, ncol, 100.0, stdv);
  for (int j = 0; j < ns; ++j) smax[(size_t)j] = tab[(size_t)j];
  for (int64_t t = 1; t < T; ++t) {
    const double* r = &tab[(size_t)t * ncol];
    for (int j = 0; j < ns; ++j) smax[(size_t)j] = std::max(smax[(size_t)j], r[j]);
  }
  for (int j = 0; j < ns; ++j) smax[(size_t)j] *= 1.2;
  if (h->have_profiles) {   // replace: free the old table
    for (double* p : {h->table, h->stdv, h->smax}) {
      auto it = std::find(h->allocs.begin(), h->allocs.end(), (void*)p);
      if (it != h->allocs.end()) { (void)hipFree(*it); h->allocs.erase(it); }
    }
  }
  int rc;
  if ((rc = dupload(h, &h->table, tab)) || (rc = dupload(h, &h->stdv, stdv)) || (rc = dupload(h, &h->smax, smax))) return rc;
  d.table = h->table; d.stdv = h->stdv; d.smax = h->smax; d.T = T;
  h->stdv_host = stdv; h->smax_host = smax;
  h->have_profiles = true;
  return MAPDN_OK;
} MAPDN_CATCH(h)

// dv: the Dev of the launch when it is not the handle's own (the droop solves run with their own active / iters / conv arrays)
static void nr_launch(mapdn_handle* h, int mode, double* reward, uint8_t* term, double* info, hipStream_t st,
                      const void* fused_actions = nullptr, int fused_dtype = 0, const Dev* dv = nullptr) {
  const Dev& d = dv ? *dv : h->d;
  if (!h->timing) { launch_nr(d, mode, reward, term, info, st, fused_actions, fused_dtype); return; }
  if (h->ev_used + 2 > h->ev.size()) {
    if (h->ev.size() >= 2 * 8192) {   // pool full: drain
      double ms; int64_t n; mapdn_nr_time_ms(h, &ms, &n); h->acc_ms = ms; h->acc_launches = n;
    } else {
      hipEvent_t a, b;
      (void)hipEventCreate(&a); (void)hipEventCreate(&b);
      h->ev.push_back(a); h->ev.push_back(b);
    }
  }
  hipEvent_t a = h->ev[h->ev_used], b = h->ev[h->ev_used + 1];
  h->ev_used += 2;
  (void)hipEventRecord(a, st);
  launch_nr(d, mode, reward, term, info, st, fused_actions, fused_dtype);
  (void)hipEventRecord(b, st);
}

// the injection of a step() / reset() call: PV buses only when Sbus and bus_ld are known to reflect the current loads
static void inject_launch(mapdn_handle* h, int mode, const void* actions, int dtype, int add_noise, hipStream_t st) {
  const Dev& d = h->d;
  if (h->sbus_stale || h->knobs.inject_full) {
    launch_inject(d, mode, actions, dtype, d.cur_pl, d.cur_ql, d.cur_pv, nullptr, add_noise, st);
    h->sbus_stale = false;
  } else launch_inject_sgen(d, mode, actions, dtype, add_noise, st);
}

// The launches of one step(): injection (its own launch, or the prologue of k_nr_tree: fuse_inject) -> solve + reward ->
// profile advance (-> the Sbus buffer of the next solve) + res_bus commit.
static void step_launches(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t add_noise, double* reward,
                          uint8_t* terminated, double* info, hipStream_t st) {
  const Dev& d = h->d;
  const bool fused = h->fuse_inject && !h->sbus_stale;
  if (!fused) inject_launch(h, MODE_STEP, actions, actions_dtype, add_noise, st);
  nr_launch(h, MODE_STEP, reward, terminated, info, st, fused ? actions : nullptr, actions_dtype);
  if (d.zip) {
    // voltage-dependent loads: the commit of a ZIP bus reads the loads the solve used (cur_pl / cur_ql), so it runs before the profile
    // rows overwrite them (two launches; no fused buses with ZIP loads)
    launch_advance(d, 0, 0, 1, d.sb_off_alt, st);
    launch_advance(d, add_noise, 1, 0, d.sb_off_alt, st);
  } else {
    launch_commit_fused(d, st);     // (only with fused buses: their own p_mw / q_mvar, before the element tables advance)
    launch_advance(d, add_noise, 1, 1, d.sb_off_alt, st);   // next profile row (-> the Sbus buffer of the next solve) + res_bus commit
  }
  std::swap(h->d.sb_off, h->d.sb_off_alt);
}

int mapdn_reset(mapdn_handle* h, const int64_t* start_rows, int32_t add_noise, int32_t max_tries, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!h->have_profiles) { h->err = "reset before set_profiles"; return MAPDN_E_STATE; }
  if (max_tries < 1) max_tries = 1;
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const Dev& d = h->d;
  for (int t = 0; t < max_tries; ++t) {
    launch_reset_begin(d, start_rows, t == 0, st);
    launch_advance(d, add_noise, 1, 0, d.sb_off, st);   // the advance precedes the solve here: it fills the buffer the solve reads
    inject_launch(h, MODE_RESET, nullptr, MAPDN_F64, add_noise, st);
    nr_launch(h, MODE_RESET, nullptr, nullptr, nullptr, st);
    launch_commit_fused(d, st);
    launch_advance(d, 0, 0, 1, d.sb_off, st);    // res_bus commit of the envs that found a solvable start
  }
  HIPCHK(h, hipGetLastError());
  h->was_reset = true;
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_step(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t add_noise, double* reward,
               uint8_t* terminated, double* info, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!h->was_reset) { h->err = "step before reset"; return MAPDN_E_STATE; }
  if (!actions || !reward || !terminated || !info) { h->err = "step: null buffer"; return MAPDN_E_INVALID; }
  if (actions_dtype != MAPDN_F32 && actions_dtype != MAPDN_F64) { h->err = "step: bad actions dtype"; return MAPDN_E_INVALID; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  step_launches(h, actions, actions_dtype, add_noise, reward, terminated, info, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_step_obs(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t add_noise, double* reward,
                   uint8_t* terminated, double* info, void* obs, int32_t obs_dtype, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!h->was_reset) { h->err = "step before reset"; return MAPDN_E_STATE; }
  if (!actions || !reward || !terminated || !info || !obs) { h->err = "step_obs: null buffer"; return MAPDN_E_INVALID; }
  if (actions_dtype != MAPDN_F32 && actions_dtype != MAPDN_F64) { h->err = "step_obs: bad actions dtype"; return MAPDN_E_INVALID; }
  if (obs_dtype != MAPDN_F32 && obs_dtype != MAPDN_F64) { h->err = "step_obs: bad obs dtype"; return MAPDN_E_INVALID; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const Dev& d = h->d;
  const int C = h->plan.n_agents * h->plan.obs_size;
  step_launches(h, actions, actions_dtype, add_noise, reward, terminated, info, st);
  launch_gather(d, d.gbuf, h->obs_rows, h->obs_scale, 1.0, h->obs_xptr, h->obs_xrow, obs, obs_dtype, C, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_obs(mapdn_handle* h, void* obs, int32_t dtype, void* stream) try {
  if (!h || !obs) return MAPDN_E_INVALID;
  if (!h->was_reset) { h->err = "get_obs before reset"; return MAPDN_E_STATE; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  launch_gather(h->d, h->d.gbuf, h->obs_rows, h->obs_scale, 1.0, h->obs_xptr, h->obs_xrow, obs, dtype,
                h->plan.n_agents * h->plan.obs_size, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_state(mapdn_handle* h, void* state, int32_t dtype, void* stream) try {
  if (!h || !state) return MAPDN_E_INVALID;
  if (!h->was_reset) { h->err = "get_state before reset"; return MAPDN_E_STATE; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  launch_gather(h->d, h->d.gbuf, h->state_rows, h->state_scale, 1.0, nullptr, nullptr, state, dtype, h->plan.state_size, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

static void transpose_out(mapdn_handle* h, const double* src, double scale, const int32_t* rows, double* out, int n, hipStream_t st) {
  launch_gather(h->d, src, rows, nullptr, scale, nullptr, nullptr, out, MAPDN_F64, n, st);
}

int mapdn_get_results(mapdn_handle* h, double* vm_pu, double* va_degree, double* p_mw, double* q_mvar, double* pl_mw,
                      double* sgen_p, double* sgen_q, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!h->was_reset) { h->err = "get_results before reset"; return MAPDN_E_STATE; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const Dev& d = h->d;
  if (vm_pu) transpose_out(h, d.vm, 1.0, h->iota_idx, vm_pu, d.nbo, st);
  if (va_degree) transpose_out(h, d.va, 180.0 / M_PI, h->iota_idx, va_degree, d.nbo, st);
  if (p_mw) transpose_out(h, d.res_p, 1.0, h->iota_idx, p_mw, d.nbo, st);
  if (q_mvar) transpose_out(h, d.res_q, 1.0, h->iota_idx, q_mvar, d.nbo, st);
  if (pl_mw) transpose_out(h, d.pl, 1.0, h->iota_idx, pl_mw, d.n_line, st);
  if (sgen_p) transpose_out(h, d.cur_pv, 1.0, h->iota_idx, sgen_p, d.ns, st);
  if (sgen_q) transpose_out(h, d.cur_q, 1.0, h->iota_idx, sgen_q, d.ns, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

// res_gen: p_mw is a constant of the plan, q_mvar what commit_bus left, vm_pu / va_degree the rows of the gens' buses
int mapdn_get_res_gen(mapdn_handle* h, double* p_mw, double* q_mvar, double* vm_pu, double* va_degree, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!h->was_reset) { h->err = "get_res_gen before reset"; return MAPDN_E_STATE; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const Dev& d = h->d;
  const int ng = d.n_gen;
  if (ng == 0) return MAPDN_OK;
  if (p_mw) transpose_out(h, h->gen_p_rows, 1.0, h->iota_idx, p_mw, ng, st);   // constant rows, uploaded once (setup_env_state)
  if (q_mvar) transpose_out(h, d.res_gen_q, 1.0, h->iota_idx, q_mvar, ng, st);
  if (vm_pu) transpose_out(h, d.vm, 1.0, h->gen_bus_rows, vm_pu, ng, st);
  if (va_degree) transpose_out(h, d.va, 180.0 / M_PI, h->gen_bus_rows, va_degree, ng, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_loads(mapdn_handle* h, double* load_p, double* load_q, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  if (load_p) transpose_out(h, h->d.cur_pl, 1.0, h->iota_idx, load_p, h->d.nl, st);
  if (load_q) transpose_out(h, h->d.cur_ql, 1.0, h->iota_idx, load_q, h->d.nl, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

// ---- res_line / res_trafo ------------------------------------------------------------------------------------------------------------
int mapdn_set_branch_ratings(mapdn_handle* h, const double* line_max_i_ka, const double* line_df, const double* br_vn_hv_kv,
                             const double* br_vn_lv_kv, const double* br_rating_mva) try {
  if (!h) return MAPDN_E_INVALID;
  const int n_line = h->plan.n_line, n_tr = (int)h->plan.branches.size() - n_line;
  // NaN in a RATING column (max_i_ka, rating_mva) leaves that row unrated, as a missing value does in pandapower; anything else that is
  // not a finite positive number is refused, by column and row
  auto check = [&](const double* v, int n, const char* what, bool nan_ok) {
    for (int i = 0; v && i < n; ++i) {
      if (nan_ok && v[i] != v[i]) continue;
      if (!(v[i] > 0.0) || !std::isfinite(v[i])) {
        h->err = std::string("set_branch_ratings: ") + what + "[" + std::to_string(i) + "] = " + std::to_string(v[i]) + " must be finite and > 0";
        return false;
      }
    }
    return true;
  };
  if (!check(line_max_i_ka, n_line, "line_max_i_ka", true) || !check(line_df, n_line, "line_df", false) ||
      !check(br_vn_hv_kv, n_tr, "br_vn_hv_kv", false) || !check(br_vn_lv_kv, n_tr, "br_vn_lv_kv", false) ||
      !check(br_rating_mva, n_tr, "br_rating_mva", true))
    return MAPDN_E_INVALID;
  std::vector<BranchRec> br(h->plan.branches);                   // (unrated: rate = NaN)
  for (int l = 0; line_max_i_ka && l < n_line; ++l)
    br[l].rate = line_max_i_ka[l] * (line_df ? line_df[l] : 1.0) * br[l].parallel;
  for (int k = 0; br_rating_mva && br_vn_hv_kv && br_vn_lv_kv && k < n_tr; ++k) {
    BranchRec& r = br[n_line + k];
    r.rate = br_rating_mva[k]; r.tv_f = br_vn_hv_kv[k]; r.tv_t = br_vn_lv_kv[k];
  }
  if (!h->host_only) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!br.empty()) HIPCHK(h, hipMemcpy(h->branches_dev, br.data(), br.size() * sizeof(BranchRec), hipMemcpyHostToDevice));
  }
  h->branches.swap(br);
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_branch_results(mapdn_handle* h, const double* vm_pu, const double* va_degree, const mapdn_branch_out* line,
                             const mapdn_branch_out* trafo, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if ((vm_pu == nullptr) != (va_degree == nullptr)) { h->err = "get_branch_results: vm_pu and va_degree go together (both, or both NULL for the env's state)"; return MAPDN_E_INVALID; }
  if (!vm_pu && !h->was_reset) { h->err = "get_branch_results before reset"; return MAPDN_E_STATE; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  const Dev& d = h->d;
  BranchArgs a{};
  a.rec = h->branches_dev; a.n_line = d.n_line; a.n_trafo = (int32_t)h->branches.size() - d.n_line; a.B = d.B; a.sn = d.sn;
  if (vm_pu) { a.vm = vm_pu; a.va = va_degree; a.sb = 1; a.se = d.nbo; a.ang = M_PI / 180.0; }
  else { a.vm = d.vm; a.va = d.va; a.sb = d.Bp; a.se = 1; a.ang = 1.0; }
  const mapdn_branch_out* tab[2] = {line, trafo};
  bool any[2] = {false, false};
  for (int t = 0; t < 2; ++t) {
    if (!tab[t]) continue;
    double* const cols[BC_N] = {tab[t]->p_from_mw, tab[t]->q_from_mvar, tab[t]->p_to_mw, tab[t]->q_to_mvar, tab[t]->pl_mw, tab[t]->ql_mvar,
                                tab[t]->i_from_ka, tab[t]->i_to_ka, tab[t]->i_ka, tab[t]->loading_percent};
    for (int c = 0; c < BC_N; ++c) { a.out[t][c] = cols[c]; any[t] = any[t] || cols[c]; }
  }
  a.line_tiles = any[0] ? (a.n_line + BR_TILE - 1) / BR_TILE : 0;
  a.trafo_tiles = any[1] ? (a.n_trafo + BR_TILE - 1) / BR_TILE : 0;
  launch_branch_results(a, d.Bp, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_loading_summary(mapdn_handle* h, double limit_percent, double* max_loading, int32_t* worst_branch, int32_t* n_overloaded,
                              void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!h->was_reset) { h->err = "get_loading_summary before reset"; return MAPDN_E_STATE; }
  if (!max_loading || !worst_branch || !n_overloaded) { h->err = "get_loading_summary: null buffer"; return MAPDN_E_INVALID; }
  if (limit_percent != limit_percent) { h->err = "get_loading_summary: limit_percent is NaN"; return MAPDN_E_INVALID; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  const Dev& d = h->d;
  LoadingArgs a{};
  a.rec = h->branches_dev; a.n_branch = (int32_t)h->branches.size(); a.B = d.B; a.Bp = d.Bp; a.vm = d.vm; a.va = d.va; a.sn = d.sn;
  a.limit = limit_percent; a.max_loading = max_loading; a.worst = worst_branch; a.n_over = n_overloaded;
  launch_loading_summary(a, (hipStream_t)stream);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_start_rows(mapdn_handle* h, int64_t* start_rows, void* stream) try {
  if (!h || !start_rows) return MAPDN_E_INVALID;
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(start_rows, h->d.start_row, (size_t)h->d.B * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_auto_reset_mask(mapdn_handle* h, uint8_t* mask, void* stream) try {
  if (!h || !mask) return MAPDN_E_INVALID;
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(mask, h->d.resetting, (size_t)h->d.B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_returns(mapdn_handle* h, double* returns, void* stream) try {
  if (!h || !returns) return MAPDN_E_INVALID;
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(returns, h->d.sum_rewards, (size_t)h->d.B * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_solve_only(mapdn_handle* h, const double* p_load, const double* q_load, const double* p_sgen, const double* q_sgen,
                     double* vm_pu, double* va_degree, int32_t* iterations, uint8_t* converged, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!p_load || !q_load || !p_sgen || !q_sgen) { h->err = "solve_only: null input"; return MAPDN_E_INVALID; }
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const Dev& d = h->d;
  launch_to_envminor(d, p_load, h->t_pl, d.nl, st);
  launch_to_envminor(d, q_load, h->t_ql, d.nl, st);
  launch_to_envminor(d, p_sgen, h->t_pv, d.ns, st);
  launch_to_envminor(d, q_sgen, h->t_q, d.ns, st);
  HIPCHK(h, hipMemsetAsync(d.active, 1, d.B, st));
  if (d.Bp > d.B) HIPCHK(h, hipMemsetAsync(d.active + d.B, 0, d.Bp - d.B, st));
  launch_inject(d, MODE_SOLVE, nullptr, MAPDN_F64, h->t_pl, h->t_ql, h->t_pv, h->t_q, 0, st);
  h->sbus_stale = true;                          // Sbus now holds the caller's loads, not cur_pl / cur_ql
  nr_launch(h, MODE_SOLVE, nullptr, nullptr, nullptr, st);
  if (vm_pu) transpose_out(h, d.nrbuf, 1.0, h->vm_row, vm_pu, d.nbo, st);
  if (va_degree) transpose_out(h, d.nrbuf, 180.0 / M_PI, h->va_row, va_degree, d.nbo, st);
  if (iterations) launch_copy_i32(d.iters, iterations, d.B, st);
  if (converged) launch_copy_u8(d.conv, converged, d.B, st);
  HIPCHK(h, hipGetLastError());
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_profile_stats(const mapdn_handle* h, double* stdv, double* smax) try {
  if (!h) return MAPDN_E_INVALID;
  if (!h->have_profiles) { const_cast<mapdn_handle*>(h)->err = "get_profile_stats before set_profiles"; return MAPDN_E_STATE; }
  if (stdv) std::memcpy(stdv, h->stdv_host.data(), h->stdv_host.size() * sizeof(double));
  if (smax) std::memcpy(smax, h->smax_host.data(), h->smax_host.size() * sizeof(double));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_ybus_dense(const mapdn_handle* h, double* out) try {
  if (!h || !out) return MAPDN_E_INVALID;
  const Plan& P = h->plan;
  for (size_t i = 0; i < P.ybus.size(); ++i) { out[2 * i] = P.ybus[i].real(); out[2 * i + 1] = P.ybus[i].imag(); }
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_obs_index(const mapdn_handle* h, int32_t* kind, int32_t* index) try {
  if (!h || !kind || !index) return MAPDN_E_INVALID;
  std::memcpy(kind, h->plan.obs_kind.data(), h->plan.obs_kind.size() * sizeof(int32_t));
  std::memcpy(index, h->plan.obs_idx.data(), h->plan.obs_idx.size() * sizeof(int32_t));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_nr_geometry(const mapdn_handle* h, int32_t* out) try {
  if (!h || !out) return MAPDN_E_INVALID;
  const mapdn_handle::Geo& g = h->geo;
  const int32_t v[20] = {h->solver, g.W, g.L, g.lean, g.rows, g.h_lds, g.g_lds, g.rec_lds, g.flat_lds, g.line_lds, g.mm_pass,
                         (int32_t)h->lds_bytes, (int32_t)g.wgs, g.resident, g.rounds, (int32_t)std::min(g.model_ns, 2.0e9),
                         h->fuse_inject ? 1 : 0, (int32_t)h->plan.fused_obus.size(), h->plan.nb, h->cfg.nr_init};
  std::memcpy(out, v, sizeof(v));
  if (h->solver == 1) out[2] = h->sp_lanes;
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_nr_kernel(const mapdn_handle* h, int32_t* out) try {
  if (!h || !out) return MAPDN_E_INVALID;
  const int dc = h->cfg.nr_init == 2 ? 1 : 0, zip = (h->plan.zip ? 1 : 0) | (h->plan.gen_start ? 2 : 0);   // bit 1: the GEN form
  int32_t v[8] = {h->solver, 0, 0, 0, 0, 0, 0, 0};
  if (h->solver == 0) {
    const mapdn_handle::Geo& g = h->geo;
    const NrInst* I = nr_inst_of(g.W, g.L, g.h_lds, g.g_lds, g.rec_lds, g.flat_lds, h->nr_var);
    if (!I) return api_fail(h, MAPDN_E_INTERNAL, "mapdn_get_nr_kernel: the handle's geometry has no k_nr_tree instantiation");
    const int32_t t[7] = {I->W, I->L, I->HL, I->GL, I->RES, (I->VAR & NR_VAR_DC) ? 1 : 0, ((I->VAR & NR_VAR_ZIP) ? 1 : 0) | ((I->VAR & NR_VAR_GEN) ? 2 : 0)};
    std::memcpy(v + 1, t, sizeof(t));
  } else if (h->solver == 1) {
    v[1] = h->sp_lanes; v[2] = dc; v[3] = zip;
  } else {
    const bool ga = nr_dense_ga(h->d.dn_N);
    v[1] = nr_dense_waves(h->d.dn_N, ga); v[2] = ga ? 1 : 0;
  }
  std::memcpy(out, v, sizeof(v));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_dc_angles(const mapdn_handle* h, const double* p_bus_demand_mw, double* va_rad) try {
  if (!h || !p_bus_demand_mw || !va_rad) return MAPDN_E_INVALID;
  const Plan& P = h->plan;
  if (!P.dc_ok) return api_fail(h, MAPDN_E_INVALID, P.fused_obus.empty() ? "the DC power flow matrix Bbus of this net is singular or not finite"
                                                                          : "the DC-angle start is not defined on a net with fused buses (bus_alias)");
  const int n = P.n;
  std::vector<double> pbus(n);                   // Pbus = Re(Sbus) + dc_pc, Re(Sbus) = -P_demand / sn (as the injection forms it)
  for (int k = 0; k < n; ++k) pbus[k] = -(p_bus_demand_mw[P.bus_of_pos[k]] - P.gen_p_pos[k]) / P.sn_mva + P.dc_pc[k];   // (sbus_entry: P_gen is a negative demand)
  std::vector<double> th(n + 1, 0.0);            // by position; the slack (n) stays 0
  if (h->solver == 0) {                          // k_nr_tree's sweeps, node by node (children in the canonical order)
    Schedule S;
    build_schedule(P, 1, S);
    std::vector<double> c(n, 0.0), hh(n, 0.0);
    for (int k = 0; k < n; ++k) {
      double y = pbus[k];
      for (int j = S.mm_ptr[k]; j < S.mm_ptr[k + 1]; ++j) y -= c[S.mm_child[j]];
      hh[k] = y * P.dc_id[k];
      c[k] = P.dc_bpk[k] * hh[k];
    }
    for (int k = n - 1; k >= 0; --k) th[k] = std::fma(-P.dc_g[k], th[P.par[k]], hh[k]);
  } else {                                       // k_nr_sparse's block program on the Bbus assembly
    SparseProg G;
    const int S = h->sp_lanes ? 64 / h->sp_lanes : 4;
    sparse_program(P, S, G);
    std::vector<double> B((size_t)G.n_blocks * 4, 0.0);          // a00 a01 a10 a11
    for (size_t r = 0; r < G.rows.size(); ++r) {
      const SpRow& R = G.rows[r];
      if (!R.live) continue;
      const int i = (int)R.node;
      for (int q = 0; q < G.max_nnz; ++q) {
        const SpNz& z = G.nz[r * G.max_nnz + q];
        if ((int)(z.col & ~SP_COL_GEN) == i) B[(size_t)i * 4] = z.bdc;
        else if (z.slot >= 0) { double* o = &B[(size_t)z.slot * 4]; o[0] = z.bdc; o[1] = o[2] = o[3] = 0.0; }
      }
      B[(size_t)i * 4 + 3] = 1.0;
      B[(size_t)(n + i) * 4] = pbus[i];
    }
    for (int p = 0; p < G.n_phases; ++p)
      for (int s = 0; s < S; ++s) {
        const SpOp& op = G.ops[(size_t)p * S + s];
        const unsigned type = op.type & 255u;
        if (type == 0u) continue;
        const double* a = &B[(size_t)op.a * 4]; const double* b = &B[(size_t)op.b * 4];
        double r[4];
        if (type == 1u) { const double id = 1.0 / (a[0] * a[3] - a[1] * a[2]); r[0] = a[3] * id; r[1] = -a[1] * id; r[2] = -a[2] * id; r[3] = a[0] * id; }
        else {
          const double m[4] = {a[0] * b[0] + a[1] * b[2], a[0] * b[1] + a[1] * b[3], a[2] * b[0] + a[3] * b[2], a[2] * b[1] + a[3] * b[3]};
          const double* c0 = &B[(size_t)op.c * 4];
          for (int j = 0; j < 4; ++j) r[j] = type == 2u ? m[j] : c0[j] - m[j];
        }
        std::memcpy(&B[(size_t)op.c * 4], r, sizeof(r));
      }
    for (int i = 0; i < n; ++i) th[i] = B[(size_t)(n + i) * 4];
  }
  for (int b = 0; b < P.nbo; ++b) va_rad[b] = th[P.pos_of_obus[b]];
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_flat_factors(const mapdn_handle* h, double* factors, int32_t* bus_of_pos) try {
  if (!h || !factors) return MAPDN_E_INVALID;
  if (!h->plan.radial) return MAPDN_E_TOPOLOGY;   // the tree factorisation exists for radial feeders only
  Schedule S;
  build_schedule(h->plan, 1, S);                 // one worker: row r of the schedule is one node
  const int n = h->plan.n;
  for (int r = 0; r < S.R; ++r) {
    const StepRec& T = S.steps[(size_t)r];
    if (T.flags & S_LIVE) std::memcpy(factors + (size_t)(T.kp & 0xffffu) * FLAT_N, &S.flat[(size_t)r * FLAT_N], FLAT_N * sizeof(double));
  }
  if (bus_of_pos) std::memcpy(bus_of_pos, h->plan.bus_of_pos.data(), (size_t)(n + 1) * sizeof(int32_t));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_schedule(const mapdn_handle* h, int32_t W, int32_t* n_rows, int32_t* rows, int32_t* parent) try {
  if (!h || !n_rows || W < 1 || W > 16) return MAPDN_E_INVALID;
  if (!h->plan.radial) return MAPDN_E_TOPOLOGY;
  Schedule S;
  build_schedule(h->plan, W, S);
  *n_rows = S.R;
  if (rows) for (size_t i = 0; i < S.steps.size(); ++i) rows[i] = (S.steps[i].flags & S_LIVE) ? (int32_t)(S.steps[i].kp & 0xffffu) : -1;
  if (parent) std::memcpy(parent, h->plan.par.data(), h->plan.par.size() * sizeof(int32_t));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_get_sparse_program(const mapdn_handle* h, int32_t S, int32_t* dims, int32_t* ops, int32_t* order, int32_t* slots_ij) try {
  if (!h || !dims || S < 1 || S > 64) return MAPDN_E_INVALID;
  SparseProg G;
  sparse_program(h->plan, S, G);
  dims[0] = G.n_blocks; dims[1] = G.n_fill; dims[2] = G.n_phases; dims[3] = G.rows_per_sub; dims[4] = G.max_nnz;
  dims[5] = (int32_t)(G.slots_ij.size() / 3);
  if (ops) std::memcpy(ops, G.ops.data(), G.ops.size() * sizeof(SpOp));
  if (order) std::memcpy(order, G.order.data(), G.order.size() * sizeof(int32_t));
  if (slots_ij) std::memcpy(slots_ij, G.slots_ij.data(), G.slots_ij.size() * sizeof(int32_t));
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_dense_solve(const double* a, const double* b, double* x, int32_t n, int32_t batch, void* stream) try {
  if (!a || !b || !x) return MAPDN_E_INVALID;
  const int rc = dense_solve_debug(a, b, x, n, batch, (hipStream_t)stream);
  return rc == 0 ? MAPDN_OK : (rc == -1 ? MAPDN_E_INVALID : MAPDN_E_HIP);
} MAPDN_CATCH(nullptr)

int mapdn_stats(mapdn_handle* h, int64_t* reset_failures, double* mean_iters, int32_t* max_iters, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  launch_stats(h->d, h->stats_dev, st);
  long long host[4];
  HIPCHK(h, hipMemcpyAsync(host, h->stats_dev, sizeof(host), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (reset_failures) *reset_failures = host[0];
  if (mean_iters) *mean_iters = host[2] ? (double)host[1] / (double)host[2] : 0.0;
  if (max_iters) *max_iters = (int32_t)host[3];
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_nr_timing(mapdn_handle* h, int32_t enable) try {
  if (!h) return MAPDN_E_INVALID;
  h->timing = enable != 0;
  return MAPDN_OK;
} MAPDN_CATCH(h)

int mapdn_nr_time_ms(mapdn_handle* h, double* total_ms, int64_t* launches) try {
  if (!h) return MAPDN_E_INVALID;
  NEEDDEV(h);
  HIPCHK(h, hipSetDevice(h->device));
  double ms = h->acc_ms; int64_t n = h->acc_launches;
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    HIPCHK(h, hipEventSynchronize(h->ev[i + 1]));
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, h->ev[i], h->ev[i + 1]));
    ms += t; n += 1;
  }
  h->ev_used = 0; h->acc_ms = 0.0; h->acc_launches = 0;
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  return MAPDN_OK;
} MAPDN_CATCH(h)

}  // extern "C"

// The traditional baselines' host side — droop_resolve / droop_prepare / droop_run, opf_resolve / opf_prepare / opf_run / opf_probe and
// the one loop driver they share — compiled inside this unit like ppo.hip and branch.hip; the entry points below check the arguments.
#include "baselines_host.hpp"

extern "C" {

int mapdn_droop_actions(mapdn_handle* h, const mapdn_droop_config* cfg, double* actions, double* vm_pu, int32_t* iterations,
                        uint8_t* status, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  mapdn_droop_config c;
  if (const char* why = droop_resolve(cfg, c)) return api_fail(h, MAPDN_E_INVALID, why);
  if (h->plan.n_gen) return api_fail(h, MAPDN_E_INVALID, "droop_actions: nets with generators (net.gen, gen buses) are not supported (the reference's droop script has no voltage-controlled buses)");
  if (h->plan.gen_start) return api_fail(h, MAPDN_E_INVALID, "droop_actions: a start other than ext_grid_vm_pu (vm_init_pu: out-of-service net.gen rows) is not supported (the loop's solves start at the ext_grid set-point)");
  if (!actions || !iterations || !status) { h->err = "droop_actions: null buffer"; return MAPDN_E_INVALID; }
  NEEDDEV(h);
  if (!h->was_reset) { h->err = "droop_actions before reset"; return MAPDN_E_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return droop_run(h, c, actions, vm_pu, iterations, status, (hipStream_t)stream);
} MAPDN_CATCH(h)

int mapdn_opf_actions(mapdn_handle* h, const mapdn_opf_config* cfg, double* actions, double* vm_pu, double* loss_mw, double* violation,
                      int32_t* iterations, uint8_t* status, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  mapdn_opf_config c;
  if (const char* why = opf_resolve(h, cfg, c)) return api_fail(h, MAPDN_E_INVALID, why);
  if (!actions || !iterations || !status) { h->err = "opf_actions: null buffer"; return MAPDN_E_INVALID; }
  NEEDDEV(h);
  if (!h->was_reset) { h->err = "opf_actions before reset"; return MAPDN_E_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return opf_run(h, c, actions, vm_pu, loss_mw, violation, iterations, status, (hipStream_t)stream);
} MAPDN_CATCH(h)

// One linearisation and one QP at the caller's set-points, for the kernel tests: the launches of opf_run's first iteration (the start
// launch — which here begins from a instead of 0 and writes the Sbus of that a —, the solve, k_opf_linearise, k_opf_qp; no k_opf_update
// after them), then the workspace as it stands, env-major.  Writes what opf_run writes.
int mapdn_opf_probe(mapdn_handle* h, const mapdn_opf_config* cfg, const double* a, int32_t ns, double* v_re, double* v_im, double* vm, double* S,
                    double* g, double* H, double* loss_mw, double* violation, double* d, double* y, uint8_t* linearised,
                    uint8_t* qp_capped, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  mapdn_opf_config c;
  if (const char* why = opf_resolve(h, cfg, c)) return api_fail(h, MAPDN_E_INVALID, why);
  if (!a) return api_fail(h, MAPDN_E_INVALID, "opf_probe: a is NULL");
  if (ns != h->plan.ns) return api_fail(h, MAPDN_E_INVALID, "opf_probe: ns must be the handle's number of sgens");
  NEEDDEV(h);
  if (!h->was_reset) { h->err = "opf_probe before reset"; return MAPDN_E_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return opf_probe(h, c, a, ns, v_re, v_im, vm, S, g, H, loss_mw, violation, d, y, linearised, qp_capped, (hipStream_t)stream);
} MAPDN_CATCH(h)

// What step() would report for n_candidates joint actions of every env, without taking the step (whatif.hip; whatif_run).  The
// argument checks come first, so that a host-only handle names a bad argument too; nothing is launched on a refusal.
int mapdn_evaluate_actions(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t n_candidates, double* reward, double* info,
                           uint8_t* status, int32_t* iterations, double* vm_pu, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!actions || !reward || !info || !status) return api_fail(h, MAPDN_E_INVALID, "evaluate_actions: null buffer (actions, reward, info and status are required)");
  if (actions_dtype != MAPDN_F32 && actions_dtype != MAPDN_F64) return api_fail(h, MAPDN_E_INVALID, "evaluate_actions: bad actions dtype");
  if (n_candidates < 1 || n_candidates > MAPDN_WHATIF_MAX_CANDIDATES)
    return api_fail(h, MAPDN_E_INVALID, "evaluate_actions: n_candidates must lie in 1 ... 1024 (MAPDN_WHATIF_MAX_CANDIDATES)");
  NEEDDEV(h);
  if (!h->was_reset) { h->err = "evaluate_actions before reset"; return MAPDN_E_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return whatif_run(h, actions, actions_dtype, n_candidates, reward, info, status, iterations, vm_pu, (hipStream_t)stream);
} MAPDN_CATCH(h)

// mapdn_evaluate_actions with d reward / d action of every candidate beside it (grad.hip; grad_run).  The refusals come first, so that a
// host-only handle names them too; nothing is launched on a refusal.
int mapdn_action_gradients(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t n_candidates, double* grad, double* reward,
                           double* info, uint8_t* status, int32_t* iterations, double* vm_pu, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (const char* why = grad_refusal(h)) return api_fail(h, MAPDN_E_INVALID, why);
  if (!actions || !grad || !reward || !info || !status)
    return api_fail(h, MAPDN_E_INVALID, "action_gradients: null buffer (actions, grad, reward, info and status are required)");
  if (actions_dtype != MAPDN_F32 && actions_dtype != MAPDN_F64) return api_fail(h, MAPDN_E_INVALID, "action_gradients: bad actions dtype");
  if (n_candidates < 1 || n_candidates > MAPDN_WHATIF_MAX_CANDIDATES)
    return api_fail(h, MAPDN_E_INVALID, "action_gradients: n_candidates must lie in 1 ... 1024 (MAPDN_WHATIF_MAX_CANDIDATES)");
  NEEDDEV(h);
  if (!h->was_reset) { h->err = "action_gradients before reset"; return MAPDN_E_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return grad_run(h, actions, actions_dtype, n_candidates, grad, reward, info, status, iterations, vm_pu, (hipStream_t)stream);
} MAPDN_CATCH(h)

// The voltages of every candidate that mapdn_evaluate_actions would score, and the products of n_cotangents caller-supplied cotangents
// over them with their Jacobian by the actions (vjp.hip; vjp_run).  The argument checks come first, then the refusals, both on a
// host-only handle too; nothing is launched on a refusal.
int mapdn_voltage_vjp(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t n_candidates, int32_t n_cotangents,
                      const double* cot_vm, const double* cot_va, double* grad, double* vm_pu, double* va_degree, uint8_t* status,
                      int32_t* iterations, void* stream) try {
  if (!h) return MAPDN_E_INVALID;
  if (!actions || !status) return api_fail(h, MAPDN_E_INVALID, "voltage_vjp: null buffer (actions and status are required)");
  if (actions_dtype != MAPDN_F32 && actions_dtype != MAPDN_F64) return api_fail(h, MAPDN_E_INVALID, "voltage_vjp: bad actions dtype");
  if (n_candidates < 1 || n_candidates > MAPDN_WHATIF_MAX_CANDIDATES)
    return api_fail(h, MAPDN_E_INVALID, "voltage_vjp: n_candidates must lie in 1 ... 1024 (MAPDN_WHATIF_MAX_CANDIDATES)");
  if (n_cotangents < 0 || n_cotangents > MAPDN_VJP_MAX_COTANGENTS)
    return api_fail(h, MAPDN_E_INVALID, "voltage_vjp: n_cotangents must lie in 0 ... 1024 (MAPDN_VJP_MAX_COTANGENTS)");
  if (n_cotangents >= 1 && !cot_vm && !cot_va)
    return api_fail(h, MAPDN_E_INVALID, "voltage_vjp: n_cotangents >= 1 needs cot_vm or cot_va (both are NULL)");
  if ((n_cotangents == 0) != (grad == nullptr))
    return api_fail(h, MAPDN_E_INVALID, "voltage_vjp: grad must be NULL with n_cotangents = 0 and a buffer otherwise");
  if (const char* why = vjp_refusal(h)) return api_fail(h, MAPDN_E_INVALID, why);
  NEEDDEV(h);
  if (!h->was_reset) { h->err = "voltage_vjp before reset"; return MAPDN_E_STATE; }
  HIPCHK(h, hipSetDevice(h->device));
  return vjp_run(h, actions, actions_dtype, n_candidates, n_cotangents, cot_vm, cot_va, grad, vm_pu, va_degree, status, iterations,
                 (hipStream_t)stream);
} MAPDN_CATCH(h)

// ---- the PPO half of MAPPO / IPPO's update (csrc/ppo.hip): argument checks here, nothing is launched on a refusal
static bool ppo_shape_ok(int64_t rows, int32_t n) { return rows >= 1 && n >= 1 && rows <= ((int64_t)1 << 40) / n; }

int mapdn_ppo_gae(const float* reward, const float* value, const float* next_value, const float* done, const float* last_step, float* adv,
                  int64_t rows, int32_t n, int64_t stride, double gamma, double lambda, void* stream) try {
  if (!reward || !value || !next_value || !done || !last_step || !adv || !ppo_shape_ok(rows, n) || stride < 1) return MAPDN_E_INVALID;
  // ppo.py:52-53: gamma and gamma * lambda_ are Python doubles; PyTorch rounds each to f32 where it meets the f32 tensor
  return launch_ppo_gae(reward, value, next_value, done, last_step, adv, rows, n, stride, (float)gamma, (float)(gamma * lambda), (hipStream_t)stream);
} MAPDN_CATCH(nullptr)

int mapdn_ppo_loss_blocks(int64_t elems) try {
  return elems < 1 ? 0 : ppo_loss_blocks(elems);
} MAPDN_CATCH(nullptr)

int mapdn_ppo_policy_loss(const float* action, const float* mean, const float* log_std, const float* avail, const float* old_log_prob,
                          const float* adv, const float* valid, const float* scale, double eps_clip, float* loss, float* dmean,
                          float* partial, int64_t rows, int32_t n, void* stream) try {
  if (!action || !mean || !log_std || !old_log_prob || !adv || !scale || !loss || !dmean || !partial || !ppo_shape_ok(rows, n) || !(eps_clip >= 0.0))
    return MAPDN_E_INVALID;
  // ppo.py:63: 1 - eps_clip and 1 + eps_clip are formed in double, then rounded to f32 by clamp
  return launch_ppo_policy_loss(action, mean, log_std, avail, old_log_prob, adv, valid, scale, (float)(1.0 - eps_clip), (float)(1.0 + eps_clip), loss,
                                dmean, partial, rows, n, (hipStream_t)stream);
} MAPDN_CATCH(nullptr)

int mapdn_ppo_value_loss(const float* v, const float* v_old, const float* reward, const float* v_next, const float* done,
                         const float* valid, const float* scale, double gamma, double eps_clip, double coef, float* loss, float* dv,
                         float* partial, int64_t rows, int32_t n, void* stream) try {
  if (!v || !v_old || !reward || !v_next || !done || !scale || !loss || !dv || !partial || !ppo_shape_ok(rows, n) || !(eps_clip >= 0.0))
    return MAPDN_E_INVALID;
  return launch_ppo_value_loss(v, v_old, reward, v_next, done, valid, scale, (float)gamma, (float)eps_clip, (float)coef, loss, dv, partial, rows, n,
                               (hipStream_t)stream);
} MAPDN_CATCH(nullptr)

}  // extern "C"
