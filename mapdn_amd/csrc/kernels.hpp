// kernels.hpp — device-visible argument block + host launchers of kernels.hip
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan.hpp"

namespace mapdn {

enum { MODE_STEP = 0, MODE_RESET = 1, MODE_SOLVE = 2 };
enum { STREAM_PV = 0, STREAM_LOAD_P = 1, STREAM_LOAD_Q = 2, STREAM_ACTION = 3, STREAM_START = 4 };

// NR global scratch `nrbuf` (env-minor), three regions:
//   factor blocks  [n+2][NBP] pair rows (Bp x 16 bytes)  one block per NODE (position; n+1 = the trash node every idle
//                                step works on): the LU factors (G0,G1) (G2,G3) (h0,h1) written in the forward sweep and
//                                read back in the backward sweep — only for the factors that do not fit in LDS
//                                (nr_h_lds / nr_g_lds)
//   Sbus           2 x [nblk] pair rows   (Re, Im) of the scheduled injection, by node position k (n, n+1: slack and
//                                trash node, stay 0); two buffers, flipped by the host after every step (k_advance fills
//                                the next one)
//   Vout           [n+1][4] rows of Bp doubles   per position (n == slack): e f |V| angle — the solution (k_nr_tree)
// Voltages and everything that crosses workers live in LDS during the solve.
enum { NB_G01 = 0, NB_G23, NB_H, NBP };
enum { VO_E = 0, VO_F, VO_VM, VO_VA, VOF };

// Everything a kernel needs, passed by value (kernarg segment -> scalar loads).
// Layout rule: per-env arrays are env-minor, X[item][Bp]; Bp = B rounded up to 64.
struct Dev {
  int32_t B, Bp, nb, n, nl, ns, n_line, ncol;
  double vroot, sn, tol;
  int32_t max_it;
  // ---- topology plan (shared by all envs; wave-uniform reads)
  const int32_t* bus_of_pos;
  const int32_t *load_ptr, *load_idx, *sgen_ptr, *sgen_idx;
  const double *shunt_p, *shunt_q;
  const double *load_scale, *sgen_scale;     // [nl], [ns] element scaling * in_service (runpp sees p, q * scaling)
  // buses with sgens ("PV buses", n_sgb of them: positions sgb_pos, inverse sgb_of_pos[nb] or -1) and buses with loads but no
  // sgens (lb_pos, n_lb): k_inject_sgen works on the former; bus_ld [n_sgb][Bp] pairs = load part (P, Q) of their injection
  const int32_t *sgb_pos, *sgb_of_pos, *lb_pos, *mlo_pos, *ld_dest; int32_t n_sgb, n_lb, n_mlo;   // mlo_pos: buses with several loads and no sgens;
                                                   // ld_dest[nl]: where a load that is alone on its bus goes (see k_advance)
  double* bus_ld;
  const LineFlow* lines;
  const int32_t* root_children; const double* root_y; int32_t n_root_children;   // children of the slack: position, Y_root,k
  double yrr0, yrr1;
  // ---- profile tables: [T][ncol], columns = pv | load_p | load_q
  const double* table; const double* stdv; const double* smax;
  int64_t T; int32_t n_start_days, per_hour, per_day;
  // ---- config
  int32_t barrier_type, use_line_weight, episode_limit, reset_action, auto_reset;
  double voltage_weight, q_weight, line_weight, v_lower, v_upper, action_low, action_high;
  uint32_t seed_lo, seed_hi; int64_t env_id_offset;
  // ---- env state
  double *cur_pv, *cur_q, *cur_pl, *cur_ql, *q_new;   // [ns|nl][Bp]  MW / MVAr
  // gatherable state lives in ONE block `gbuf` (rows of Bp doubles) so obs/state columns are plain row
  // numbers: cur_pv cur_q [ns] | vm va res_p res_q [nb]   (pointers below alias into it)
  double* gbuf;
  double *vm, *va, *res_p, *res_q;                    // [nb][Bp] by bus id; va in rad
  double *pl;                                         // [n_line][Bp] res_line.pl_mw
  double *sum_rewards;                                // [Bp]
  int32_t* steps; int64_t* start_row; uint32_t* draw;
  uint8_t *done, *pending, *active, *commit, *bad_start, *resetting;   // resetting: (re)started by this step call (auto_reset)
  int64_t* adv_row; uint32_t* adv_draw;
  // ---- NR scratch (see NB_* / VO_*): row offsets of the Sbus and Vout regions
  double* nrbuf; uint32_t nrbuf_bytes; uint32_t sb_off, r_vout;   // sb_off: byte offset of the Sbus region the solve reads
  uint32_t sb_off_alt;                                            // ... of the other Sbus buffer (double-buffered, see k_advance)
  int32_t* iters; uint8_t* conv;
  // ---- NR schedule (k_nr_tree): W waves per workgroup, L envs per workgroup (64/L lane-group workers per wave), R rows
  int32_t nr_waves, nr_lanes, nr_rows, nr_cslots, nr_xslots, nr_nclist, nr_h_lds, nr_g_lds, nr_line_lds, nr_rec_lds, nr_flat_lds;
  const StepRec* sched; uint32_t sched_bytes; const int32_t* clist;
  const double* flat; uint32_t flat_bytes;   // Schedule::flat, [Wt][R][FLAT_N]
  // mismatch pass (k_nr_tree): per (worker, turn) a record with the node, its parent, its first three children in canonical
  // order, its Sbus entry and its Y constants (Schedule::mm_recs); further children of a junction from mm_ptr / mm_child
  const int32_t *mm_ptr, *mm_child; int32_t nr_mm_pass, mm_np;
  const StepRec* mm_recs; uint32_t mm_recs_bytes;   // Schedule::mm_recs
  // a Newton step whose largest component (|dtheta|, |d|V|/|V||) is below this predicts convergence: the next
  // forward sweep is first run in its mismatch-only form (k_nr_tree)
  double nr_check_dx;
  double nr_check_quad;      // safety factor of the quadratic-convergence predictor (inf disables it, tiny = always predict)
  // ---- general-topology solve (k_nr_dense, dense.hip): Ybus rows by position in CSR form (columns are positions,
  // n == slack; values (re, im)); the dense Jacobian is N x N (2n rounded up to 16) with row stride dn_lda in LDS
  // ---- general sparse path (k_nr_sparse, sparse.hip): host-compiled elimination program (plan.hpp SparseProg)
  int32_t sparse, sp_lanes, sp_blocks, sp_fill, sp_phases, sp_rows_per_sub, sp_max_nnz;
  const SpOp* sp_ops; uint32_t sp_ops_bytes; const SpNz* sp_nz; uint32_t sp_nz_bytes; const int32_t* sp_fill_slots;
  int32_t dense, dn_N, dn_lda;
  double* dn_A;              // k_nr_dense beyond 65 buses: per-env slabs [Bp][dn_N][dn_lda] of global memory for the Jacobian (else nullptr: LDS)
  const int32_t *gy_ptr, *gy_col; const double* gy_val;
  // ---- bus fusion (plan.hpp): original buses, nbo of them, vs electrical nodes (nb); all nullptr / 0 / nbo == nb without fusion
  int32_t nbo, n_fused, n_alias, n_slack_group;
  const int32_t *pos_of_obus, *cm_kind, *fused_obus, *ob_load_ptr, *ob_load_idx, *ob_sgen_ptr, *ob_sgen_idx, *slack_group, *alias_pos;
  const double *ob_shunt_p, *ob_shunt_q;
  // ---- PV-bus injection fused into the k_nr_tree prologue (step(), handles without auto_reset): per launch, set by launch_nr.
  // sgb_rec [n_sgb + n_mlo][8] = Sbus entry of the bus (-1: slack bus, q only) | elimination position | first sgen on the bus (-1:
  // a load-only bus with several loads) | (number of sgens << 8) | min(number of loads, 2) || first load | second load | 0 | 0
  const int32_t* sgb_rec;
  const void* fi_actions; int32_t fi_dtype;      // actions [B, ns] of MAPDN_F32 / MAPDN_F64; nullptr: the injection ran as its own launch
  // ---- DC-angle start (mapdn_env_config.nr_init = 2, runpp init="dc"; appended so that the fields above keep their kernarg offsets):
  // k_nr_tree<..., DC = true> sweeps dc_recs ([Wt][R], plan.hpp DcRec), k_nr_sparse<L, true> assembles SpNz::bdc; both add dc_pc
  int32_t nr_init;
  const DcRec* dc_recs; uint32_t dc_recs_bytes;
  const double* dc_pc;                           // [n] by position: Pbus - Re(Sbus) (plan.hpp Plan::dc_pc)
  // ---- voltage-dependent (ZIP) loads (mapdn_netspec.load_const_z / _i; appended like the DC fields): k_nr_tree<..., ZIP = true> and
  // k_nr_sparse scale Sbus_k by cp + ci |V_k| + cz |V_k|^2 after iteration 0; commit_bus reports the loads at the converged |V|
  int32_t zip;
  const double* zip_c; uint32_t zip_c_bytes;     // [n + 2][2] by position: (ci, cz) (plan.hpp Plan::zip_c)
  // ---- generators (mapdn_netspec.gen_*; appended likewise; plan.hpp Plan::n_gen ...).  n_gen: the bus injection (inject.hpp sbus_entry)
  // subtracts gen_p_pos from the demand and commit_bus writes res_gen_q and the gen bus's q_mvar.  gen_start: k_nr_tree<..., GEN = true> /
  // k_nr_sparse start from v0 and mask the blocks of the nodes flagged in is_gen (gen_mask.hpp)
  int32_t n_gen, gen_start;
  const uint8_t* is_gen;                         // [n + 2] by position
  const double *gen_p_pos, *v0;                  // [n + 2] by position: P_gen (MW; 0 elsewhere), start magnitude
  uint32_t v0_bytes;
  const int32_t *gen_of_pos, *gq_ptr, *gq_col;   // [n + 2] gen at a position or -1; CSR over the gens: their Ybus rows (columns: positions)
  const double* gq_val;                          // (re, im) per entry
  double* res_gen_q;                             // [n_gen][Bp] res_gen.q_mvar of the committed state
};

// ---- the bus injection every injecting kernel shares (inject.hpp: device functions on Dev)
}  // namespace mapdn
#include "inject.hpp"
namespace mapdn {

void launch_inject(const Dev& d, int mode, const void* actions, int dtype, const double* pl, const double* ql,
                   const double* pv, const double* q, int add_noise, hipStream_t st);
// step()/reset() form of the injection: PV buses only (the rest of Sbus is kept up to date by k_advance)
void launch_inject_sgen(const Dev& d, int mode, const void* actions, int dtype, int add_noise, hipStream_t st);
// fused_actions != nullptr (MODE_STEP only): k_nr_tree's prologue performs the PV-bus injection itself (no k_inject_sgen launch)
void launch_nr(const Dev& d, int mode, double* reward, uint8_t* term, double* info, hipStream_t st,
               const void* fused_actions = nullptr, int fused_dtype = 0);
// var: the variant — NR_VAR_DC the DC-angle-start instantiations (mapdn_env_config.nr_init = 2), NR_VAR_ZIP the voltage-dependent-load ones,
// NR_VAR_GEN the ones for nets with generators (gen buses; never together with ZIP)
enum { NR_VAR_DC = 1, NR_VAR_ZIP = 2, NR_VAR_GEN = 4 };
int nr_set_lds_limit(int waves, int lanes, int h_lds, int g_lds, int rec_lds, int flat_lds, size_t bytes, int var = 0);   // -2: geometry not instantiated
int nr_geometry_compiled(int waves, int lanes, int h_lds, int g_lds, int rec_lds, int flat_lds, int var = 0);
// the instantiation launch_nr runs for this geometry / residency / variant (nullptr: none; host-side, mapdn_get_nr_kernel)
struct NrInst;
const NrInst* nr_inst_of(int waves, int lanes, int h_lds, int g_lds, int rec_lds, int flat_lds, int var);
// dynamic LDS of k_nr_tree (W waves, L envs per workgroup => Wt = W*64/L workers), in pair rows of L x 16 bytes:
// node voltages (n+2: nodes, slack, trash), h (n+2) and G (2(n+2)) when resident, contribution slots (4 rows each),
// x slots (1 row each); then verdict bytes, step-size partials (64*W doubles), overflow child list (padded to
// 16 bytes), and — when they fit — the LineFlow constants of net.line for the fused res_line epilogue
__host__ __device__ static inline size_t nr_line_bytes(int n_line) { return ((size_t)n_line * sizeof(LineFlow) + 15) & ~(size_t)15; }
// The epilogue's partial sums (10 x 64*W doubles) re-use the contribution slots, so cslots >= nr_min_cslots(W, L).
static inline int nr_min_cslots(int W, int L) { return (10 * 64 * W + 8 * L - 1) / (8 * L); }
// rec_rows / flat_rows: R when the step records / flat-start constants of all Wt workers are staged in LDS, else 0
static inline size_t nr_lds_bytes(int W, int L, int n, int cslots, int xslots, int nclist, int h_lds, int g_lds, int n_line_lds,
                                  int rec_rows, int flat_rows) {
  const size_t rows = (size_t)(n + 2) * (1 + (h_lds ? 1 : 0) + (g_lds ? 2 : 0)) + (size_t)cslots * 4 + (size_t)xslots;
  const size_t Wt = (size_t)W * (64 / L);
  return rows * (size_t)L * 16 + (size_t)W * 64 + (size_t)64 * W * sizeof(double) + (size_t)((nclist + 3) & ~3) * sizeof(int32_t) +
         nr_line_bytes(n_line_lds) + Wt * rec_rows * sizeof(StepRec) + Wt * flat_rows * FLAT_N * sizeof(double);
}
// general sparse kernel (sparse.hip): L envs per one-wave workgroup; prepare returns -2 for an L that is not instantiated
size_t nr_sparse_lds_bytes(int n, int n_blocks, int L);
int nr_sparse_prepare(int L);
void launch_nr_sparse(const Dev& d, int mode, double* reward, uint8_t* term, double* info, hipStream_t st);
// general-topology kernel (dense.hip): the Jacobian of N rows lives in LDS up to 128 rows, beyond that in global memory (GA);
// nr_dense_waves is W of the k_nr_dense<W, GA> instantiation that serves it (0: none);
// nr_dense_prepare returns -2 when the net is too large for the LDS-resident Jacobian
static inline bool nr_dense_ga(int N) { return N > 128; }
int nr_dense_waves(int N, bool ga);
size_t nr_dense_lds_bytes(const Dev& d);
size_t nr_dense_lds_bytes(int N, int lda, int n);
int nr_dense_prepare(const Dev& d);
void launch_nr_dense(const Dev& d, int mode, double* reward, uint8_t* term, double* info, hipStream_t st);
int dense_solve_debug(const double* A, const double* b, double* x, int n, int batch, hipStream_t st);
void launch_reset_begin(const Dev& d, const int64_t* start_rows, int first_try, hipStream_t st);
void launch_advance(const Dev& d, int add_noise, int do_profiles, int do_commit, uint32_t sb_write_off, hipStream_t st);
// res_bus p_mw / q_mvar of the buses of fused groups (their OWN elements), after the solve and before the profile advance
void launch_commit_fused(const Dev& d, hipStream_t st);
void launch_gather(const Dev& d, const double* base, const int32_t* rows, const double* scales, double scale_all,
                   const int32_t* x_ptr, const int32_t* x_row, void* out, int dtype, int C, hipStream_t st);
void launch_to_envminor(const Dev& d, const double* src, double* dst, int n, hipStream_t st);
void launch_copy_i32(const int32_t* s, int32_t* dd, int B, hipStream_t st);
void launch_copy_u8(const uint8_t* s, uint8_t* dd, int B, hipStream_t st);
void launch_stats(const Dev& d, long long* out, hipStream_t st);

// ---- the traditional baselines: one control-loop frame (ctlloop.hpp: CtlLoop, the fields both loops keep) around the handle's solves
}  // namespace mapdn
#include "ctlloop.hpp"
#include "opf_sparse.hpp"   // OsM: the row table of k_opf_reduce_sparse
namespace mapdn {

// ---- droop baseline (droop.hip; mapdn_droop_actions, baselines_host.hpp).  Per-env status as in include/mapdn.h.
enum { DROOP_CONVERGED = 0, DROOP_MAX_ITER = 1, DROOP_PF_FAILED = 2, DROOP_STOPPED = CTL_STOPPED, DROOP_RUNNING = CTL_RUNNING };
struct DroopState : CtlLoop {
  double va, vb, vc, vd, damping, v_tol, ratio;
  double *v_last, *dv2;              // [ns][Bp]: |V| of the last solve, the terms (v - v_last)^2 of the stop test
  const int32_t* sg_vrow;            // [ns] row of nrbuf that holds |V| of sgen j's bus (Vout, VO_VM)
};
void launch_droop_update(const Dev& d, const DroopState& s, int iter, hipStream_t st);

// ---- OPF baseline (opf.hip, opf.hpp; mapdn_opf_actions, baselines_host.hpp).  Per-env status (opf.hpp OPF_*) as in include/mapdn.h.
struct OpfState : CtlLoop {
  double v_lower, v_upper, v_tol, step_tol;
  int32_t max_backtrack;
  // topology tables (by node position): parent, children in the canonical order of the sweeps (CSR), the node of every sgen's bus
  // (n: the slack), the Y / M constants (opf.hpp OY_*), the slack's own term of the loss
  const int32_t *par, *cptr, *cidx, *sg_node;
  const double* yt; double loss_slack;
  // workspace of the linearisation, env-minor: the block-LU factors [n][OPF_FAC], M V [n][2], dV and M dV [n][ns][2], S [n][ns],
  // H [ns][ns], g [ns]; of the QP: d [ns], y [ns + n], scratch (opf_qp_work)
  double *fac, *mv, *X, *W, *S, *H, *g, *qd, *qy, *qw;
  const double* a0;                  // [ns][Bp] the set-points the start launch begins from (clipped to [-1, 1]: mapdn_opf_probe), or nullptr: a = 0
  double *t, *loss, *viol, *loss_out, *viol_out;   // [Bp]: step length; loss (p.u.) and violation of the last solve / of a_sol
  int32_t* nback;                                   // [Bp] failed solves in a row
  uint8_t *lin, *qp_capped;                         // [Bp]; lin: linearised by the last launch
};
void launch_opf_update(const Dev& d, const OpfState& s, int iter, hipStream_t st);
void launch_opf_linearise(const Dev& d, const OpfState& s, hipStream_t st);
void launch_opf_qp(const Dev& d, const OpfState& s, hipStream_t st);
// ... on a k_nr_sparse handle (opf_sparse.hip, opf_sparse.hpp; mapdn_opf_config.meshed = 1), in place of launch_opf_linearise:
// k_opf_sens_sparse<sp_lanes> (S and dV by the handle's elimination program, two columns a run; the blocks of an env live in LDS,
// nr_sparse_lds_bytes) and k_opf_reduce_sparse (M V, loss, violation, lin, W, g, H with M from the row table OsM).  Of OpfState's tables
// they read sg_node and loss_slack; fac stays unallocated.
int opf_sparse_prepare(int L);       // -2: L is not instantiated
void launch_opf_linearise_sparse(const Dev& d, const OpfState& s, const OsM& m, hipStream_t st);

// ---- mapdn_evaluate_actions (whatif.hip, whatif.hpp; baselines_host.hpp whatif_run): K candidate actions per env scored in the frame.
// Per-(env, candidate) status as in include/mapdn.h: the values of the droop / OPF codes that apply.
enum { WHATIF_SOLVED = 0, WHATIF_PF_FAILED = 2, WHATIF_STOPPED = CTL_STOPPED };
struct WhatifState : CtlLoop {       // (vm_out here: [B][K][nbo], or nullptr; a_sol, n_active: not used)
  int32_t K;
  double *reward, *info;             // [B][K], [B][K][MAPDN_N_INFO]; nullptr (both): not written (mapdn_voltage_vjp)
  uint8_t* status_out;               // [B][K]
  int32_t* iters_out;                // [B][K] Newton iterations of the candidate's solve, or nullptr
};
void launch_whatif_start(const Dev& d, const WhatifState& s, const void* actions, int dtype, int k, hipStream_t st);
void launch_whatif_score(const Dev& d, const WhatifState& s, int k, hipStream_t st);

// ---- mapdn_action_gradients (grad.hip, grad.hpp; baselines_host.hpp grad_run): d reward / d action of every candidate, in the what-if
// frame.  Its own argument block: the tree tables of the OPF baseline, the frame's flags and action rows, its workspace and its output.
struct GradState {
  const int32_t *par, *cptr, *cidx, *sg_node;    // OpfState's topology tables (opf_tables)
  const double* yt;
  double *fac, *lam;                 // [n][OPF_FAC][Bp], [n][2][Bp] env-minor: the block-LU factors and c -> z -> lambda of one candidate
  const uint8_t *act, *nr_conv;      // [Bp] the frame's active set and the verdicts of its last solve
  const double* a;                   // [ns][Bp] the frame's action rows (the candidate k_whatif_start wrote)
  int32_t K;
  double* grad;                      // [B][K][ns] env-major
};
void launch_action_grad(const Dev& d, const GradState& s, int k, hipStream_t st);

// ---- mapdn_voltage_vjp (vjp.hip, vjp.hpp; baselines_host.hpp vjp_run): M cotangents over the bus voltages of every candidate times the
// Jacobian of those voltages by the actions, in the what-if frame.  Beside GradState (whose tables, workspace and frame rows it uses; its
// K and grad are not read): the caller's cotangents and outputs.
struct VjpState {
  int32_t K, M;
  const double *cot_vm, *cot_va;     // [B][K][M][nbo] env-major, or nullptr: zeros
  double* grad;                      // [B][K][M][ns] env-major (M == 0: not written)
  double* va_out;                    // [B][K][nbo] res_bus.va_degree of the candidate, or nullptr
};
void launch_voltage_vjp(const Dev& d, const GradState& s, const VjpState& v, int k, hipStream_t st);
void launch_vjp_mask(const Dev& d, int K, const void* actions, int dtype, const uint8_t* status, double* vm_pu, hipStream_t st);

// ---- mapdn_action_gradients on a k_nr_sparse handle (grad_sparse.hip, grad_sparse.hpp; mapdn_env_config.grad_meshed = 1): the same
// adjoint system solved by the handle's elimination program on transposed blocks.  Its own argument block beside GradState (whose act,
// nr_conv, a, sg_node, K and grad it reads): the transposed assembly stream, [S][rows_per_sub][max_nnz] like Dev::sp_nz with sizes of
// its own.  No workspace: the blocks, the right-hand side and lambda of an env live in LDS (nr_sparse_lds_bytes).
struct GradSparseState {
  const GsNz* nz; uint32_t nz_bytes;
  int32_t rows_per_sub, max_nnz;
};
int grad_sparse_prepare(int L);      // -2: L is not instantiated
void launch_action_grad_sparse(const Dev& d, const GradState& s, const GradSparseState& t, int k, hipStream_t st);

// ---- res_line / res_trafo (branch.hip, branch.hpp; mapdn_get_branch_results, mapdn_get_loading_summary).  Their own small argument
// blocks: Dev stays what every other launch takes.
enum { BR_TILE = 16, LS_WAVES = 8 };
struct BranchArgs {
  const BranchRec* rec;              // [n_line + n_trafo]: net.line rows, then the per-unit pi branches
  int32_t n_line, n_trafo, B;
  int32_t line_tiles, trafo_tiles;   // tiles of BR_TILE branches of each table (0: no column of the table is asked for)
  const double *vm, *va;             // |V| and angle of original bus b, env e at [b * sb + e * se]: env state (sb = Bp, se = 1, rad) or the
  int64_t sb, se;                    // caller's [B, n_bus] arrays (sb = 1, se = n_bus, degrees)
  double ang, sn;                    // angle unit -> rad (1 or pi / 180), sn_mva
  double* out[2][BC_N];              // columns of mapdn_branch_out (BC_*) of the line and the trafo table, [B, n] each or nullptr
};
struct LoadingArgs {
  const BranchRec* rec; int32_t n_branch, B, Bp;
  const double *vm, *va;             // env state [n_bus][Bp], va in rad
  double sn, limit;
  double* max_loading; int32_t* worst; int32_t* n_over;   // [B]
};
void launch_branch_results(const BranchArgs& a, int Bp, hipStream_t st);
void launch_loading_summary(const LoadingArgs& a, hipStream_t st);

}  // namespace mapdn
