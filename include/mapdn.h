/*
 * mapdn.h — C ABI of libmapdn_hip.so: batched MI355X (gfx950) implementation of the hot path of
 * Future-Power-Networks/MAPDN's VoltageControl environment.
 *
 * The reference has no FFI: the path sits behind a Python class
 *   VoltageControl(MultiAgentEnv)   environments/var_voltage_control/voltage_control_env.py:24
 * whose numeric work is `pp.runpp(self.powergrid)` (voltage_control_env.py:557, pandapower 2.7.0).
 * Each entry point below names the reference method(s) whose arithmetic it replaces, batched over
 * B independent env instances that share one network topology.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (MAPDN_E_*); mapdn_last_error() gives text;
 *     nothing throws across the boundary.
 *   - `mapdn_handle` is opaque; one handle == one (device, env batch).  The library owns topology
 *     constants, profile tables and workspace; THE CALLER OWNS EVERY I/O BUFFER and passes raw
 *     device pointers (e.g. torch.Tensor.data_ptr()) plus the hipStream_t to enqueue on
 *     (`void* stream`, NULL = default stream).
 *   - step-path calls only enqueue kernels; they never allocate and never synchronise.
 *   - batched I/O tensors are env-major C-contiguous: actions [B, ns], obs [B, n_agents, obs_size],
 *     state [B, state_size], voltages [B, nb], reward [B], terminated [B], info [B, 11].
 *   - one handle is used by one host thread at a time; handles are independent of each other.
 */
#ifndef MAPDN_H
#define MAPDN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAPDN_OK 0
#define MAPDN_E_INVALID (-1)   /* bad argument / inconsistent netspec                        */
#define MAPDN_E_TOPOLOGY (-2)  /* net not connected, or meshed and too large for a CU's LDS        */
#define MAPDN_E_HIP (-3)       /* HIP runtime error (no device, OOM, launch failure)           */
#define MAPDN_E_STATE (-4)     /* call order violated (e.g. step before set_profiles/reset)    */
#define MAPDN_E_NOMEM (-5)     /* host allocation failed (std::bad_alloc caught at the boundary)  */
#define MAPDN_E_INTERNAL (-6)  /* any other C++ exception caught at the boundary (text: mapdn_last_error) */

#define MAPDN_N_INFO 11        /* keys of `info`, voltage_control_env.py:586-606,621 — column order:
                                  percentage_of_v_out_of_control, percentage_of_lower_than_lower_v,
                                  percentage_of_higher_than_upper_v, totally_controllable_ratio,
                                  average_voltage_deviation, average_voltage, max_voltage_drop_deviation,
                                  max_voltage_rise_deviation, total_line_loss, q_loss, destroy */

/* voltage_barrier/voltage_barrier_registry.py:9-15 */
enum { MAPDN_BARRIER_L1 = 0, MAPDN_BARRIER_L2 = 1, MAPDN_BARRIER_COURANT_BELTRAMI = 2,
       MAPDN_BARRIER_BOWL = 3, MAPDN_BARRIER_BUMP = 4 };

/* bits of `state_space` (args/env_args/var_voltage_control.yaml:11) */
enum { MAPDN_SS_PV = 1, MAPDN_SS_DEMAND = 2, MAPDN_SS_REACTIVE = 4, MAPDN_SS_VM_PU = 8,
       MAPDN_SS_VA_DEGREE = 16, MAPDN_SS_ALL = 31 };

enum { MAPDN_F32 = 0, MAPDN_F64 = 1 };

/* The columns of the pandapower net (`model.p`, voltage_control_env.py:400-405) that runpp and the
 * env read.  Host pointers, copied during mapdn_create.  Bus ids are 0..n_bus-1. */
typedef struct mapdn_netspec {
  int32_t n_bus;
  const double* bus_vn_kv;          /* [n_bus]                                             */
  const int32_t* bus_zone;          /* [n_bus] 0 = "main", k = "zone{k}"  (bus.zone)       */
  int32_t n_line;                   /* net.line                                            */
  const int32_t* line_from_bus;
  const int32_t* line_to_bus;
  const double* line_r_ohm_per_km;
  const double* line_x_ohm_per_km;
  const double* line_c_nf_per_km;
  const double* line_g_us_per_km;
  const double* line_length_km;
  const int32_t* line_parallel;
  const uint8_t* line_in_service;
  int32_t n_branch_pu;              /* generic per-unit pi branches (e.g. trafos after T->pi) */
  const int32_t* br_from_bus;
  const int32_t* br_to_bus;
  const double* br_r_pu;
  const double* br_x_pu;
  const double* br_b_pu;
  const double* br_ratio;           /* 0 => 1                                              */
  const double* br_shift_deg;
  int32_t n_shunt;                  /* net.shunt (consumer sign, MW/MVAr at 1 p.u.)        */
  const int32_t* shunt_bus;
  const double* shunt_p_mw;
  const double* shunt_q_mvar;
  int32_t n_load;
  const int32_t* load_bus;          /* net.load.bus                                        */
  int32_t n_sgen;
  const int32_t* sgen_bus;          /* net.sgen.bus                                        */
  const int32_t* sgen_zone;         /* net.sgen.name as zone id (voltage_control_env.py:532) */
  int32_t ext_grid_bus;
  double ext_grid_vm_pu;
  double sn_mva;
  double f_hz;
  /* optional columns (NULL = default), appended so that zero-initialised older callers keep working */
  const double* br_g_pu;            /* [n_branch_pu] shunt conductance of the pi branch: ppc BR_B = br_b_pu - 1j*br_g_pu
                                       (a transformer's iron losses after pandapower's T->pi conversion); NULL = 0   */
  const double* load_scaling;       /* [n_load] net.load.scaling * in_service (pd2ppc: PD = sum p_mw * scaling); NULL = 1 */
  const double* sgen_scaling;       /* [n_sgen] net.sgen.scaling * in_service; runpp and res_sgen see p, q * scaling, the env
                                       (obs, q clip, :189) the raw table values; NULL = 1                               */
  const int32_t* bus_alias;         /* [n_bus] bus fusion — closed bus-bus switches (net.switch, et == "b"), which pd2ppc's bus lookup
                                       merges into ONE ppc bus: bus_alias[b] = the representative of b's group (itself for an unfused
                                       bus; representatives represent themselves).  Fused buses share the solved voltage but stay
                                       rows of everything the env reads: res_bus vm_pu / va_degree (equal within a group), their
                                       OWN p_mw / q_mvar (the ext_grid's injection on the ext_grid's own bus), zone frames,
                                       get_state, the reward's averages over all buses.  A branch between two buses of one group
                                       is refused.  NULL = no fusion                                                          */
  const double* load_const_z;       /* [n_load] voltage-dependent loads (runpp voltage_depend_loads=True): net.load.const_z_percent / 100 */
  const double* load_const_i;       /* [n_load] ... const_i_percent / 100.  NULL (either) = 0.  Each in [0, 1], cz + ci <= 1.  A load then
                                       draws S (cp + ci |V| + cz |V|^2), cp = 1 - ci - cz, in pandapower 2.x's scheme: the Newton
                                       mismatch after every voltage update uses Sbus_k (cp + ci |V_k| + cz |V_k|^2) with the bus's WHOLE
                                       net demand Sbus_k (loads minus sgens: the sgens of a ZIP bus are scaled too, makeSbus(vm=...)),
                                       while the first mismatch (iteration 0) uses the constant-power Sbus and the Jacobian has no load
                                       derivative (a chord-like Newton: iteration counts as runpp's).  res_bus p_mw / q_mvar of a ZIP bus
                                       = its loads x the polynomial at the converged |V| minus its sgens (unscaled), plus shunts.  The
                                       host reduces the columns to per-bus constants once per handle.  MAPDN_E_INVALID (with a message):
                                       loads at one bus with different fractions (runpp solves with their mean, reports each with its
                                       own), a ZIP load on the ext_grid bus, ZIP loads with bus_alias (fused buses) or with nr_solver =
                                       dense.  All-zero columns are the constant-power path.                                       */
  int32_t n_gen;                    /* generators (in-service rows of net.gen): each makes its bus a GEN BUS — |V| held at gen_vm_pu, P =
                                       gen_p_mw * gen_scaling injected (constant, no profile column), Q free (runpp's default
                                       enforce_q_lims=False: no limits).  Newton unknowns: theta on gen and PQ buses, |V| on PQ buses;
                                       ||F||inf runs over P of both kinds and Q of the PQ buses.  0 (with NULL columns) = the path of
                                       before.  Gens are not agents: obs / state sizes do not change, the gen bus's p_mw / q_mvar reach
                                       get_obs / get_state through res_bus.  MAPDN_E_INVALID (with a message): two gens on one bus, a gen
                                       on the ext_grid bus, gens with bus_alias (fused buses), with voltage-dependent loads or with
                                       nr_solver = dense.  mapdn_droop_actions / mapdn_opf_actions refuse such a handle.              */
  const int32_t* gen_bus;           /* [n_gen] net.gen.bus                                                                            */
  const double* gen_p_mw;           /* [n_gen] net.gen.p_mw                                                                           */
  const double* gen_vm_pu;          /* [n_gen] net.gen.vm_pu (> 0)                                                                    */
  const double* gen_scaling;        /* [n_gen] net.gen.scaling; NULL = 1                                                              */
  double vm_init_pu;                /* |V| every PQ bus starts from (runpp init_vm_pu="auto": the mean of the vm_pu of the ext_grid and of
                                       ALL net.gen rows, in service or not — so it is the caller's to give when the net holds
                                       out-of-service gens).  0 or NaN = the mean of ext_grid_vm_pu and gen_vm_pu[0 .. n_gen); with no
                                       gens that is ext_grid_vm_pu, the start of before.  The slack starts at its set-point and a gen bus
                                       at its own vm_pu; the DC-angle start (nr_init = 2) uses these magnitudes.                       */
} mapdn_netspec;

/* Constructor kwargs of VoltageControl (args/env_args/var_voltage_control.yaml:3-20). */
typedef struct mapdn_env_config {
  int32_t barrier_type;             /* MAPDN_BARRIER_*                                     */
  double voltage_weight;
  double q_weight;
  double line_weight;
  int32_t use_line_weight;          /* line_weight != None   (voltage_control_env.py:612)  */
  int32_t use_q_weight;             /* q_weight != None      (voltage_control_env.py:614)  */
  double v_lower, v_upper;
  int32_t episode_limit;
  double action_low, action_high;   /* bias -/+ scale (voltage_control_env.py:76)          */
  int32_t reset_action;
  int32_t state_space;              /* MAPDN_SS_* mask                                     */
  uint64_t seed;
  int64_t env_id_offset;            /* global id of local env 0 (multi-GPU sharding)       */
  int32_t auto_reset;               /* 0: a terminated env stays frozen (reward 0, terminated 1) until mapdn_reset — the
                                       batch analogue of "the caller resets" (models/model.py:204); 1: a terminated env
                                       starts its next episode by itself on the FOLLOWING mapdn_step call: that call
                                       ignores its action, performs reset() for it (sampled start, first profile row,
                                       random initial action; voltage_control_env.py:96-135) and reports reward 0,
                                       terminated 0, info 0 and mapdn_get_auto_reset_mask() == 1; `terminated` is
                                       therefore reported exactly once per episode                                  */
  /* ---- launch / solver tuning.  Appended fields, every one 0 = automatic, so that zero-initialised older callers keep
   * working and two handles in one process can differ (nothing below is process-global).  Results do not depend on the
   * GEOMETRY fields: bus voltages, iteration counts and observations are bit-identical in every geometry; reward / info are
   * sums over buses and lines formed from per-worker partials and agree to the last ulp.  For tools and A/B runs every
   * field has an environment-variable override that is read once, inside mapdn_create (named per field). */
  int32_t nr_solver;                /* 0 auto: tree kernel (k_nr_tree) for radial feeders, sparse block program (k_nr_sparse)
                                       for meshed nets; 1: k_nr_sparse on a radial net too (cross-checks); 2: k_nr_dense, the
                                       dense LU with f64 MFMA trailing updates (any topology; the Jacobian LDS-resident up to 65 buses,
                                       in per-env slabs of global memory up to 513 buses — an exhibit, not a fast path).
                                       env: MAPDN_NR_SPARSE=1 / MAPDN_NR_DENSE=1                                         */
  int32_t nr_waves;                 /* k_nr_tree: waves per workgroup, 0 auto | 1 | 2 | 4              env: MAPDN_NR_WAVES */
  int32_t nr_lanes;                 /* k_nr_tree: envs per workgroup,  0 auto | 4 | 8 | 16 | 32           env: MAPDN_NR_LANES
                                       (a (waves, lanes) pair that is not compiled in — csrc/nr_inst_list.hpp — is refused) */
  int32_t nr_lean;                  /* 0 auto | 1 lean: only voltages + hand-off slots in LDS, several workgroups per CU |
                                       2 fat: whatever fits of h, step records, flat-start constants, net.line constants, G
                                                                                                     env: MAPDN_NR_LEAN=1/0 */
  int32_t nr_h_lds, nr_g_lds, nr_rec_lds, nr_flat_lds, nr_line_lds;
                                    /* LDS residency of the h / G factors, the step records, the flat-start constants, the
                                       net.line constants: 0 auto (whatever fits, in that order) | 1 resident | 2 not resident
                                       env: MAPDN_NR_H_LDS, MAPDN_NR_G_LDS, MAPDN_NR_REC_LDS, MAPDN_NR_FLAT_LDS,
                                       MAPDN_NR_LINE_LDS = 1/0                                                             */
  int32_t nr_mm_pass;               /* the predicted-final mismatch evaluation: 0 auto (barrier-free pass over all nodes when h
                                       is LDS-resident) | 1 pass | 2 mismatch-only tree sweep (same bits) env: MAPDN_NR_MM_PASS */
  int32_t sp_lanes;                 /* k_nr_sparse: envs per workgroup, 0 auto (scored per net) | 16 | 8 | 4 | 2
                                                                                                       env: MAPDN_SP_LANES */
  int32_t inject_full;              /* 1: step() / reset() rebuild Sbus on every bus (k_inject) instead of on the PV buses only
                                       (k_inject_sgen); same bits, for A/B runs and tests               env: MAPDN_INJECT_FULL */
  double nr_check_dx;               /* Newton-step size below which the next sweep is first tried mismatch-only; 0 = 1e-7
                                       (never changes results)                                         env: MAPDN_NR_CHECK_DX */
  double nr_check_quad;             /* safety factor of the second predictor, ||F||^3 / ||F_prev||^2 < tol / factor; 0 = 1,
                                       +inf disables it                                              env: MAPDN_NR_CHECK_QUAD */
  int32_t debug_geometry;           /* 1: print the chosen NR geometry and LDS residency to stderr   env: MAPDN_DEBUG_GEOMETRY */
  /* ---- numerical options of runpp that DO change results (pp.runpp keyword arguments the reference leaves at their
   * defaults, voltage_control_env.py:557) */
  double tolerance_mva;             /* runpp(tolerance_mva=...): 0 = 1e-8 (the pandapower default)                          */
  int32_t tolerance_is_pu;          /* How the stopping rule of newtonpf is formed from tolerance_mva.  0 (default): ||F||inf <
                                       tolerance_mva / sn_mva, F in per unit — the rule as restated in oracle/pp_restated.py from
                                       pandapower 2.7.0 (`ppci_variables` / `_run_newton_raphson_pf`; UNPINNED: pandapower is not
                                       installable here).  1: ||F||inf < tolerance_mva with F in per unit (no division).  The two
                                       coincide on every net with sn_mva == 1 (all MAPDN scenarios and bench nets);
                                       tests/test_pandapower_pin.py::test_tolerance_rule_on_sn_mva_not_one decides which one
                                       pandapower uses wherever pandapower is installed                                    */
  int32_t nr_init;                  /* runpp(init=...): 0 "flat" — every solve starts at the slack set-point, what runpp's
                                       init="auto" does on a net without lines above 70 kV (exact pandapower iterates).
                                       2 "dc" — what init="auto" does when calculate_voltage_angles is on (a line at a bus above
                                       70 kV): every solve (step, reset, solve_only) starts from the angles of a DC power flow
                                       on the env's own injection, magnitudes at the slack set-point (pandapower run_dc_pf;
                                       mapdn_get_dc_angles).  Tree and sparse solvers; refused (MAPDN_E_INVALID) with
                                       nr_solver = dense and on a net with fused buses (bus_alias).  1 ("results": start a step() solve from the
                                       env's last accepted voltages, fall back to the flat start after 3 iterations) is RESERVED
                                       and refused (MAPDN_E_INVALID): the study that was to gate it (tools/history/warm_start_study.py,
                                       profiles/r04_warm_start_study_*.json: 3.6 M solves on the oracle, 15 % of them stressed
                                       to and beyond voltage collapse) found it SAFE — never "converged" where the flat start
                                       reports LoadflowNotConverged, never another root, |dV| < 1e-9 — but USELESS for this
                                       kernel: under i.i.d. actions (bench.py's workload) the previous voltages are no closer in
                                       Newton iterations than the flat start (mean 4.12 -> 4.23 iterations on the 141-bus feeder,
                                       4.56 -> 6.34 on the 33-bus one, with the fallback), and under a smooth policy only 43 % /
                                       79 % of the envs (141 / 322 buses) save an iteration, while a workgroup's 16 envs finish
                                       together: P(all 16 save one) ~ 0.  Not built.  Other values: MAPDN_E_INVALID.         */
  /* ---- composition of the step() launches (same results; A/B switches) */
  int32_t fuse_inject;              /* step(): 0 auto — the PV-bus injection (_clip_reactive_power, Sbus of the buses with sgens)
                                       runs inside the prologue of k_nr_tree when the handle uses the tree solver and has no
                                       auto_reset (one launch less per step); 1 same, refused (MAPDN_E_INVALID) when impossible;
                                       2 always its own launch (k_inject_sgen)                        env: MAPDN_FUSE_INJECT=1/0 */
  int32_t overlap_advance;          /* removed, must be 0 (MAPDN_E_INVALID otherwise); the field keeps the layout               */
  int32_t xcd_map;                  /* removed, must be 0 (MAPDN_E_INVALID otherwise); the field keeps the layout               */
  int32_t grad_meshed;              /* mapdn_action_gradients on handles of the general sparse solver (a meshed net, or a radial one
                                       with nr_solver = 1): 0 refused by name, as before | 1 answered — the adjoint system is solved
                                       by the handle's own elimination program on transposed blocks (k_action_grad_sparse, DESIGN.md
                                       section 24).  On a tree-solver handle 1 changes nothing (same launches, same bits).  Other
                                       values: MAPDN_E_INVALID.                                        env: MAPDN_GRAD_MESHED */
} mapdn_env_config;

typedef struct mapdn_dims_t {
  int32_t n_envs, n_bus, n_line, n_load, n_sgen, n_agents, n_actions, obs_size, state_size, n_info;
  int32_t is_radial;
  int32_t max_zone_size;
  int32_t n_gen;                    /* generators (mapdn_netspec.n_gen): the columns of mapdn_get_res_gen */
} mapdn_dims_t;

typedef struct mapdn_handle mapdn_handle;

/* last error text: of `h`, or of the last failed mapdn_create when h == NULL */
const char* mapdn_last_error(const mapdn_handle* h);

/* VoltageControl.__init__ up to (not including) data loading — voltage_control_env.py:36-94.
 * Builds per-unit Ybus (pandapower pd2ppc/makeYbus), the elimination order and all gather index
 * tables on the host, uploads them to `device`, allocates state for n_envs envs.
 * Topology: pp.runpp (voltage_control_env.py:557) solves any connected net.  Radial feeders (all three MAPDN
 * scenarios) take the fill-free tree solver; a meshed net (closed tie switches, loops) takes the general sparse solver:
 * symbolic factorisation with fill on the host, the numeric part as a program of 2x2 block operations interpreted with
 * all blocks of a few envs in LDS (nets up to ~2400 blocks after fill: the 322-bus case with tie lines fits).
 * Nets beyond that and nets with buses not connected to the ext_grid return MAPDN_E_TOPOLOGY.
 * device == -1 builds a host-only handle (plan, dims, ybus/obs-index export; no device calls).
 * Launch geometry and solver choice: automatic per topology and batch size; mapdn_env_config's tuning fields (and, for tools,
 * their environment-variable overrides) select them explicitly.  mapdn_get_nr_geometry() reports what was chosen. */
int mapdn_create(const mapdn_netspec* net, const mapdn_env_config* cfg, int32_t n_envs,
                 int32_t device, mapdn_handle** out);
void mapdn_destroy(mapdn_handle* h);
int mapdn_dims(const mapdn_handle* h, mapdn_dims_t* out);

/* _load_pv_data/_load_active_demand_data/_load_reactive_demand_data (voltage_control_env.py:407-438)
 * after CSV parsing and *_scale: HOST row-major tables pv [T, ns], load_p [T, nl], load_q [T, nl].
 * Also derives the per-column std/100 (:70-72) and s_max = 1.2*max (:515-520).  Synchronous. */
int mapdn_set_profiles(mapdn_handle* h, const double* pv, const double* load_p, const double* load_q,
                       int64_t n_rows, int32_t time_delta_min, int32_t days);

/* Host-side export of what mapdn_set_profiles derived from the tables (parity tests): stdv [n_sgen + 2 n_load] = the per-column noise
 * scale `values.std(axis=0) / 100.0` in table order pv | load_p | load_q (voltage_control_env.py:70-72, numpy's own summation order:
 * csrc/colstats.hpp), smax [n_sgen] = 1.2 * max_t pv (:518-520).  HOST pointers; either may be NULL. */
int mapdn_get_profile_stats(const mapdn_handle* h, double* stdv, double* smax);

/* reset() / manual_reset() — voltage_control_env.py:96-176.  start_rows: device int64 [B] giving
 * `start` of :445 per env, or NULL to sample (hour, day, interval) per env from the keyed RNG.
 * Retries unsolvable initial states up to `max_tries` times (reference: unbounded loop, :108). */
int mapdn_reset(mapdn_handle* h, const int64_t* start_rows, int32_t add_noise, int32_t max_tries,
                void* stream);

/* step(actions, add_noise) — voltage_control_env.py:178-211 (= _take_action :548-566 with the
 * pandapower runpp inside, _calc_reward :574-623, _set_demand_and_pv :491-513).
 * actions: device [B, ns] of actions_dtype; reward f64 [B]; terminated u8 [B]; info f64 [B, 11].
 * Envs already terminated are frozen: reward 0, terminated 1, info unchanged (zeros). */
int mapdn_step(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t add_noise,
               double* reward, uint8_t* terminated, double* info, void* stream);

/* step() immediately followed by get_obs(), the pair every caller of the reference issues (models/model.py:216,219;
 * utilities/tester.py:48-49) as one call: the same four launches as mapdn_step + mapdn_get_obs, one host entry.
 * (A single fused post-solve kernel — commit + profile advance + gather out of an LDS tile — was built and measured:
 * 29.5 us against 26.3 us for the two wide launches on case141 x 4096; not kept, see DESIGN.md.)
 * obs: device [B, n_agents, obs_size] of obs_dtype. */
int mapdn_step_obs(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t add_noise,
                   double* reward, uint8_t* terminated, double* info, void* obs, int32_t obs_dtype, void* stream);

/* get_obs() — voltage_control_env.py:232-316 (distributed mode): [B, n_agents, obs_size]. */
int mapdn_get_obs(mapdn_handle* h, void* obs, int32_t dtype, void* stream);
/* get_state() — voltage_control_env.py:213-230: [B, state_size]. */
int mapdn_get_state(mapdn_handle* h, void* state, int32_t dtype, void* stream);

/* tester getters — voltage_control_env.py:625-647; any pointer may be NULL.
 * vm_pu, va_degree, p_mw, q_mvar: f64 [B, nb]; pl_mw: f64 [B, n_line]; sgen_p, sgen_q: f64 [B, ns] */
int mapdn_get_results(mapdn_handle* h, double* vm_pu, double* va_degree, double* p_mw, double* q_mvar,
                      double* pl_mw, double* sgen_p, double* sgen_q, void* stream);
/* current load table values f64 [B, nl] (net.load.p_mw / q_mvar) */
int mapdn_get_loads(mapdn_handle* h, double* load_p, double* load_q, void* stream);

/* ---- res_line / res_trafo: the branch tables the reference reads from pandapower after every runpp — res_line.loading_percent,
 * i_from_ka, i_to_ka (environments/var_voltage_control/pf_res_plot.py:142-150) and res_trafo.loading_percent, i_hv_ka, i_lv_ka
 * (pf_res_plot.py:161-163) — restated from pandapower 2.7.0 results_branch.py (_get_line_results, _get_trafo_results with
 * trafo_loading="current") [PP-recalled].  With Sf = Vf conj(yff Vf + yft Vt), St = Vt conj(ytf Vf + ytt Vt) in per unit (the pi constants of
 * makeYbus): p_from_mw + j q_from_mvar = Sf sn_mva, p_to_mw + j q_to_mvar = St sn_mva; pl_mw / ql_mvar = Re / Im (Sf + St) sn_mva in the
 * four-term form of the res_line.pl_mw that mapdn_get_results reports; i_from_ka = |Sf| sn_mva / (sqrt(3) |Vf| bus_vn_kv[from]), i_to_ka
 * likewise, i_ka their maximum (|S| == 0 gives 0); loading_percent = 100 i_ka / (max_i_ka df parallel) of a line and
 * 100 sqrt(3) max(i_hv_ka vn_hv_kv, i_lv_ka vn_lv_kv) / br_rating_mva of a per-unit pi branch (a transformer: from = hv, to = lv).
 * An out-of-service line reports 0 in every column; a branch without a rating reports loading_percent = NaN.
 *
 * Ratings: HOST arrays, any of them NULL, copied and uploaded once (synchronous; on a host-only handle only validated).
 * line_max_i_ka, line_df [n_line] = net.line.max_i_ka, net.line.df (NULL df: 1; net.line.parallel is the netspec's); br_vn_hv_kv,
 * br_vn_lv_kv [n_branch_pu] = the transformer's nameplate voltages; br_rating_mva [n_branch_pu] = its sn_mva x parallel x df.  A NULL
 * line_max_i_ka leaves every line unrated, a NULL among the three br_ columns every pi branch; a NaN in line_max_i_ka / br_rating_mva
 * leaves that row unrated (pandapower's missing value).  Any other entry that is not finite and > 0 is MAPDN_E_INVALID, named by
 * column and row.  A call replaces the ratings of the call before. */
int mapdn_set_branch_ratings(mapdn_handle* h, const double* line_max_i_ka, const double* line_df,
                             const double* br_vn_hv_kv, const double* br_vn_lv_kv, const double* br_rating_mva);

typedef struct mapdn_branch_out {            /* device f64, any pointer NULL */
  double *p_from_mw, *q_from_mvar, *p_to_mw, *q_to_mvar, *pl_mw, *ql_mvar,
         *i_from_ka, *i_to_ka, *i_ka, *loading_percent;
} mapdn_branch_out;

/* The two tables for every env in one launch (k_branch_results), only the columns whose pointer is not NULL; `line` / `trafo` may be NULL.
 * vm_pu, va_degree: device f64 [B, n_bus] by bus — what mapdn_get_results and mapdn_solve_only write — and the tables are computed at
 * those voltages: env state is neither read nor touched (fused buses: the caller's own rows of the two ends are read).  Both NULL: the
 * env's current vm / va (MAPDN_E_STATE before mapdn_reset); exactly one NULL: MAPDN_E_INVALID.  Enqueues only. */
int mapdn_get_branch_results(mapdn_handle* h, const double* vm_pu, const double* va_degree,
                             const mapdn_branch_out* line,   /* [B, n_line]      */
                             const mapdn_branch_out* trafo,  /* [B, n_branch_pu], from = hv, to = lv */
                             void* stream);

/* Per env, over the rated in-service branches at the env's current state, lines numbered 0 .. n_line - 1 and pi branches from n_line:
 * max_loading f64 [B] = the largest loading_percent, worst_branch i32 [B] = the lowest index that attains it (-1, with max_loading = NaN
 * and n_overloaded = 0, when nothing is rated), n_overloaded i32 [B] = the count of loading_percent > limit_percent.  One launch
 * (k_loading_summary) from the voltages; the bits do not depend on the batch size.  Device pointers; MAPDN_E_STATE before mapdn_reset. */
int mapdn_get_loading_summary(mapdn_handle* h, double limit_percent,
                              double* max_loading /*[B]*/, int32_t* worst_branch /*[B]*/,
                              int32_t* n_overloaded /*[B]*/, void* stream);

/* `start` of voltage_control_env.py:445 for every env: device int64 [B] */
int mapdn_get_start_rows(mapdn_handle* h, int64_t* start_rows, void* stream);

/* sum_rewards of the running episode (voltage_control_env.py:203) for every env: device f64 [B] */
/* uint8 [n_envs]: 1 for the envs that the last mapdn_step call (re)started (auto_reset == 1), else 0.  An env whose restart
 * power flow does not solve is NOT reported here: it stays frozen (reward 0, terminated 1) and draws a new start on the next
 * call, like the reference's `while not solvable` loop (voltage_control_env.py:108); until then its load / PV tables already
 * hold the rejected start's values while res_bus still holds the previous episode's voltages. */
int mapdn_get_auto_reset_mask(mapdn_handle* h, uint8_t* mask, void* stream);

int mapdn_get_returns(mapdn_handle* h, double* returns, void* stream);

/* Pure power flow == pp.runpp(net) (voltage_control_env.py:557) on explicit element powers:
 * p_load, q_load f64 [B, nl]; p_sgen, q_sgen f64 [B, ns] (MW / MVAr) ->
 * vm_pu, va_degree f64 [B, nb]; iterations i32 [B]; converged u8 [B].  Does not touch env state. */
int mapdn_solve_only(mapdn_handle* h, const double* p_load, const double* q_load, const double* p_sgen,
                     const double* q_sgen, double* vm_pu, double* va_degree, int32_t* iterations,
                     uint8_t* converged, void* stream);

/* Host-side debug export of the per-unit admittance matrix the library built (for parity tests):
 * dense row-major complex [nb, nb] as (re, im) pairs (with fused buses — bus_alias — over the merged nodes: nb = the number of
 * representatives, in ascending order of their bus index). */
int mapdn_get_ybus_dense(const mapdn_handle* h, double* ybus_re_im);
/* Host-side export of the integer gather tables of get_obs: kind/index per obs column
 * [n_agents*obs_size] (kinds: 0 zero pad, 1 p_mw, 2 q_mvar, 3 pv, 4 q, 5 vm_pu, 6 va rad). */
int mapdn_get_obs_index(const mapdn_handle* h, int32_t* kind, int32_t* index);

/* Host-side export of the NR elimination schedule for W cooperating waves (plan check, CPU tests):
 * rows [W * (*n_rows)] node position per (wave, row) or -1, parent [n] parent position per node
 * (n = n_bus-1 means the slack).  Call with rows == NULL to query *n_rows first. */
int mapdn_get_schedule(const mapdn_handle* h, int32_t n_waves, int32_t* n_rows, int32_t* rows, int32_t* parent);

/* Host-side export of the launch geometry mapdn_create settled on (also for device == -1 handles, which assume a 256-CU
 * device): out[20] = solver (0 tree, 1 sparse, 2 dense), waves, lanes (envs per workgroup), lean, schedule rows, h_lds, g_lds,
 * rec_lds, flat_lds, line_lds, mm_pass, dynamic LDS bytes per workgroup, workgroups, workgroups resident per CU (model),
 * rounds of workgroups, modelled launch time in ns (the chooser's score; 0 when the geometry was forced), fuse_inject (1: step()
 * performs the PV-bus injection in the solver's prologue), number of buses in fused groups (bus_alias), electrical nodes, nr_init
 * (0 flat start, 2 DC-angle start). */
int mapdn_get_nr_geometry(const mapdn_handle* h, int32_t* out20);

/* Host-side export of the DC-angle start (nr_init = 2, runpp init="dc"; plan check, CPU tests): the angles va_rad [n_bus] (rad, slack 0)
 * that the solvers start from for the net bus demand p_bus_demand_mw [n_bus] (MW, consumer sign: loads minus sgens after scaling),
 * computed on the host from the handle's plan constants in the solver's own order of operations — the tree sweeps of k_nr_tree, or
 * the block program of k_nr_sparse on the Bbus assembly.  Solves Bbus[pvpq, pvpq] Va[pvpq] = Pbus[pvpq] with
 * Bbus = (Cf - Ct)' diag(1 / (x |tap|)) (Cf - Ct), Pbus = -P_demand / sn_mva - (Cf - Ct)' (b (-shift)) - GS / sn_mva (pandapower
 * run_dc_pf).  The generators' P (mapdn_netspec.gen_p_mw * gen_scaling) is subtracted from the demand of their buses here, as the
 * injection does: p_bus_demand_mw holds loads minus sgens only.  HOST pointers; works on host-only handles.  MAPDN_E_INVALID on a net
 * with fused buses. */
int mapdn_get_dc_angles(const mapdn_handle* h, const double* p_bus_demand_mw, double* va_rad);

/* Host-side export of the flat-start factorisation the NR kernel's first iteration uses (plan check, CPU tests):
 * factors [n][12] per elimination position = S_calc (re, im), D^-1 (4, row-major), A_pk (re, im), G (4, row-major)
 * of the block LU of the Jacobian at the start of runpp's init="auto" — the slack at ext_grid vm_pu, every gen bus at its own vm_pu,
 * every other bus at mapdn_netspec.vm_init_pu (without generators: ext_grid vm_pu everywhere), all angles 0 — unknowns
 * [dtheta, d|V|/|V|], the block of a gen bus masked (csrc/gen_mask.hpp: D^-1 = [[1 / D0, 0], [0, 1]], second row of G zero);
 * bus_of_pos [n+1] (optional) = bus id of every elimination position (position n is the slack). */
int mapdn_get_flat_factors(const mapdn_handle* h, double* factors, int32_t* bus_of_pos);

/* res_gen of the env's committed state (pandapower results_gen): DEVICE f64 [n_envs, n_gen] each, any pointer NULL —
 * p_mw = gen_p_mw * gen_scaling, q_mvar = Im(V_k conj((Ybus V)_k)) sn_mva + QD_k (QD: the bus's loads - sgens + shunt q |V|^2),
 * vm_pu and va_degree those of the gen's bus.  Rolled back with the rest of the state after an unsolvable step.  A handle without
 * generators writes nothing.  MAPDN_E_STATE before the first reset. */
int mapdn_get_res_gen(mapdn_handle* h, double* p_mw, double* q_mvar, double* vm_pu, double* va_degree, void* stream);

/* Host-side export of the general sparse solver's elimination PROGRAM for S sub-lanes (plan check, CPU tests): dims [6] =
 * block slots, fill-only blocks, phases, assembly rows per sub-lane, max row entries, number of off-diagonal blocks;
 * ops [phases * S * 4] = (type, c, a, b) with (type & 255) 0 NOP, 1 B[c] = inv(B[a]), 2 B[c] = B[a] B[b], 3 B[c] -= B[a] B[b]
 * (bits 8 / 9 of type: wave-uniform hints "this phase holds an INV / an UPD")
 * (block slots: diagonal of node i = i, right-hand side of node i = n + i as the block [b | 0]); order [n] = minimum-degree
 * elimination order (positions); slots_ij [3 * dims[5]] = (i, j, slot) of every off-diagonal block incl. fill.  Executing the
 * ops in phase order on the assembled blocks solves J x = b — tests/test_general_topology.py does it in numpy against
 * scipy's spsolve (what pandapower calls in pypower/newtonpf.py).  Any pointer but dims may be NULL. */
int mapdn_get_sparse_program(const mapdn_handle* h, int32_t sub_lanes, int32_t* dims, int32_t* ops, int32_t* order, int32_t* slots_ij);

/* Debug / pin export of the general solver's linear algebra: solves `batch` independent dense systems A x = b
 * (device pointers; A row-major [batch, n, n], b and x [batch, n]; n even, <= 1024; LDS-resident up to n = 128, in global scratch —
 * synchronous — beyond) with the blocked LU
 * (2x2 block pivots, v_mfma_f64_16x16x4_f64 trailing updates) that k_nr_dense runs on the Jacobian — what pandapower
 * does with SuperLU in pypower/newtonpf.py (dx = -spsolve(J, F)).  Tests compare with numpy.linalg.solve. */
int mapdn_dense_solve(const double* a, const double* b, double* x, int32_t n, int32_t batch, void* stream);

/* Rollout-side forward of the shared-parameter recurrent agent (agents/rnn_agent.py:5-32 as called by
 * models/model.py:101-139): fc1 (+ one-hot agent-id column) -> LayerNorm -> ReLU -> GRUCell -> fc2, one launch, inference only.
 * Device pointers, fp32, contiguous: obs [rows, obs_dim] (rows = envs x agents, agent = row % n_agents), hid_in / hid_out
 * [rows, 64], w1 [64, obs_dim + id_dim] (id_dim = n_agents or 0), w_ih / w_hh [192, 64] (torch.nn.GRUCell layout: r, z, n),
 * w2 [1, 64]; means [rows].  Hidden size 64, action_dim 1 (the reference's defaults).  hid_out may be NULL (the new hidden state is not stored).
 * Arithmetic: every product is an fp32 fmaf chain on the matrix cores, LayerNorm as the modules'; the GRU gates are
 * sigmoid(v) = rcp(1 + exp(-v)) and tanh(v) = 1 - 2 rcp(exp(2 v) + 1) on the hardware exp / rcp (~1e-7 absolute error each, finite
 * and saturating for any finite v), not the library's division and tanhf — so means / hid_out follow the f32 modules to a few 1e-7,
 * not bit for bit; DESIGN.md ("Learner kernels against float64") holds the errors measured per launch geometry and over a 240-step
 * recurrent episode.  MAPDN_POLICY_FWD_V1=1 (read at every call) selects the earlier form of the kernel (division + tanhf gates). */
int mapdn_policy_forward(const float* obs, const float* hid_in, const float* w1, const float* b1, const float* ln_g,
                         const float* ln_b, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                         const float* w2, const float* b2, float* means, float* hid_out, int32_t rows, int32_t n_agents,
                         int32_t obs_dim, int32_t id_dim, float ln_eps, void* stream);

/* The same launch for the learner's TRAINING-time forward (models/maddpg.py:103-125 through agents/rnn_agent.py:16-32): also writes
 * x1 [rows, 64] = fc1(obs) + b1 + id column (the LayerNorm input, all the backward keeps); hid_out may be NULL (not stored). */
int mapdn_policy_forward_train(const float* obs, const float* hid_in, const float* w1, const float* b1, const float* ln_g,
                               const float* ln_b, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                               const float* w2, const float* b2, float* means, float* hid_out, float* x1_out, int32_t rows,
                               int32_t n_agents, int32_t obs_dim, int32_t id_dim, float ln_eps, void* stream);
/* Backward of the agent's trunk LayerNorm -> ReLU -> GRUCell -> fc2 (agents/rnn_agent.py:16-32) for d loss / d means [rows], one launch
 * (csrc/policy_bwd.hip) that recomputes the trunk from x1 and hid_in and writes what the remaining weight-gradient products need:
 *   dx1 [rows, 64] = d loss / d x1 (-> fc1: dW1 = dx1^T [obs | id], db1);
 *   dgates [rows, 256] = d loss / d gate pre-activations  r | z | n_input | n_hidden  (torch.nn.GRUCell: dW_ih = dgates[:, 0:192]^T xn,
 *                        dW_hh = dgates[:, [0:128, 192:256]]^T hid_in);  xn [rows, 64] = relu(LayerNorm(x1));
 *   small [512] = db_r | db_z | db_ni | db_nh | dgamma | dbeta | dw2 (64 each) | db2 (1) + pad, reduced in a fixed order (no atomics):
 *                 b_ih gradient = db_r | db_z | db_ni, b_hh gradient = db_r | db_z | db_nh;
 *   scratch: mapdn_policy_backward_scratch_floats(rows) floats.  Hidden size 64, one action output; fp32, contiguous device pointers.
 * Pad rule (this call and mapdn_critic_head_backward / _mse alike): the pad elements of an OUTPUT (small[449 .. 511], grads[4354 .. 4415])
 * are written as zero; `scratch` need not be initialised — its pad columns are neither read nor written, every other element is written
 * before it is read. */
int64_t mapdn_policy_backward_scratch_floats(int64_t rows);
int mapdn_policy_backward(const float* dmeans, const float* x1, const float* hid_in, const float* ln_g, const float* ln_b, float ln_eps,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* w2, float* dx1,
                          float* dgates, float* xn, float* small, float* scratch, int64_t rows, void* stream);

/* 1 when mapdn_policy_forward has a launch shape for this observation width (the parameter set and a tile's activations must
 * fit the 160 KB LDS of a CU: obs_dim up to ~2 400 columns without ids), else 0 — callers then keep their own forward. */
int mapdn_policy_forward_fits(int32_t obs_dim, int32_t id_dim);
/* The launch shape behind that answer (host only, no device needed; returns what mapdn_policy_forward_fits returns): threads per
 * workgroup (512 / 256 = k_policy_fwd2<512> / <256>, or k_policy_fwd<...> under MAPDN_POLICY_FWD_V1), whether the id columns of fc1 are
 * staged in LDS, and the dynamic LDS in bytes; all three 0 when nothing fits.  Any pointer may be NULL.  The launch calls the same function. */
int mapdn_policy_forward_geometry(int32_t obs_dim, int32_t id_dim, int32_t* threads, int32_t* ids_lds, int32_t* lds_bytes);

/* LayerNorm over 64 features (+ fused ReLU when relu != 0) for the learner's training-time passes (agents/rnn_agent.py:16-21,
 * critics/mlp_critic.py:22-27: fc1 -> LayerNorm -> ReLU), forward and backward; device pointers, fp32, contiguous [rows, 64].
 * forward also writes the row statistics (mean, rstd [rows]) the backward needs.  backward: dx [rows, 64], dgamma, dbeta [64];
 * `partial` is scratch of mapdn_layernorm64_backward_blocks(rows) x 128 floats (block partial sums, reduced in a fixed order:
 * deterministic, no atomics). */
int mapdn_layernorm64_forward(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                              int64_t rows, float eps, int32_t relu, void* stream);
int mapdn_layernorm64_backward_blocks(int64_t rows);
int mapdn_layernorm64_backward(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                               const float* rstd, float* dx, float* dgamma, float* dbeta, float* partial, int64_t rows,
                               int32_t relu, void* stream);
/* ... with every input row FORMED as base[row / n] + per_n[row % n] instead of read (base [rows / n][64], per_n [n][64], rows a multiple
 * of n): the central critic's first layer feeds the LayerNorm  W_obs·obs_all + b  per batch element plus the id column of the agent
 * (critics/mlp_critic.py:22-27 behind models/maddpg.py:35-79), and the [batch, agents, 64] tensor of their sum is never materialised.
 * _bc_backward returns dx per formed row; the caller reduces it over the agents / over the batch. */
int mapdn_layernorm64_bc_forward(const float* base, const float* per_n, int32_t n, const float* gamma, const float* beta, float* y,
                                 float* mean, float* rstd, int64_t rows, float eps, int32_t relu, void* stream);
int mapdn_layernorm64_bc_backward(const float* dy, const float* base, const float* per_n, int32_t n, const float* gamma, const float* beta,
                                  const float* mean, const float* rstd, float* dx, float* dgamma, float* dbeta, float* partial,
                                  int64_t rows, int32_t relu, void* stream);
/* The critic's last two steps on rows of 64 as one pass: v[row] = relu(pre[row, :]) . w + bias  (critics/mlp_critic.py:22-36: the
 * activation after fc2, then fc3 with one output) — relu(pre) is not materialised.  Backward: dpre = [pre > 0] dv w; dw [64]; db [64]
 * with the bias gradient in db[0]; `partial` = mapdn_layernorm64_backward_blocks(rows) x 128 floats of scratch (fixed-order reduction). */
int mapdn_relu_dot64_forward(const float* pre, const float* w, float bias, float* v, int64_t rows, void* stream);
int mapdn_relu_dot64_backward(const float* dv, const float* pre, const float* w, float* dpre, float* dw, float* db, float* partial,
                              int64_t rows, void* stream);

/* The critic trunk behind its first layer as ONE launch each way (critics/mlp_critic.py:22-36 as trained by
 * learning_algorithms/ddpg.py:15-39 / models/maddpg.py:103-125):   v[row] = relu( relu(LayerNorm(x[row])) W2^T + b2 ) . w3 + b3
 * on rows of 64, fp32 on v_mfma_f32_16x16x4_f32 (csrc/critic.hip).  x is read ([rows][64], per_n == NULL) or FORMED as
 * base[row / n] + per_n[row % n] (x = base [rows / n][64], per_n [n][64], rows a multiple of n, n <= 256: the central critic).
 * Device pointers, contiguous; gamma, beta, b2, w3 [64], w2 [64][64] (out, in), b3 [1]; rows < 2^31.
 * backward recomputes the forward from the same inputs (nothing is saved but them):
 *   dx      [rows][64]                       (x read)   — or dbase [rows / n][64] = sum of dx over every group of n rows (x formed);
 *   grads   [4416 (+ n * 64)] when param_grads != 0 or x is formed:  dW2 [64][64] | dgamma | dbeta | db2 | dw3 [64 each] | db3 [1] |
 *           [4353] the loss of _mse (0 otherwise) | pad to 4416, written as zero | dper_n [n][64] (formed rows only; with param_grads == 0
 *           only dper_n is written);
 *   scratch mapdn_critic_head_scratch_floats(rows, n, formed) floats (per-workgroup partial sums — the wavefronts of a workgroup are summed through LDS —, reduced in a fixed order: deterministic).
 * _backward_dot: only dact[row] = dx[row] . dot_w[row % n] (dot_w [n][64]; n = 1 when x is read) — the policy update through the
 * central critic, whose own-action column of fc1 (models/maddpg.py:52-58) is the only gradient path back to the policy. */
int mapdn_critic_head_forward(const float* x, const float* per_n, int32_t n, const float* gamma, const float* beta, float eps,
                              const float* w2, const float* b2, const float* w3, const float* b3, float* v, int64_t rows, void* stream);
int64_t mapdn_critic_head_scratch_floats(int64_t rows, int32_t n, int32_t formed);
/* The backward launch for (rows, n, formed, mode) — mode 0 _backward(param_grads = 1), 1 _backward(param_grads = 0), 2 _backward_dot,
 * 3 _mse: k_head_bwd<formed, mode, threads> on `blocks` workgroups with `lds_bytes` of dynamic LDS.  cus = 0 asks the current device for
 * its CU count; cus > 0 answers for that count on the host alone.  Honours MAPDN_HEAD_BWD_THREADS (256 / 512; 512 only where its LDS
 * fits).  MAPDN_E_INVALID for arguments or an LDS need the launch refuses.  The launch calls the same functions. */
int mapdn_critic_head_backward_geometry(int64_t rows, int32_t n, int32_t formed, int32_t mode, int32_t cus, int32_t* threads,
                                        int32_t* blocks, int32_t* lds_bytes);
int mapdn_critic_head_backward(const float* dv, const float* x, const float* per_n, int32_t n, const float* gamma, const float* beta,
                               float eps, const float* w2, const float* b2, const float* w3, const float* b3, float* dx, float* grads,
                               float* scratch, int64_t rows, int32_t param_grads, void* stream);
/* the value loss of the DDPG family (learning_algorithms/ddpg.py:36-38) and every gradient of it in ONE launch, without a forward:
 * loss = sum_rows scale[0] * wrow[row / n] * (ret[row] - v[row])^2 (wrow NULL: 1; wrow [rows / n], or [rows] when x is read) -> grads[4353];
 * dx / dbase and grads as mapdn_critic_head_backward(param_grads = 1) for dv = d loss / d v. */
int mapdn_critic_head_mse(const float* ret, const float* wrow, const float* scale, const float* x, const float* per_n, int32_t n,
                          const float* gamma, const float* beta, float eps, const float* w2, const float* b2, const float* w3,
                          const float* b3, float* dx, float* grads, float* scratch, int64_t rows, void* stream);
int mapdn_critic_head_backward_dot(const float* dv, const float* x, const float* per_n, int32_t n, const float* gamma, const float* beta,
                                   float eps, const float* w2, const float* b2, const float* w3, const float* b3, const float* dot_w,
                                   float* dact, int64_t rows, void* stream);

/* MATD3's twin critic (models/matd3.py:35-86: ONE critic valued twice, with one more input column that is 0 for values1 and 1 for
 * values2) behind its first layer as ONE launch over both heads (csrc/critic_twin.hip): the formed row of the central critic,
 * x1[row] = base[row / n] + per_n[row % n], and x2[row] = x1[row] + flag_col (flag_col [64] = the last column of fc1.weight); both go
 * through the head of mapdn_critic_head_forward with the same parameters.  Arguments as there (rows a multiple of n, n <= 256); a tile
 * of rows is formed once and the W2 operand loaded once for both heads.
 * _forward: v1, v2, vmin [rows] — each may be NULL, not all three; vmin[row] = min(v1[row], v2[row]) (matd3.py:141-142; NaN wins, as torch.min).
 * _mse: loss = scale[0] * sum_rows wrow[row / n] * 1/2 [(ret[row] - v1[row])^2 + (ret[row] - v2[row])^2] (matd3.py:143-150; wrow [rows / n]
 *   or NULL: 1) and every gradient of it, without a forward launch:
 *   dbase [rows / n][64] = dx of both heads summed over each group of n rows;
 *   grads [4480 + n * 64] = dW2 | dgamma | dbeta | db2 | dw3 | db3 | [4353] the loss | pad to 4416 written as zero — laid out as the grads of
 *           mapdn_critic_head_mse, every entry summed over both heads — | [4416 .. 4479] d flag_col = the second head's dx summed over all
 *           rows | [4480 ..] dper_n [n][64] (both heads);
 *   scratch mapdn_critic_twin_scratch_floats(rows, n) floats (per-workgroup partials, reduced in a fixed order: deterministic; pad rule as above).
 * _geometry: the launch _mse takes — k_twin_mse<threads> on `blocks` workgroups with `lds_bytes` of dynamic LDS (cus as in
 *   mapdn_critic_head_backward_geometry); MAPDN_E_INVALID where the per-wavefront [n][64] accumulators do not fit LDS (n > 88). */
int mapdn_critic_twin_forward(const float* base, const float* per_n, int32_t n, const float* flag_col, const float* gamma, const float* beta,
                              float eps, const float* w2, const float* b2, const float* w3, const float* b3, float* v1, float* v2,
                              float* vmin, int64_t rows, void* stream);
int64_t mapdn_critic_twin_scratch_floats(int64_t rows, int32_t n);
int mapdn_critic_twin_geometry(int64_t rows, int32_t n, int32_t cus, int32_t* threads, int32_t* blocks, int32_t* lds_bytes);
int mapdn_critic_twin_mse(const float* ret, const float* wrow, const float* scale, const float* base, const float* per_n, int32_t n,
                          const float* flag_col, const float* gamma, const float* beta, float eps, const float* w2, const float* b2,
                          const float* w3, const float* b3, float* dbase, float* grads, float* scratch, int64_t rows, void* stream);

/* COMA's counterfactual baseline (models/coma.py:139-151: the critic valued sample_size more times per transition and agent, with that
 * agent's action replaced by a draw from its policy, and the values averaged) as ONE forward launch (csrc/critic_cf.hip).  The first
 * layer is linear in the actions, so with one action per agent a sampled row is the taken row plus a rank-1 term:
 *   baseline[row] = 1/S sum_s head(x[row] + delta[s][row] * act_col[row % n]),  head = that of mapdn_critic_head_forward;
 * x [rows][64] the first layer at the TAKEN actions, act_col [n][64] = fc1's action columns (row i: the column of agent i's action),
 * delta [S][rows] = sampled - taken action of the row's own agent.  The sampled row is formed by one fused multiply-add per element;
 * the sum runs in the order s = 0 .. S - 1 and is divided by S.  v0 [rows] or NULL: head(x[row]), the value at the taken actions
 * (coma.py:152) from the same read of x.  The tile of x, its act_col rows and the W2 operand are loaded once for all S samples.
 * No gradient exists: the advantage is detached (coma.py:182).  Device pointers, contiguous; rows < 2^31 (need not be a multiple of n),
 * 1 <= S <= 64, n >= 1; anything else is MAPDN_E_INVALID and nothing is launched. */
int mapdn_critic_head_counterfactual(const float* x, int32_t n, const float* act_col, const float* delta, int32_t S, const float* gamma,
                                     const float* beta, float eps, const float* w2, const float* b2, const float* w3, const float* b3,
                                     float* baseline, float* v0, int64_t rows, void* stream);

/* The core of MAAC's attention critic (critics/maac_critic.py:116-136, 156-157) as one forward and one backward launch
 * (csrc/critic_attn.hip).  sel, key, val [B][n][64] f32; head h owns columns h d .. (h + 1) d, d = 64 / H.  For sample b, agent i, head h:
 *   logit_ij = sel_i . key_j over j != i,  p_ij = softmax_j(logit_ij / sqrt(d)) (row maximum subtracted),  out_i = sum_j p_ij val_j,
 *   logit_sq[i][h] = sum_b sum_{j != i} logit_ij^2   ([n][H]; the regulariser is 1e-3 sum_h logit_sq[i][h] / (B (n - 1))).
 * _forward: out [B][n][64], logit_sq [n][H]; scratch: mapdn_attention_scratch_floats(B, n, H) floats (one partial of logit_sq per
 *   workgroup, summed in a fixed order: deterministic, no atomics).  Nothing but the operands is saved for the backward.
 * _backward: recomputes the probabilities; dout [B][n][64], dlogit_sq [n][H] (enters as 2 logit_ij dlogit_sq[i][h]) -> dsel, dkey, dval
 *   [B][n][64].
 * Device pointers, contiguous, the [B][n][64] ones 16-byte aligned.  B >= 1, 2 <= n <= mapdn_attention_max_agents() (48), H in {1, 2, 4},
 * B n 64 < 2^31; a null or misaligned pointer or any other shape is MAPDN_E_INVALID and nothing is launched. */
int mapdn_attention_forward(const float* sel, const float* key, const float* val, int64_t B, int32_t n, int32_t H, float* out,
                            float* logit_sq, float* scratch, void* stream);
int mapdn_attention_backward(const float* dout, const float* dlogit_sq, const float* sel, const float* key, const float* val, int64_t B,
                             int32_t n, int32_t H, float* dsel, float* dkey, float* dval, void* stream);
int64_t mapdn_attention_scratch_floats(int64_t B, int32_t n, int32_t H);
int32_t mapdn_attention_max_agents(void);

/* SQDDPG's Shapley coalition critic (models/sqddpg.py:37-106) behind its first layer, rows formed in the kernel (csrc/critic_shap.hip).
 * For sample b, coalition draw s and agent i, with pos[b][s][i] the position of agent i in the draw's order and gc = argsort(pos):
 *   x[b][s][i] = base[b] + id_cols[i] + P[b][s][pos_i],   P[b][s][p] = sum_{q <= p} act[b][gc[q]] act_cols[q],
 *   v[b][s][i] = head(x[b][s][i])  (LayerNorm -> ReLU -> fc2 -> ReLU -> fc3, as mapdn_critic_head_forward),  phi[b][i] = mean_s v[b][s][i].
 * base [b][64] (the observation columns of fc1 applied to all observations, plus its bias), id_cols / act_cols [n][64] (the agent-id and
 * action columns of fc1, transposed), act [b][n] f32, pos [b][S][n] INT32 (a draw of torch.multinomial, narrowed by the caller).
 * _forward: v [b][S][n] indexed by agent; phi [b][n] or NULL.
 * _backward (recomputes the forward): dv [b][S][n] (a caller that holds dphi passes dphi / S expanded over s).
 *   param_grads = 1: dbase [b][64]; grads [4416 + 2 n 64] = the trunk's gradients in the layout of mapdn_critic_head_backward, then
 *     d id_cols [n][64], then d act_cols [n][64]; scratch: mapdn_critic_shapley_scratch_floats(b, S, n) floats (one partial per
 *     workgroup, summed in a fixed order: deterministic, no atomics); dact [b][n] or NULL.
 *   param_grads = 0: dact [b][n] only (dact[b][i] = sum_s dx[b][s][i] . act_cols[pos_i]: only the own slot carries a gradient);
 *     dbase, grads, scratch may be NULL.
 * _geometry: mode 0 forward, 1 backward with param_grads, 2 backward without; cus = 0: the current device's CU count.  Reports the launch
 *   (threads, workgroups, LDS bytes) and, whatever the shape, the LDS budget per CU (163840) and the largest n that fits it.
 * Refused with MAPDN_E_INVALID before any launch: a null pointer (other than the optional ones) or one that is not aligned (16 bytes for
 * base, id_cols, act_cols, dbase and the trunk's vectors, 4 bytes otherwise); b < 1, S < 1, n < 1; n above the reported maximum;
 * b S n >= 2^31; a pos in HOST memory with a row that is not a permutation of 0 .. n - 1 (pinned memory is checked and then read by the
 * kernel; pageable host memory is refused).  For pos in device memory a permutation per row is a precondition: the kernels clamp its
 * values into [0, n), so a broken one gives wrong numbers but no access outside the buffers. */
int mapdn_critic_shapley_forward(const float* base, const float* id_cols, const float* act_cols, const float* act, const int32_t* pos,
                                 int64_t b, int32_t S, int32_t n, const float* gamma, const float* beta, float eps, const float* w2,
                                 const float* b2, const float* w3, const float* b3, float* v, float* phi, void* stream);
int mapdn_critic_shapley_backward(const float* dv, const float* base, const float* id_cols, const float* act_cols, const float* act,
                                  const int32_t* pos, int64_t b, int32_t S, int32_t n, const float* gamma, const float* beta, float eps,
                                  const float* w2, const float* b2, const float* w3, const float* b3, float* dbase, float* grads,
                                  float* scratch, float* dact, int32_t param_grads, void* stream);
int64_t mapdn_critic_shapley_scratch_floats(int64_t b, int32_t S, int32_t n);
int mapdn_critic_shapley_geometry(int64_t b, int32_t S, int32_t n, int32_t mode, int32_t cus, int32_t* threads, int32_t* blocks,
                                  int32_t* lds_bytes, int32_t* lds_budget, int32_t* max_n);

/* The glue of one batched rollout step (models/model.py:197-262) as three launches instead of ~45 one-line PyTorch kernels
 * (csrc/rollout.hip).  Device pointers, contiguous.
 * mapdn_explore_actions: action = tanh(mean + std * eps) (utilities/util.py:57-66; no tanh when tanh_bound == 0), action_pol =
 *   (avail != 0) * action (maddpg.py:92-93; avail / action_pol may be NULL), actual = translate_action(action) = 0.5 (clamp(action, -1,
 *   1) + 1) (high - low) + low with low / high = bias -/+ scale (utilities/util.py:123-132); f32, the PyTorch chain's operations in
 *   its order, bit-identical — NaN included: the clamp hands a NaN on as torch.clamp does, so a NaN mean gives a NaN action, a NaN
 *   action_pol (also where avail == 0: 0 * NaN) and a NaN actual: the env is handed the NaN, as the reference's is.
 * mapdn_rollout_stats: sums[0..10] += sum over live envs of info[e][k], sums[11] += of reward[e], sums[12] += live envs; then
 *   alive_out[e] = alive[e] & !done[e] (models/model.py:243-248, 225; alive_out may be alive); info [n_envs][11], reward [n_envs] f64; alive / done one byte per env.
 * mapdn_copy_segments: dst[i][0 .. nbytes[i]) = src[i][...] for up to 48 segments in one launch (the fields of a transition into
 *   their replay-ring positions, utilities/replay_buffer.py:25-29); HOST arrays of device pointers; 16-byte aligned, nbytes % 16 == 0. */
int mapdn_explore_actions(const float* mean, const float* eps, const float* avail, float stdv, int32_t tanh_bound, double action_scale,
                          double action_bias, float* action, float* action_pol, float* actual, int64_t n, void* stream);
int mapdn_rollout_stats(const double* info, const double* reward, const uint8_t* alive, const uint8_t* done, uint8_t* alive_out, double* sums,
                        int32_t n_envs, void* stream);
int mapdn_copy_segments(const void* const* src, void* const* dst, const int64_t* nbytes, int32_t n_segments, void* stream);

/* The PPO half of MAPPO / IPPO's update (learning_algorithms/ppo.py:39-70; csrc/ppo.hip).  Device pointers, contiguous f32: per-agent
 * tensors [rows][n], done / last_step / valid [rows]; rows >= 1, n >= 1, rows * n <= 2^40, no NULL pointer unless said so; anything
 * else is MAPDN_E_INVALID and nothing is launched.
 * mapdn_ppo_gae: adv[i] = delta[i] + gamma lambda mask[i] adv[i + stride] (0 beyond the last row), delta[i] = reward[i] + gamma
 *   next_value[i] mask[i] - value[i], mask[i] = 1 - done[i] where last_step[i] != 0 and 1 elsewhere (ppo.py:46-54, which is stride 1;
 *   a timeout row — last_step without done — does not cut the chain, nor does a done without last_step).  stride >= 1: row i's
 *   successor is row i + stride, so rows in (step, env) order with stride = the env count are one chain per env; chains may differ
 *   in length by one (rows % stride != 0); stride > rows gives chains of one row.  gamma and gamma * lambda are rounded to f32 as
 *   PyTorch rounds a Python scalar that meets an f32 tensor; the f32 operations are the reference's, in its order, uncontracted.
 * mapdn_ppo_loss_blocks: the number of floats `partial` must hold for a loss over rows * n = elems elements on the current device
 *   (one per workgroup of the launch); 0 for elems < 1.
 * mapdn_ppo_policy_loss: loss[0] = -scale[0] sum_e w[e] min(rho A, clamp(rho, 1 - eps_clip, 1 + eps_clip) A), w[e] = valid[row(e)]
 *   (valid NULL: 1), rho = exp(m lp - m old_log_prob), lp = the log-density of action under N(mean, exp(log_std)), m = (avail != 0)
 *   (avail NULL: 1), A = adv (ppo.py:30-33, 39, 62-64); dmean[e] = d loss[0] / d mean[e] as autograd gives it: torch.min halves the
 *   gradient where its operands are equal, clamp passes it on its bounds.  scale [1]: 1 / (max(sum valid, 1) n), the mean's divisor.
 * mapdn_ppo_value_loss: loss[0] = coef scale[0] sum_e w[e] max((v - R)^2, (v_old + clamp(v - v_old, -eps_clip, eps_clip) - R)^2),
 *   R = reward + gamma (1 - done) v_next (ppo.py:56, 67-70); dv[e] = d loss[0] / d v[e], ties as above.
 * Either loss: one streaming launch that writes the gradient and one partial sum per workgroup (wave-64 shuffles, then LDS), and a
 * one-workgroup pass that adds the partials in a fixed order — no floating-point atomics, the same input gives the same bits. */
int mapdn_ppo_gae(const float* reward, const float* value, const float* next_value, const float* done, const float* last_step, float* adv,
                  int64_t rows, int32_t n, int64_t stride, double gamma, double lambda, void* stream);
int mapdn_ppo_loss_blocks(int64_t elems);
int mapdn_ppo_policy_loss(const float* action, const float* mean, const float* log_std, const float* avail, const float* old_log_prob,
                          const float* adv, const float* valid, const float* scale, double eps_clip, float* loss, float* dmean,
                          float* partial, int64_t rows, int32_t n, void* stream);
int mapdn_ppo_value_loss(const float* v, const float* v_old, const float* reward, const float* v_next, const float* done,
                         const float* valid, const float* scale, double gamma, double eps_clip, double coef, float* loss, float* dv,
                         float* partial, int64_t rows, int32_t n, void* stream);

/* Calibration aid for the HBM counters (tools/calibrate_traffic.py): copies rows x Bp x 16 bytes from src to dst (device pointers) with
 * the solver's own global access pattern — raw-buffer 16-byte loads / stores of env-minor pair rows, 256 contiguous bytes per
 * 16-lane worker (pattern 0) — or with whole waves on one row (pattern 1), so that rocprofv3's FETCH_SIZE / WRITE_SIZE can be read
 * against a known byte count.  Bp a multiple of 256, rows x Bp x 16 < 4 GiB. */
int mapdn_debug_stream(const double* src, double* dst, int32_t rows, int32_t Bp, int32_t pattern, void* stream);

/* "MAPDN_SRC_HASH=<hex>": sha256 of the sources + flags the library was built from (mapdn_amd/build.py::source_hash).  The Python
 * loader refuses (or rebuilds) a library whose hash differs from the sources beside it.  No reference counterpart: build hygiene. */
const char* mapdn_build_info(void);

/* counters (host, synchronises the given stream): number of envs whose last reset exhausted
 * max_tries; mean / max NR iterations of the last solve */
int mapdn_stats(mapdn_handle* h, int64_t* reset_failures, double* mean_iters, int32_t* max_iters,
                void* stream);

/* seconds-resolution device timing of the dominant kernel for bench.py: enables hipEvent pairs
 * around every NR-solve launch on its stream; mapdn_nr_time_ms returns the accumulated time and
 * launch count since the last call and resets them (synchronises). */
int mapdn_nr_timing(mapdn_handle* h, int32_t enable);
int mapdn_nr_time_ms(mapdn_handle* h, double* total_ms, int64_t* launches);

/* Host-side export of the power-flow kernel instantiation this handle launches (coverage tests; also for device == -1 handles):
 * out[8] = solver, then by solver
 *   0 k_nr_tree<W, L, HL, GL, RES, DC, ZIP, GEN>: W, L, HL, GL, RES, DC, ZIP | GEN << 1 (RES 0: the generic residency body; csrc/nr_inst_list.hpp)
 *   1 k_nr_sparse<L, DC>:                    L, DC, ZIP | GEN << 1 (both decided at run time), 0, 0, 0, 0
 *   2 k_nr_dense<W, GA>:                     W, GA (the Jacobian in global memory), 0, 0, 0, 0, 0 */
int mapdn_get_nr_kernel(const mapdn_handle* h, int32_t* out8);

/* ---- Volt/VAR droop control: the reference's traditional baseline (traditional_control/pf_droop_matpower_all.m:84-162, law :196-231).
 * A field left 0 takes the script's value (so an all-zero struct, or NULL, is the script's configuration). */
typedef struct mapdn_droop_config {
  double va, vb, vc, vd;            /* breakpoints (p.u.) of the law: 0.95, 1.0, 1.0, 1.05; need va < vb <= vc < vd           */
  double damping;                   /* a <- (1 - damping) a + damping f(v): 0.1; 0 < damping <= 1                             */
  int32_t max_iter;                 /* power flows per env at most: 100; 1 ... 10000                                          */
  double v_tol;                     /* stop when ||v - v_last||_2 < v_tol over the sgen buses: 1e-4; > 0                      */
  double reactive_ratio;            /* q_max = min(sqrt(s_max^2 - p^2), reactive_ratio s_max): 1; > 0                         */
} mapdn_droop_config;

/* The droop controller's actions for the env's current state (the loads and PV the next mapdn_step solves with, noise applied):
 * per env a = 0, v_last = 100, then for i = 1 ... max_iter: power flow with q_j = sqrt(s_max_j^2 - p_j^2) a_j; v_j = |V| at sgen j's
 * bus; stop when ||v - v_last||_2 < v_tol, else v_last = v, a = (1 - damping) a + damping f(v) min(1, ratio s_max / lim).
 *   actions    f64 [B, ns]: a of the last solved power flow (step() takes it unclipped)
 *   vm_pu      f64 [B, nb] or NULL: |V| of that power flow (NaN for status 2 and 3)
 *   iterations i32 [B]: power flows solved;  status u8 [B]: 0 converged, 1 max_iter reached, 2 a power flow failed (actions = the
 *              last a whose power flow converged, 0 if the first failed), 3 not solved (terminated / frozen / waiting for its
 *              auto-reset restart; a = 0)
 * Device pointers on `stream`.  Not a step-path call: it polls the count of envs still iterating every 4 power flows (a stream
 * synchronisation) and allocates its workspace on the first call.  The obs, state, results, returns, counters and the next
 * mapdn_step are what they would have been without the call.  MAPDN_E_INVALID for a config outside the ranges above (checked on host-only handles too). */
int mapdn_droop_actions(mapdn_handle* h, const mapdn_droop_config* cfg, double* actions, double* vm_pu, int32_t* iterations,
                        uint8_t* status, void* stream);

/* ---- Optimal power flow: the reference's second traditional baseline (the traditional_control scripts: runopf on the loss objective with
 * the PV inverters' reactive power as the controls), as a reduced-space SQP on the handle's own power flow.
 * Per env, on the env's current state (the loads and PV the next mapdn_step solves with, noise applied):
 *     minimise   sum_k Re(V_k conj((Ybus V)_k))            (the total active loss)
 *     over       a in [-1, 1]^ns,  q_j = sqrt(s_max_j^2 - p_j^2) a_j
 *     subject to v_lower <= |V_k(a)| <= v_upper at every non-slack bus.
 * A field left 0 takes its default (so an all-zero struct, or NULL, is the default configuration). */
typedef struct mapdn_opf_config {
  double v_lower, v_upper;          /* voltage bounds (p.u.): the env's (mapdn_env_config); need 0 < v_lower < v_upper              */
  double v_tol;                     /* a point is feasible when its violation is <= v_tol: 5e-6 (MATPOWER's opf.violation); > 0     */
  double step_tol;                  /* stop when |d|inf < step_tol (and feasible): 1e-6; > 0                                        */
  int32_t max_iter;                 /* power flows per env at most: 50; 1 ... 1000                                                  */
  int32_t max_backtrack;            /* halvings of the step in a row when the trial point's power flow fails: 8; 1 ... 60          */
  int32_t meshed;                   /* 0: handles of the tree solver only.  1: handles of the sparse solver (k_nr_sparse: a meshed
                                       net, or a radial one with nr_solver = sparse) answer too: the sensitivities by the handle's
                                       elimination program, two columns a run; on a tree-solver handle 1
                                       changes nothing.  Other values: MAPDN_E_INVALID                                            */
} mapdn_opf_config;

/* a = 0, then for i = 1 ... max_iter: power flow at a; S = d|V|/da, g = dloss/da and the Gauss-Newton Hessian H from the converged V
 * (exact sensitivities: the Jacobian's block LU on the tree; with meshed = 1 on a sparse-solver handle, the handle's elimination
 * program); d = argmin g'd + d'Hd/2 s.t. -1 - a <= d <= 1 - a, v_lower <= |V| + S d
 * <= v_upper; stop when |d|inf < step_tol and the violation is <= v_tol, else a <- clip(a + d).  A trial point whose power flow fails
 * is retried at a + d/2, a + d/4, ...
 *   actions    f64 [B, ns]: a of the last solved power flow (step() takes it unclipped)
 *   vm_pu      f64 [B, nb] or NULL: |V| of that power flow (NaN when none solved)
 *   loss_mw    f64 [B]: the objective there, MW;  violation f64 [B]: max(|V| - v_upper, v_lower - |V|, 0) over the non-slack buses, p.u.
 *              (both NaN when none solved)
 *   iterations i32 [B]: power flows solved
 *   status     u8 [B]: 0 converged and feasible, 1 max_iter reached (or the last QP hit its iteration cap): the last solved point with
 *              its violation, 2 a power flow failed even after backtracking (actions = the last a that solved, 0 if the first failed),
 *              3 not solved (terminated / frozen / waiting for its auto-reset restart; a = 0)
 * Device pointers on `stream`.  Not a step-path call (it polls the count of envs still iterating; the workspace is allocated on the
 * first call).  The obs, state, results, returns, counters and the next mapdn_step are what they would have been without the call.
 * MAPDN_E_INVALID, on host-only handles too, for a config outside the ranges above and for what the linearisation does not cover:
 * meshed nets and handles on another solver than the tree solver (with meshed = 1: handles of the dense solver only),
 * voltage-dependent (ZIP) loads, generators, a start other than ext_grid_vm_pu, fused buses, more than 64 sgens. */
int mapdn_opf_actions(mapdn_handle* h, const mapdn_opf_config* cfg, double* actions, double* vm_pu, double* loss_mw, double* violation,
                      int32_t* iterations, uint8_t* status, void* stream);

/* Diagnostic entry for the kernel tests of the OPF baseline (tests/test_opf_kernels_gpu.py): ONE linearisation and ONE QP at the caller's
 * set-points, by the launches of mapdn_opf_actions' first iteration and nothing else — the start launch, which here begins from `a`
 * (clipped to [-1, 1]) instead of 0 and writes the Sbus of that a; one power flow in MODE_SOLVE with the OPF's own active set;
 * k_opf_linearise (a sparse-solver handle with meshed = 1: k_opf_sens_sparse and k_opf_reduce_sparse); k_opf_qp from zero multipliers —
 * and then the workspace as those launches left it.  Device pointers on `stream`:
 *   a          f64 [B, ns] in: the set-points;  ns: the row length of a, must be the handle's number of sgens
 * and, each may be NULL, env-major, by NODE k = 0 .. n - 1 (the elimination position; bus_of_pos of mapdn_get_flat_factors maps it to its
 * bus on a radial plan, a meshed plan takes the non-slack buses in ascending order; n = n_bus - 1, the slack is no node):
 *   v_re, v_im, vm f64 [B, n]: the converged V and the |V| the kernels read;   S f64 [B, n, ns] = d|V_k| / da_j;   g f64 [B, ns] = dloss / da (p.u.);   H f64 [B, ns, ns]
 *   loss_mw    f64 [B] (MW) and violation f64 [B] (p.u., against the config's bounds) at that V
 *   d          f64 [B, ns] the QP's step;   y f64 [B, ns + n] its multipliers: the box rows, then one row per node (> 0: upper bound)
 *   linearised u8 [B]: 1 when the env was solved (not terminated / frozen / waiting for its restart), its power flow converged and it was
 *              linearised; 0 otherwise: then d and y are 0, and V, S, g, H, loss_mw and violation are unspecified (workspace of an
 *              earlier call)
 *   qp_capped  u8 [B]: 1 when the QP hit its iteration cap (d is then its least-violation compromise)
 * Like mapdn_opf_actions: the obs, state, results, returns, counters and the next mapdn_step are what they would have been without the
 * call, also after mapdn_solve_only; the refusals of mapdn_opf_actions' config and nets (checked on host-only handles too), and
 * MAPDN_E_INVALID for a == NULL or an ns that is not the handle's; nothing is launched on a refusal. */
int mapdn_opf_probe(mapdn_handle* h, const mapdn_opf_config* cfg, const double* a, int32_t ns, double* v_re, double* v_im, double* vm, double* S,
                    double* g, double* H, double* loss_mw, double* violation, double* d, double* y, uint8_t* linearised,
                    uint8_t* qp_capped, void* stream);

/* ---- What-if: the reward and info of candidate actions without a step.
 * For every env e and candidate k: exactly what mapdn_step with actions[e][k] would report as reward and info from the env's current
 * state (voltage_control_env.py:178-196, 548-623) — the loads and PV of the current profile row, q_j = sqrt(s_max_j^2 - p_j^2) a_j by
 * the step path's own function, the handle's own power flow (tree, sparse or dense; DC start, ZIP loads and fused buses included), then
 * _calc_reward or the unsolvable branch of step() — and nothing of that state is committed or advanced.  Env-major buffers:
 *   actions    [B, K, ns] of actions_dtype (MAPDN_F32 / MAPDN_F64, widened as mapdn_step widens them); K = n_candidates,
 *              1 ... MAPDN_WHATIF_MAX_CANDIDATES
 *   reward     f64 [B, K];   info f64 [B, K, MAPDN_N_INFO] (column order as above)
 *   status     u8 [B, K], the values of the droop / OPF codes that apply:
 *              0 solved: the 11 infos of a converged step; iterations = the Newton count of the candidate's solve; vm_pu = the solved |V|
 *              2 the power flow did not converge: as step() reports it — the statistics of the committed state, reward - 200,
 *                destroy = 1, totally_controllable_ratio = 0, q_loss = mean |q| of the candidate's raw q; iterations as above; vm_pu NaN
 *              3 not evaluated: step() would not solve this env (terminated and frozen, or waiting for its auto-reset restart):
 *                reward, info and vm_pu NaN, iterations 0
 *   iterations i32 [B, K] or NULL;   vm_pu f64 [B, K, nb] or NULL
 * Device pointers on `stream`.  Only enqueues (three launches per candidate: the candidate's Sbus rows, the solve, the scoring); no
 * host synchronisation; the workspace, which does not grow with K, is allocated on the first call.  An env's row has the same bits
 * whatever B, K, the env's place in the batch and the other candidates are.  The obs, state, results, returns, counters, flags, RNG
 * draws and the next mapdn_step are what they would have been without the call, also after mapdn_solve_only.
 * Refused, by name in mapdn_last_error and with nothing launched: MAPDN_E_INVALID for a NULL actions / reward / info / status, a bad
 * dtype, n_candidates < 1 or > MAPDN_WHATIF_MAX_CANDIDATES (checked on host-only handles too); MAPDN_E_STATE before mapdn_reset and on
 * a host-only handle. */
#define MAPDN_WHATIF_MAX_CANDIDATES 1024
int mapdn_evaluate_actions(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t n_candidates,
                           double* reward, double* info, uint8_t* status, int32_t* iterations, double* vm_pu, void* stream);

/* ---- Action gradients: d reward / d action of candidate actions by an adjoint tree solve.
 * mapdn_evaluate_actions, and beside every row (e, k) of it
 *   grad       f64 [B, K, ns]: grad[e][k][j] = d reward[e][k] / d actions[e][k][j], every other entry of the candidate and the env's state
 *              held fixed.  reward = -(voltage_weight mean_b barrier(|V_b|) + q_weight mean_j |q_j scaling_j|), or with line_weight set
 *              -(voltage_weight mean_b barrier(|V_b|) + line_weight mean_l pl_mw_l) over net.line; q_j = sqrt(s_max_j^2 - p_j^2) a_j.
 *              The power-flow part is exact at the converged V: J' lambda = (d reward / d(theta, |V|))' with the polar Jacobian's
 *              block LU on the elimination tree, then one read per sgen.  At a kink the derivative is that of the branch the forward
 *              evaluation takes (bowl: |v - 1| > 0.05; courant_beltrami: max(0, .); bump: its three ranges); sign(0) = 0 for l1 at
 *              v == 1 and for |q_j| at q_j == 0.  An sgen on the ext_grid bus gets the direct q term alone.
 *              Rows of status 2 (the power flow did not converge) and 3 (not evaluated) are NaN.  So is a row of status 0 in which some
 *              q_j is not finite — a NaN or infinite action on an sgen of the ext_grid bus, whose injection no power flow reads, or a
 *              limit that is NaN because p_j exceeds s_max_j: the reward of such a row is not finite, and sign(NaN) = 0 would report a
 *              stationary point.  Its reward, info, status, iterations and vm_pu are what mapdn_evaluate_actions writes.
 * reward, info, status, iterations and vm_pu are bit for bit what mapdn_evaluate_actions writes for the same candidates and state, and
 * the call leaves the env's state and its next mapdn_step alone in the same way.  Only enqueues (four launches per candidate); the
 * workspace (18 doubles per node and env, allocated on the first call) does not grow with K; a row has the same bits whatever B, K,
 * the env's place in the batch and the other candidates are.
 * With mapdn_env_config.grad_meshed = 1 a handle of the general sparse solver (a meshed net) answers too: k_action_grad_sparse solves
 * the same adjoint system with the handle's elimination program on transposed blocks, in LDS, without a workspace.
 * Refused, by name in mapdn_last_error and with nothing launched, on host-only handles too: MAPDN_E_INVALID for meshed nets and
 * handles on another solver than the tree solver (grad_meshed = 1: for handles on the dense solver, and on the sparse solver for a
 * start other than ext_grid_vm_pu), voltage-dependent (ZIP) loads, generators, fused buses, a NULL actions / grad /
 * reward / info / status, a bad dtype, n_candidates < 1 or > MAPDN_WHATIF_MAX_CANDIDATES; MAPDN_E_STATE before mapdn_reset and on a
 * host-only handle.  nr_init = 2 (DC start) is accepted: the gradient depends on the converged V alone. */
int mapdn_action_gradients(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t n_candidates, double* grad,
                           double* reward, double* info, uint8_t* status, int32_t* iterations, double* vm_pu, void* stream);

/* ---- Voltage VJP: the bus voltages of candidate actions differentiated by the actions, for any cotangent.
 * For every env e and candidate k, with vm_pu[e][k][b] and va_degree[e][k][b] the bus voltages that mapdn_step with actions[e][k]
 * (unclipped, as mapdn_evaluate_actions takes them) would commit, and for every cotangent m = 0 ... M - 1 (M = n_cotangents):
 *   grad[e][k][m][j] = sum_b cot_vm[e][k][m][b] d vm_pu_b / d a_j + cot_va[e][k][m][b] d va_degree_b / d a_j,
 * every other entry of the candidate and the env's state held fixed (the limits sqrt(s_max_j^2 - p_j^2) are those of the state at the
 * call).  Exact at the converged power flow: the polar Jacobian is factorised once per (e, k) on the elimination tree, and every
 * cotangent costs one adjoint solve on those factors.  There is no direct term.  Env-major buffers:
 *   actions    [B, K, ns] of actions_dtype; K = n_candidates, 1 ... MAPDN_WHATIF_MAX_CANDIDATES
 *   cot_vm, cot_va   f64 [B, K, M, nb], each may be NULL (zeros); M = 0 ... MAPDN_VJP_MAX_COTANGENTS.  The entries of the ext_grid bus
 *              are never read (its voltage does not move): a NaN there does not reach the result
 *   grad       f64 [B, K, M, ns]; NULL if and only if M == 0.  An sgen on the ext_grid bus gets exactly 0.0
 *   vm_pu, va_degree   f64 [B, K, nb], each may be NULL; vm_pu is bit for bit what mapdn_evaluate_actions writes
 *   status     u8 [B, K] and iterations i32 [B, K] or NULL: bit for bit what mapdn_evaluate_actions writes
 * Rows of status 2 (the power flow did not converge) and 3 (not evaluated) are NaN in grad, vm_pu and va_degree; so is a row of
 * status 0 in which some q_j = sqrt(s_max_j^2 - p_j^2) a_j is not finite (mapdn_action_gradients' rule).
 * Device pointers on `stream`.  Only enqueues (four launches per candidate, three with M = 0 and va_degree NULL, one more after the last
 * candidate when vm_pu is given); the workspace is that of mapdn_action_gradients and does not grow with K or M; a row has the same bits
 * whatever B, K, M, the env's place in the batch, the other candidates and the other cotangents are.  The env's state and its next
 * mapdn_step are left alone as by mapdn_evaluate_actions.
 * Refused, by name in mapdn_last_error and with nothing launched, on host-only handles too — first the arguments: MAPDN_E_INVALID for a
 * NULL actions / status, a bad dtype, n_candidates < 1 or > MAPDN_WHATIF_MAX_CANDIDATES, n_cotangents < 0 or >
 * MAPDN_VJP_MAX_COTANGENTS, M >= 1 with both cotangents NULL, M == 0 with a grad buffer or M >= 1 without one; then the handle
 * ("voltage_vjp: ... not supported"): handles of the sparse and of the dense solver (whatever grad_meshed says), meshed nets,
 * voltage-dependent (ZIP) loads, generators, fused buses.  MAPDN_E_STATE before mapdn_reset and on a host-only handle. */
#define MAPDN_VJP_MAX_COTANGENTS 1024
int mapdn_voltage_vjp(mapdn_handle* h, const void* actions, int32_t actions_dtype, int32_t n_candidates, int32_t n_cotangents,
                      const double* cot_vm, const double* cot_va, double* grad, double* vm_pu, double* va_degree, uint8_t* status,
                      int32_t* iterations, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAPDN_H */
