/*
 * dragg_mi355x.h -- C ABI of the batched MI355X (gfx950) home-MPC solver.
 *
 * Drop-in replacement for the per-home HEMS solve of corymosiman12/dragg:
 *
 *   reference                                   this ABI
 *   -----------------------------------------   ------------------------------------------
 *   MPCCalc.run_home()        mpc_calc.py:649   dragg_mpc_step()      (device-resident state)
 *     get_initial_conditions  mpc_calc.py:264     (initial state read from the hash arrays)
 *     water_draws             mpc_calc.py:193     (computed on device from draw_hourly)
 *     set_environmental_vars  mpc_calc.py:206     (slices of oat/ghi/tou + reward price)
 *     add_*_constraints       mpc_calc.py:291-432 (built on device, never materialised)
 *     solve_mpc (GLPK_MI)     mpc_calc.py:434     (int_mode round, default: the MILP solved
 *                                                  exactly -- thermal chains by an exact
 *                                                  Pareto-front DP, battery by an exact
 *                                                  piecewise-linear DP; relax / round_lp:
 *                                                  banded-KKT ADMM + exact vertex polish)
 *     cleanup_and_finish      mpc_calc.py:476     (success extraction / fallback thermostat)
 *     redis_write_optimal_vals mpc_calc.py:100    (hash arrays updated in place)
 *   manage_home + ProcessPool aggregator.py:723   one launch over all homes of a timestep
 *   collect_data sums         aggregator.py:751   dragg_mpc_aggregate() / dragg_mpc_aggregate_rows()
 *   run_baseline's loop       aggregator.py:757   dragg_mpc_step_main() + dragg_mpc_step_side()
 *                                                  (lag mode: a home still in its step-function DP
 *                                                  does not hold up the other homes' next steps)
 *   MPCCalc per-solve (explicit inputs)         dragg_mpc_solve_explicit()
 *
 * Conventions
 *  - Every pointer in the structs below is a DEVICE pointer (hipMalloc / torch
 *    CUDA tensors), fp64 unless stated; arrays are struct-of-arrays with the home
 *    index innermost: element (f, h) of a [F][N] array lives at f*N + h.
 *  - All entry points return 0 on success or a negative dragg_mpc_error code;
 *    nothing throws across the ABI.  Launches are asynchronous on `stream`
 *    (a hipStream_t, NULL = default stream); no host synchronisation inside.
 *  - The per-home redis hash (`redis_client.py`, all values str) is replaced by
 *    two fp64 arrays: `vals` [DRAGG_NVAL][N] (the scalar fields a step writes)
 *    and `fc` [N][DRAGG_NFC][H] (the `<key>_<j>` forecast fields, rewritten only
 *    by a successful solve).  NaN means "field absent from the hash".
 */
#ifndef DRAGG_MI355X_H
#define DRAGG_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRAGG_MPC_ABI_VERSION 10

/* home types (aggregator.py:425, 468, 520, 555); bit 0 = pv, bit 1 = battery */
enum dragg_home_type {
    DRAGG_BASE = 0, DRAGG_PV_ONLY = 1, DRAGG_BATTERY_ONLY = 2, DRAGG_PV_BATTERY = 3
};

/* per-home parameters, rows of params[DRAGG_NPARAM][N] (mpc_calc.py:157-189, 239-258) */
enum dragg_param {
    DRAGG_P_R = 0,        /* hvac.r                               */
    DRAGG_P_C,            /* hvac.c * 1000                        */
    DRAGG_P_PC,           /* hvac.p_c / S                         */
    DRAGG_P_PH,           /* hvac.p_h / S                         */
    DRAGG_P_RW,           /* wh.r * 1000                          */
    DRAGG_P_PW,           /* wh.p / S                             */
    DRAGG_P_CW,           /* wh.tank_size * 4.2                   */
    DRAGG_P_V,            /* wh.tank_size                         */
    DRAGG_P_TMIN, DRAGG_P_TMAX, DRAGG_P_TWMIN, DRAGG_P_TWMAX,
    DRAGG_P_TINIT,        /* hvac.temp_in_init                    */
    DRAGG_P_TWINIT,       /* wh.temp_wh_init                      */
    DRAGG_P_BRATE,        /* battery.max_rate                     */
    DRAGG_P_EMIN,         /* battery.capacity_lower * capacity    */
    DRAGG_P_EMAX,         /* battery.capacity_upper * capacity    */
    DRAGG_P_ETAC, DRAGG_P_ETAD,
    DRAGG_P_EINIT,        /* battery.e_batt_init * capacity       */
    DRAGG_P_PVAREA, DRAGG_P_PVEFF,
    DRAGG_NPARAM
};

/* forecast keys: rows of fc[N][DRAGG_NFC][H] (`<key>_<j>` hash fields, mpc_calc.py:514-520) */
enum dragg_fc_key {
    DRAGG_K_P_GRID = 0, DRAGG_K_FORECAST_P_GRID, DRAGG_K_P_LOAD, DRAGG_K_TEMP_IN_EV,
    DRAGG_K_TEMP_WH_EV, DRAGG_K_HVAC_COOL, DRAGG_K_HVAC_HEAT, DRAGG_K_WH_HEAT, DRAGG_K_COST,
    DRAGG_K_WATERDRAWS, DRAGG_K_P_PV, DRAGG_K_U_PV_CURT, DRAGG_K_P_BATT_CH,
    DRAGG_K_P_BATT_DISCH, DRAGG_K_E_BATT,
    DRAGG_NFC
};

/* scalar hash fields: rows of vals[DRAGG_NVAL][N]; rows 0..14 are the keys above, i.e. the
   un-suffixed `<key>` field (mpc_calc.py:516, 584-594) */
enum dragg_val {
    DRAGG_V_TEMP_IN_OPT = DRAGG_NFC, DRAGG_V_TEMP_WH_OPT, DRAGG_V_CORRECT_SOLVE,
    DRAGG_V_SOLVE_COUNTER,
    DRAGG_NVAL
};

/* per-home status written by a step (status[N]) */
enum dragg_status {
    DRAGG_ST_OPTIMAL = 0,          /* solved: the MILP optimum (round) / LP vertex (relax)      */
    DRAGG_ST_INFEASIBLE = 1,       /* proven infeasible by interval presolve                   */
    DRAGG_ST_INFEASIBLE_CERT = 2,  /* ADMM primal-infeasibility certificate                     */
    DRAGG_ST_MAX_ITER = 3,         /* no verified vertex within max_iter                         */
    DRAGG_ST_ROUND_FAIL = 4,       /* boxes pass presolve, but no integer duty schedule exists  */
    DRAGG_ST_ERR_PARSE = 5,        /* fallback's float(str[0]) would raise (mpc_calc.py:537)     */
    DRAGG_ST_ERR_MISSING = 6,      /* hash field missing at t>0 (KeyError, mpc_calc.py:280-289)  */
    DRAGG_ST_SOLVER_ERROR = 7      /* the named solver raised: prob.solve's exception is          */
                                   /* swallowed and the fallback runs (mpc_calc.py:450-454)       */
};

enum dragg_mpc_error {
    DRAGG_OK = 0, DRAGG_E_ARG = -1, DRAGG_E_HIP = -2, DRAGG_E_LDS = -3, DRAGG_E_HORIZON = -4
};

/* integer handling of the duty-cycle variables (mpc_calc.py:171-173) */
enum dragg_int_mode {
    DRAGG_INT_ROUND = 0,    /* MILP, exact: thermal front DP + battery LP DP (default) */
    DRAGG_INT_RELAX = 1,    /* LP relaxation (ADMM + exact vertex polish)             */
    DRAGG_INT_ROUND_LP = 2, /* LP relaxation for status/battery, then the integer DP  */
    DRAGG_INT_FAIL = 3      /* a solver that cannot take the MILP (hems.solver "ECOS": cvxpy's
                               ECOS is not MIP-capable, so prob.solve raises inside the try of
                               mpc_calc.py:450-454): every solve takes the fallback,
                               status DRAGG_ST_SOLVER_ERROR                           */
};

typedef struct dragg_mpc_dims {
    int32_t n_homes;       /* N (0 = an empty shard: every entry point is a no-op,
                              per-home pointers may be NULL; aggregate writes zeros)    */
    int32_t horizon;       /* H = prediction_horizon * dt            (mpc_calc.py:150) */
    int32_t sub_steps;     /* S = sub_subhourly_steps                (mpc_calc.py:148) */
    int32_t dt;            /* hourly_agg_steps                       (mpc_calc.py:149) */
    int32_t n_draw_hours;  /* columns of draw_hourly                                   */
    int32_t n_env;         /* length of oat/ghi/tou                                    */
    int32_t n_rp;          /* length of reward_price (1 or >= H, mpc_calc.py:353)      */
    int32_t int_mode;      /* dragg_int_mode                                           */
    int32_t max_iter;      /* ADMM iteration cap (<=0: default 4000)                   */
    int32_t check_every;   /* polish / residual check interval (<=0: default 10)       */
    double discount;       /* discount_factor                        (mpc_calc.py:152) */
    int32_t flags;         /* dragg_flag bits (0 = default)                             */
    int32_t n_groups;      /* G (since v10; 0 or 1 = one community, as before).  G > 1: a
                              grouped batch -- the n_homes homes are G consecutive replicas
                              of Nb = n_homes / G base homes (n_homes % G == 0): home r is
                              replica (group) r / Nb of base home r % Nb.  Group g is solved
                              under row g of problem.reward_price ([G][n_rp]) and draws the
                              keyed season noise of its BASE home (global home home_offset +
                              base * home_stride), so G candidate prices are solved against
                              one community in one dragg_mpc_step.  Every per-home array
                              (params, home_type, draw_hourly, vals, fc, the outputs, an
                              explicit noise array) is n_homes wide as always: the caller
                              tiles the base community's G times (state: dragg_mpc_replicate).
                              Such a step is dragg_mpc_step_episodes' (below) with every group
                              on the shared seed, start index and clock: one mechanism, one
                              set of kernels.  dragg_mpc_solve_explicit and the lag-mode
                              entry points return DRAGG_E_ARG for G > 1                    */
} dragg_mpc_dims;

/* dims.flags */
enum dragg_flag {
    /* int_mode round is exact on every TOU chain by default: a chain the Pareto-front DPs cannot
       take (a feasible set narrower than one duty step, mixed-sign prices without a usable bound, a
       front past 2,048 labels, S != 6) is solved by the exact step-function DP (out.int_path bit
       15).  The one exception: a chain under RL prices (a price change at more than H/4 stages)
       whose front passes 2,048 labels keeps its bucketed schedule (int_path reason 3) unless this
       flag is set -- there the step-function DP costs ~25x the whole RL action. */
    DRAGG_FLAG_EXACT = 1
};

typedef struct dragg_mpc_problem {
    const double* params;       /* [DRAGG_NPARAM][N]                                    */
    const int32_t* home_type;   /* [N] dragg_home_type                                  */
    const double* draw_hourly;  /* [n_draw_hours][N] wh.draw_sizes (aggregator.py:377)  */
    const double* oat;          /* [n_env] redis 'OAT' list                             */
    const double* ghi;          /* [n_env] redis 'GHI' list                             */
    const double* tou;          /* [n_env] redis 'tou' list                             */
    const double* reward_price; /* [n_rp]  redis 'reward_price' list; a grouped batch    */
                                /* (dims.n_groups = G > 1): [G][n_rp], row g = group g's */
    int32_t start_index;        /* start_hour_index (aggregator.py:630-638)             */
    int32_t home_offset;        /* global index of home 0 of this shard (noise key; a    */
                                /* grouped batch: of base home 0)                        */
    uint64_t seed;              /* keyed season-noise stream when noise == NULL         */
    void* workspace;            /* device scratch, dragg_mpc_workspace_bytes(dims) bytes */
                                /* (int_mode round: DP back-pointers); may be NULL when  */
                                /* that size is 0                                        */
    int32_t home_stride;        /* global index of home i = home_offset + i*home_stride */
                                /* (strided shards; 0 or 1 = a contiguous shard)         */
    int32_t reserved;
} dragg_mpc_problem;

typedef struct dragg_mpc_hash {
    double* vals;               /* [DRAGG_NVAL][N]  in/out, NaN = absent               */
    double* fc;                 /* [N][DRAGG_NFC][H] in/out (home-contiguous since v7) */
} dragg_mpc_hash;

typedef struct dragg_mpc_out {
    int32_t* status;            /* [N] dragg_status                                     */
    int32_t* iters;             /* [N] ADMM iterations used (0 if presolve decided)    */
    double* obj;                /* [N] objective sum_k gamma^k price_k p_grid_k         */
    double* relax_obj;          /* [N] LP-relaxation objective (NaN if infeasible)     */
    double* hist;               /* optional [DRAGG_NVAL][N] copy of vals after the step */
    int64_t* cycles;            /* optional [DRAGG_NPHASE][N] shader cycles per phase   */
    int32_t* int_path;          /* optional [N] integer-DP path (int_mode round): 0 = the
                                   exact front DP solved both thermal chains; bit 0 / bit 1
                                   = the indoor-air / tank chain kept an approximate (feasible)
                                   schedule; bits 4-7 / 8-11 its reason: 3 = an RL-priced chain
                                   (a price change at more than H/4 stages) whose front passed
                                   the big launch's 2,048 labels keeps its bucketed schedule
                                   (default build; DRAGG_FLAG_EXACT sends it to the step-function
                                   DP), 6 = the exact step-function DP past its capacity (its pool
                                   of 2^20 breakpoints per chain, or its work bound of 2 M merge
                                   points per pass): the bucketed schedule it was handed stands in
                                   (else the feasibility pass's); bit 12 = solved by a later launch (its front
                                   outgrew the hot launch's capacity; still exact when
                                   bits 0-11 are 0); bits 13 / 14 = status ROUND_FAIL
                                   decided by the indoor-air / tank chain (no integer duty
                                   schedule for it); bit 15 = solved by the exact
                                   step-function DP (a feasible set narrower than one duty
                                   step, mixed-sign prices, S != 6, a front past 2,048)  */
} dragg_mpc_out;

/* solver phases timed into dragg_mpc_out.cycles (diagnostic; NULL = not stamped) */
enum dragg_phase {
    DRAGG_PH_SETUP = 0,   /* inputs, problem build, presolve              */
    DRAGG_PH_ITER,        /* ADMM iterations (rhs, KKT solve, updates);   */
                          /* int_mode round: the bucketed DP              */
    DRAGG_PH_FACTOR,      /* block-LDL' factorisations                    */
    DRAGG_PH_POLISH,      /* exact basis polish; int_mode round: the mid  */
                          /* / big launch's exact front pass              */
    DRAGG_PH_CHECK,       /* residuals, certificate, rho adaptation       */
    DRAGG_PH_INTEGER,     /* integer duty-cycle DP                        */
    DRAGG_PH_WRITE,       /* objective, cleanup_and_finish, hash writes   */
    DRAGG_PH_BATTERY,     /* exact battery LP (int_mode round)            */
    DRAGG_NPHASE
};

/* explicit per-solve inputs (parity tests and the per-home MPCCalc facade) */
typedef struct dragg_mpc_explicit {
    const int32_t* t;           /* [N] timestep (fallback rule needs t > 0)             */
    const double* T0;           /* [N] temp_in_init value                               */
    const double* Tw0;          /* [N] temp_wh_init value (after draw mixing)           */
    const double* E0;           /* [N] e_batt_init value (ignored for non-battery)      */
    const int32_t* counter;     /* [N] solve_counter read from the hash                 */
    const int32_t* winter;      /* [N] 1 = max(oat_ev) <= 30 (mpc_calc.py:303)          */
    const double* draw;         /* [H+1][N] draw_size                                   */
    const double* oat;          /* [H+1][N] oat_current                                 */
    const double* ghi;          /* [H+1][N] ghi_current                                 */
    const double* price;        /* [H][N]   total_price                                 */
} dragg_mpc_explicit;

/* Resources of the solver's launches as the code object and the runtime report them
   (hipFuncGetAttributes, hipOccupancyMaxActiveBlocksPerMultiprocessor on the current device):
   index 0 = the hot launch (int_mode round: DM_FRONT; relax / round_lp: the LP kernel),
   index 1 = the big launch (DM_BUCKET), index 2 = the mid launch (DM_MID), index 3 = the
   step-function launch (DM_NARROW); indices 1-3 are zeros outside int_mode round. */
#define DRAGG_NLAUNCH 4
typedef struct dragg_mpc_kernel_info {
    int32_t vgprs[DRAGG_NLAUNCH];          /* registers per lane (hipFuncAttributes.numRegs)   */
    int32_t scratch_bytes[DRAGG_NLAUNCH];  /* private memory per lane (spills; localSizeBytes) */
    int32_t lds_bytes[DRAGG_NLAUNCH];      /* dynamic LDS per workgroup at these dims          */
    int32_t threads[DRAGG_NLAUNCH];        /* threads per workgroup (one home per workgroup)   */
    int32_t blocks_per_cu[DRAGG_NLAUNCH];  /* resident workgroups per CU at that LDS           */
} dragg_mpc_kernel_info;

int dragg_mpc_abi_version(void);
const char* dragg_mpc_strerror(int code);

/* Dynamic LDS bytes one home (workgroup) needs for this horizon; < 0 if H unsupported. */
int dragg_mpc_lds_bytes(const dragg_mpc_dims* dims);

/* Device workspace bytes a launch with these dims needs (problem.workspace); < 0 on error. */
int64_t dragg_mpc_workspace_bytes(const dragg_mpc_dims* dims);

/* Device bytes of the lag mode's side workspace (dragg_mpc_lag.side_workspace; since v9): the side
   pass keeps only its device lists and per-block scratch there (the per-home regions are read from
   problem.workspace), ~0.5 GB at 10k homes, H = 48, against the workspace's 1.34 GB. */
int64_t dragg_mpc_side_workspace_bytes(const dragg_mpc_dims* dims);

/* Byte offset of every region of problem.workspace, in order, and its size (`total` =
   dragg_mpc_workspace_bytes; the side workspace is the span [deferred, w_rows)); for diagnostics that
   read the workspace.  A list is [N] i32 entries (home in bits 0-27), then its length and a take
   counter.  int_mode round / fail: the layout (cell_rows hold rows only when dims.n_rp > 1);
   round_lp: the back-pointers alone, every other field equals `total`; relax: all zero. */
typedef struct dragg_mpc_workspace_regions {
    int64_t back_pointers, solutions, deferred, big_rows, steps_list, steps_pools, mid_list, mid_rows, w_rows,
            cell_rows, total;
} dragg_mpc_workspace_regions;
/* Host-only query; returns dragg_mpc_workspace_bytes' error codes. */
int dragg_mpc_workspace_regions_get(const dragg_mpc_dims* dims, dragg_mpc_workspace_regions* regions);

/* The sha-256 of the sources this library was built from (the kernel file and this header; since
   v9): the host refuses a library whose stamp is not its sources' (a stale build). */
const char* dragg_mpc_source_hash(void);

/* One closed-loop timestep for all N homes: reads the hash arrays (t > 0) or the
   parameters (t == 0), solves, and writes the hash arrays back in place.
   noise: [H][N] standard normals for the season draw (mpc_calc.py:222) or NULL for the
   keyed on-device stream philox(seed, home, t). */
int dragg_mpc_step(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob,
                   dragg_mpc_hash* hash, dragg_mpc_out* out, int32_t timestep,
                   const double* noise, void* stream);

/* Independent solves with explicit inputs; hash supplies the fallback's forecast fields
   and receives the written fields exactly as in dragg_mpc_step. prob->oat/ghi/tou/
   reward_price/draw_hourly are ignored. */
int dragg_mpc_solve_explicit(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob,
                             const dragg_mpc_explicit* in, dragg_mpc_hash* hash,
                             dragg_mpc_out* out, void* stream);

/* Diagnostic knobs, read from the environment when the library loads and again only here (never
   per step): DRAGG_WAVES_PER_HOME=1|2|4 (the hot launch's waves per home; results bit-identical) and
   DRAGG_FORCE_STEP_DP=1 (every chain through the step-function DP; tests), DRAGG_STEP_POOL_CAP=n and
   DRAGG_STEP_WORK_CAP=n (a smaller pool / work bound of that DP; tests of its capacity path),
   DRAGG_HOT_ILP=1|2 (64-child chunks per front-DP pass of the one-wave hot launch; default: 2 at <= 8 homes
   per CU, else 1; results bit-identical), DRAGG_SIDE_GRID=hot,mid,big,narrow (the lag mode's side-pass
   grids, each clamped to 1 .. its launch's per-block scratch slots: dragg_mpc_side_grid reports the
   grids in effect), DRAGG_NARROW_LDS_KB=n (the step-function launch's LDS per block; default all of a
   CU's: a smaller block can share a CU with hot-launch blocks; results bit-identical).  Unset: the defaults.  Lag mode (dragg_mpc_step_main / _side) honours every knob
   but DRAGG_WAVES_PER_HOME: both its passes run the one-wave hot kernel. */
void dragg_mpc_reload_knobs(void);

/* The lag mode's side-pass grids for these dims under the current knobs: grid4 = blocks of its hot,
   mid (and cell), big and step-function launches (zeros for an empty shard).  Host-only query. */
int dragg_mpc_side_grid(const dragg_mpc_dims* dims, int32_t* grid4);

/* Fill `info` for these dims (needs a GPU: queries the current device). */
int dragg_mpc_kernel_info_get(const dragg_mpc_dims* dims, dragg_mpc_kernel_info* info);

/* collect_data sums (aggregator.py:751-753): out3 = {sum p_grid_opt, sum
   forecast_p_grid_opt, sum cost_opt} over the shard's homes; an absent field (NaN: a home
   the reference would have crashed on, KeyError at aggregator.py:750-752) makes its sum NaN. */
int dragg_mpc_aggregate(const dragg_mpc_dims* dims, const dragg_mpc_hash* hash, double* out3,
                        void* stream);

/* Fan a base batch's state out to a grouped batch (since v10): `dims` describes the grouped batch
   (n_homes = G * Nb, n_groups = G; G <= 1: a plain copy), src_hash holds the base batch's vals
   [DRAGG_NVAL][Nb] and fc [Nb][DRAGG_NFC][H], dst_hash the grouped batch's vals [DRAGG_NVAL][G * Nb] and
   fc [G * Nb][DRAGG_NFC][H].  Every replica receives its base home's fields bit for bit (NaN payloads
   included: NaN = field absent).  One kernel: each source element is read once and stored G times.
   src_hash is only read.  DRAGG_E_ARG also for a vals or fc pointer, on either side, that is not a multiple
   of 8 (before the grouped segment mover such a pointer was undefined behaviour); nothing is written then. */
int dragg_mpc_replicate(const dragg_mpc_dims* dims, const dragg_mpc_hash* src_hash,
                        dragg_mpc_hash* dst_hash, void* stream);

/* The way back: adopt one of C copies as the destination batch's state (since v10, additive).  `dst_dims`
   describes the destination: Nd = n_homes homes in E = max(n_groups, 1) groups of Nb = Nd / E homes.  The
   source holds `copies` = C copies of it, copy-major -- copy c in columns [c * Nd, (c + 1) * Nd), the layout
   dragg_mpc_replicate writes with G = C -- so its vals are [DRAGG_NVAL][C * Nd], its fc [C * Nd][DRAGG_NFC][H]
   and its per-home outputs C * Nd wide.  `choice` is a device int32 [E]: group e of the destination
   receives, from copy choice[e], the columns of its Nb homes -- every row of vals, each home's fc block, and
   every member of dragg_mpc_out that is non-NULL in BOTH src_out and dst_out (status, iters, obj, relax_obj,
   int_path, hist; cycles is ignored; either struct may be NULL: the hash arrays alone).  A choice outside
   [0, C) leaves every column of group e untouched -- no byte of it is written: idle or parked episodes and
   "no valid candidate" pass through.  Bit for bit (NaN payloads included: NaN = field absent); src_* is
   only read.  One kernel; a block works on one group, so the choice is read once per block.  n_homes == 0:
   a no-op.  DRAGG_E_ARG: copies < 1, n_homes % E != 0, E > 65535, a NULL choice or NULL hash pointers, or an
   array pointer that is not a multiple of its element size (8 for the double arrays, 4 for status, iters and
   int_path; before the grouped segment mover such a pointer was undefined behaviour); nothing is written then. */
int dragg_mpc_adopt(const dragg_mpc_dims* dst_dims, int32_t copies, const int32_t* choice,
                    const dragg_mpc_hash* src_hash, const dragg_mpc_out* src_out,
                    dragg_mpc_hash* dst_hash, dragg_mpc_out* dst_out, void* stream);

/* The choice for dragg_mpc_adopt, made on the device (since v10, additive): for each group e of `dst_dims`
   the copy c that minimises |sums[c * E + e][0] - target[e]| (sums: dragg_mpc_aggregate_groups' rows of the
   C * E-group source, [C * E][3]; target [E]); ties go to the smaller |prices[c * E + e][0]| (prices
   [C * E][n_rp], the source's reward-price rows), then to the smaller c.  The doubles are compared as they
   are, no tolerance.  A copy whose load is NaN is never chosen; choice[e] = -1 if none is valid. */
int dragg_mpc_select_groups(const dragg_mpc_dims* dst_dims, int32_t copies, const double* sums,
                            const double* target, const double* prices, int32_t n_rp, int32_t* choice,
                            void* stream);

/* collect_data's sums of every group of a grouped batch (since v10): out[G][3], row g exactly as
   dragg_mpc_aggregate on a batch holding group g's Nb homes (the same lanes and reduction order:
   bit-identical); a NaN makes only its own group's sum NaN.  G <= 1: one row, dragg_mpc_aggregate's.
   n_homes == 0: zeros. */
int dragg_mpc_aggregate_groups(const dragg_mpc_dims* dims, const dragg_mpc_hash* hash, double* out,
                               void* stream);

/* Vectorised episodes: the grouped batch of dims.n_groups (G >= 1 here) with up to three values of each
   group's own, so that every group is a full episode of the base community: its own season-noise seed, its
   own start index into the environment lists and its own clock.  This is the one grouped step:
   dragg_mpc_step with G > 1 runs it with all three shared.  Home r is in group g = r / Nb and has base
   home b = r % Nb; its step is exactly
   dragg_mpc_step of base home b with seed ep.seed[g] (global home home_offset + b * home_stride),
   start_index ep.start_index[g], timestep ep.timestep[g] and reward-price row g -- nothing else changes, so
   group g equals, bit for bit, a plain batch of the Nb base homes run with those values.  The clock is per
   group: one group may be at t = 0 and take its initial conditions from params while another reads its
   hash arrays.  A NULL member means the shared value (problem.seed, problem.start_index, the `timestep`
   argument) for every group; with all three NULL the step is dragg_mpc_step's.  An explicit `noise` array
   ([H][N]) is used as given.
   Idle groups: a group whose timestep is negative takes no part in the step -- its blocks return before any
   write, so none of its columns changes in vals, fc, status, iters, obj, relax_obj, int_path or out.hist, and
   none of its homes enters a later launch.  A group whose window [start_index + timestep, ... + horizon] does
   not lie inside the environment lists (start_index < 0 or start_index + timestep + horizon >= n_env) is
   idle too: the values live on the device, where only the kernel can check them.
   The state persists in the hash arrays from step to step like any batch's; the caller advances the clocks.
   Per-group sums: dragg_mpc_aggregate_groups; state fan-out: dragg_mpc_replicate.  Returns DRAGG_E_ARG for
   ep == NULL or n_homes % G != 0.  dragg_mpc_solve_explicit and lag mode stay refused for G > 1. */
typedef struct dragg_mpc_episodes {      /* all device pointers, [G], G = max(dims.n_groups, 1) */
    const uint64_t* seed;         /* group g's season-noise seed     (NULL: problem.seed for all)        */
    const int32_t*  start_index;  /* group g's start_hour_index      (NULL: problem.start_index)         */
    const int32_t*  timestep;     /* group g's own timestep; < 0: the group is idle (NULL: `timestep`)   */
} dragg_mpc_episodes;
int dragg_mpc_step_episodes(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob,
                            const dragg_mpc_episodes* ep, dragg_mpc_hash* hash, dragg_mpc_out* out,
                            int32_t timestep, const double* noise, void* stream);

/* The keyed season-noise stream of a batch of episodes (dragg_mpc_season_noise's draw, the same kernel, with
   the groups' own seeds and clocks): writes [H][N] normals, home r drawing the stream of
   (ep.seed[g], global home home_offset + (r % Nb) * home_stride, ep.timestep[g]) -- ep.timestep NULL: the
   `timestep` argument; ep.seed must be given (there is no shared seed here); ep.start_index is not read.  The
   columns of an idle group (timestep < 0) are left as they are. */
int dragg_mpc_season_noise_episodes(const dragg_mpc_dims* dims, const dragg_mpc_episodes* ep,
                                    int32_t home_offset, int32_t home_stride, int32_t timestep,
                                    double* noise_out, void* stream);

/* A device-resident vector environment around dragg_mpc_step_episodes (since v10, additive): what an RL
   driver keeps per episode -- its clock, the rows of its history, collect_data's sums and the aggregator's
   setpoint rule (gen_setpoint, aggregator.py:677-696) -- filed and updated by one kernel after a step, and
   started over by one kernel, with no host round trip.  All pointers are device pointers; G =
   max(dims.n_groups, 1), Nb = n_homes / G, N = n_homes.  A history store may be NULL (it is then not kept).
     clock     [G]     steps each group has taken
     max_load, min_load [G], tracked [G][prev_timesteps] (oldest first): gen_setpoint's state
     obs       [5][G]  rows agg_load, forecast_load, agg_cost, agg_setpoint, timestep (exact in a double)
     status_hist, path_hist [T][N] int32; hist [T][DRAGG_NVAL][N]; agg_hist [T][G][3]   (T = num_timesteps) */
#define DRAGG_ENV_PREV_MAX 128
typedef struct dragg_mpc_env {
    int32_t num_timesteps;      /* T >= 1: rows of the history stores                                    */
    int32_t prev_timesteps;     /* P, 1 .. DRAGG_ENV_PREV_MAX: the tracked loads (agg.rl.prev_timesteps) */
    double max_poss_load;       /* a fresh episode tracks P loads of half of it                          */
    double start_load;          /* agg_load and forecast_load of a fresh episode (3 kW per home)         */
    const int32_t* ran;         /* [G] dragg_mpc_env_file: the timesteps the step just ran with          */
                                /* (dragg_mpc_episodes.timestep; < 0 or >= T: the group took no step)    */
    int32_t* clock;
    double* max_load;
    double* min_load;
    double* tracked;
    double* obs;
    const double* sums;         /* [G][3] dragg_mpc_env_file: dragg_mpc_aggregate_groups' rows           */
    int32_t* status_hist;
    int32_t* path_hist;
    double* hist;
    double* agg_hist;
} dragg_mpc_env;

/* After a step: for every group g with t = env.ran[g] in [0, T), file group g's Nb columns of out.status,
   out.int_path and out.hist (the step's [DRAGG_NVAL][N] row) into row t of status_hist, path_hist and hist,
   and sums[g] into agg_hist[t][g]; clock[g] = t + 1; then the environment state as the host keeps it:
   timestep = t + 1, (agg_load, forecast_load, agg_cost) = sums[g], and gen_setpoint's rule in its order --
   at timestep < 2 the tracked loads start over at max_poss_load / 2 and max_load / min_load at -inf / +inf,
   later the oldest tracked load makes room for agg_load; the setpoint is their average, summed in numpy's
   pairwise order (np.average of P <= 128 doubles) and divided by P; then agg_load replaces max_load if it is
   greater or timestep % 24 == 0, and min_load likewise -- bit for bit the host's doubles; then the five
   observations.  A group that took no step is not touched: no byte of its columns in any store, nor its
   clock, tracked loads, max_load, min_load or observations (its blocks return before any access).  One
   kernel; `ran` is only read and must not be `clock`.  A store and its source come together: out.status with
   status_hist, out.int_path with path_hist, out.hist with hist (out may be NULL when none is kept);
   agg_hist's source is sums.  n_homes == 0: a no-op.  DRAGG_E_ARG: a NULL env, ran, clock, sums, obs,
   max_load, min_load or tracked; P outside 1 .. DRAGG_ENV_PREV_MAX; T < 1; n_homes % G != 0; G > 65535; a
   store without its source or a source without its store; ran == clock. */
int dragg_mpc_env_file(const dragg_mpc_dims* dims, const dragg_mpc_env* env, const dragg_mpc_out* out,
                       void* stream);

/* Start the groups g with mask[g] != 0 (device bytes [G]) over: their columns of hash.vals and their homes'
   blocks of hash.fc NaN (0x7ff8000000000000: field absent, the state of a new batch), their columns of every
   row of the stores cleared (hist NaN; status_hist, path_hist and agg_hist 0), clock 0, and the environment
   state of a fresh episode: timestep 0, agg_load = forecast_load = start_load, agg_cost 0, the setpoint rule
   applied to fresh tracked loads.  Only the masked groups' columns are written: an unmasked group keeps
   every byte.  One kernel; env.ran and env.sums are not read.  DRAGG_E_ARG as above, or a NULL mask or hash. */
int dragg_mpc_env_reset(const dragg_mpc_dims* dims, const dragg_mpc_env* env, const uint8_t* mask,
                        dragg_mpc_hash* hash, void* stream);

/* The choice over K-step rollouts (since v10, additive): dragg_mpc_select_groups for candidates that were
   rolled K steps ahead -- after dragg_mpc_replicate, K times (dragg_mpc_step_episodes at the clocks ran + j,
   dragg_mpc_aggregate_groups into block j of `sums`).  E = max(dst_dims.n_groups, 1) episodes, `copies` = C
   candidates each, copy-major groups c * E + e; all pointers are device pointers.
   For episode e let t = ran[e], k = min(K, T - t) (0 if t < 0 or t >= T: the episode took no step) and, for
   candidate c, l_j = sums[j][c * E + e][0].
   Setpoints: s_0 = target[e]; s_j, j >= 1, is the setpoint gen_setpoint's rule returns at timestep t + j with load
   l_(j-1) on the state the call before left -- what dragg_mpc_env_file would file if the candidate were played j
   times, bit for bit: at timestep < 2 the tracked loads start over at fresh_load (so a rollout from t = 0 never
   tracks l_0), later the oldest makes room for the new load; the average is summed in numpy's pairwise order and
   divided by P.  max_load / min_load do not enter.  `tracked` is only read: the window after j steps is a
   function of it and l_0 .. l_(j-1).
   Score: (((0.0 + w_0 * |l_0 - s_0|) + w_1 * |l_1 - s_1|) + ...) over j < k, plain fp64 in ascending j, the
   product rounded before the sum.  Rows j >= k of `sums` are never read.  A candidate with a NaN l_j, j < k, is
   invalid: its score is NaN and it is never chosen.
   Choice: the valid c of least score; ties go to the smaller |prices[c * E + e][0]|, then to the smaller c (the
   candidates are compared in ascending c with dragg_mpc_select_groups' comparison; the doubles as they are, no
   tolerance).  None valid, or k = 0: choice[e] = -1 and every score of e NaN.  With K = 1 and weights {1.0} the
   choice is dragg_mpc_select_groups' for every input with ran[e] in [0, T).
   One kernel (a block per episode, a lane per candidate); vector stores, no atomics; sums, ran, tracked, target,
   weights and prices are only read.  n_homes == 0: every choice -1, every score NaN.  DRAGG_E_ARG: a NULL p or a
   NULL member other than score; steps < 1; prev_timesteps outside 1 .. DRAGG_ENV_PREV_MAX; num_timesteps < 1;
   n_rp < 1; copies < 1; n_homes % E != 0; nothing is written then. */
typedef struct dragg_mpc_paths {
    int32_t steps;            /* K >= 1 */
    int32_t num_timesteps;    /* T */
    int32_t prev_timesteps;   /* P, 1 .. DRAGG_ENV_PREV_MAX */
    double  fresh_load;       /* max_poss_load / 2 */
    const double*  sums;      /* [K][C*E][3], copy-major groups c*E+e: aggregate_groups' rows per rollout step */
    const int32_t* ran;       /* [E] the clock step 0 ran with; < 0 or >= T: the episode took no step */
    const double*  tracked;   /* [E][P] gen_setpoint's tracked loads now (oldest first); only read */
    const double*  target;    /* [E] the setpoint now (observation row agg_setpoint) */
    const double*  weights;   /* [K] */
    const double*  prices;    /* [C*E][n_rp] */
    int32_t n_rp;
    int32_t* choice;          /* [E] */
    double*  score;           /* optional [C*E] */
} dragg_mpc_paths;
int dragg_mpc_select_paths(const dragg_mpc_dims* dst_dims, int32_t copies, const dragg_mpc_paths* p,
                           void* stream);

/* Plan observations (since v10, additive): the community's planned curves per group, reduced from the hash
   arrays every successful solve leaves on the device.  A pure function of them: reads hash.vals and hash.fc
   only, writes plan.curve, plan.count and plan.stats only.  G = max(dims.n_groups, 1), Nb = n_homes / G;
   home i of group g is column n = g * Nb + i.
   The curve of forecast key k is time-aligned: with cnt = vals[DRAGG_V_SOLVE_COUNTER][n] and c = (int)cnt if
   0 <= cnt < H, else H (NaN -- a home that never solved -- and a counter at or past H), home n contributes
     entry 0       vals[k][n]: the collected value (collect_data's; after a success fc[n][k][0] bit for bit,
                   after a fallback the thermostat's),
     entry j >= 1  fc[n][k][c + j] if c + j < H, else nothing: a home in fallback contributes its stale plan at
                   the right wall-clock stage (the index write_fallback itself reads).
   A NaN value (a PV key of a home without PV, a field never written) is absent: it adds nothing and is not
   counted; count[g][.][j] is the number of homes behind curve[g][.][j].
   The summation order is part of the contract: partial p[w], w = 0 .. DRAGG_PLAN_WAYS - 1, starts at +0.0 and
   adds the present values of homes i = w, w + 16, w + 32, ... in ascending order with plain fp64 adds; the sum
   is the balanced tree over the 16 partials, p[2m] + p[2m + 1] level by level: ((p0 + p1) + (p2 + p3)) + ...
   The order depends on Nb alone, never on G or the launch: group g's rows equal those of a batch of its Nb
   homes, bit for bit.  stats sums the present values of a vals row in the same order; min and max run over
   them (the sign of a zero min or max is unspecified); none present: count 0, sum +0.0, min +inf, max -inf.
   n_homes == 0: every group gets that empty result (curve +0.0, count 0).  One kernel; vector stores, no
   atomics.  DRAGG_E_ARG: a NULL dims, hash or plan; a key bit at or past DRAGG_NFC or a row bit at or past
   DRAGG_NVAL; horizon < 1; n_homes % G != 0 or G > 65535 (a grid row per group); curve or count NULL with
   fc_keys != 0, stats NULL with val_rows != 0 (an output whose mask is zero may be NULL and is not written);
   with n_homes > 0 a NULL hash.vals, or a NULL hash.fc with fc_keys != 0. */
#define DRAGG_PLAN_WAYS 16
typedef struct dragg_mpc_plan {
    uint32_t fc_keys;   /* bit k < DRAGG_NFC: the horizon curve of forecast key k            */
    uint32_t val_rows;  /* bit r < DRAGG_NVAL: statistics of vals row r                      */
    double*  curve;     /* [G][nk][H] sums; nk = popcount(fc_keys), keys in ascending order  */
    int32_t* count;     /* [G][nk][H] homes that contributed to each sum                     */
    double*  stats;     /* [G][nr][4]: count, sum, min, max; nr = popcount(val_rows)         */
} dragg_mpc_plan;
int dragg_mpc_plan_groups(const dragg_mpc_dims* dims, const dragg_mpc_hash* hash, const dragg_mpc_plan* plan,
                          void* stream);

/* Price classes (since v10, additive): a reward price per class of homes in one community.  A class is an
   integer 0 .. P - 1 per BASE home; the map belongs to the community and is shared by every group (episode,
   sweep replica) of a grouped batch.  State has no class: dragg_mpc_replicate, dragg_mpc_adopt, the sums and the
   environment entries are unchanged. */
#define DRAGG_CLASS_MAX 64
typedef struct dragg_mpc_classes {
    int32_t n_classes;            /* P, 1 .. DRAGG_CLASS_MAX                                              */
    const int32_t* price_class;   /* device [Nb], by base home (Nb = n_homes / max(n_groups, 1)); may be  */
                                  /* NULL when P == 1                                                     */
} dragg_mpc_classes;

/* dragg_mpc_step_episodes with problem.reward_price read as [G][P][n_rp]: home r of group g = r / Nb reads row
   g * P + price_class[r % Nb]; everything else about the step is dragg_mpc_step_episodes'.  Homes do not
   interact within a step, so the columns of group g's class-c homes equal, bit for bit, those of the plain step
   of group g under row (g, c) alone.  classes == NULL or n_classes == 1: the call IS dragg_mpc_step_episodes
   (the same launches, the same bits; reward_price [G][n_rp]).  A class value outside 0 .. P - 1 is clamped into
   that range by the kernel (the lookup is a scalar load per block: a block is one home): device data cannot make
   it read past the price rows.  dragg_mpc_workspace_bytes is unchanged.  DRAGG_E_ARG: n_classes outside
   1 .. DRAGG_CLASS_MAX, a NULL price_class with n_classes > 1, and wherever dragg_mpc_step_episodes returns it. */
int dragg_mpc_step_classes(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob,
                           const dragg_mpc_episodes* ep, const dragg_mpc_classes* classes, dragg_mpc_hash* hash,
                           dragg_mpc_out* out, int32_t timestep, const double* noise, void* stream);

/* dragg_mpc_plan_groups per (group, class): plan.curve and plan.count are [G][P][nk][H], plan.stats is
   [G][P][nr][4].  Contract: class c's rows of group g equal dragg_mpc_plan_groups' rows of group g bit for bit
   when the homes of g that are not in class c are absent -- every vals row of theirs (the solve counter
   included) and every fc entry NaN.  The summation order is therefore dragg_mpc_plan_groups': the 16 ways run
   over the GROUP's home positions i = w, w + 16, ... (not over the class's members), then the balanced tree; a
   home of another class adds nothing and is not counted.  An empty class gets the empty result: sum +0.0, count
   0, min +inf, max -inf.  A class value outside 0 .. P - 1 counts as clamped into it, as in the step.
   classes == NULL or n_classes == 1: dragg_mpc_plan_groups' output ([G][...]).  One kernel, a grid plane per
   class; vector stores, no atomics, no block reads what another writes.  DRAGG_E_ARG: dragg_mpc_plan_groups'
   cases and the class ones of dragg_mpc_step_classes. */
int dragg_mpc_plan_classes(const dragg_mpc_dims* dims, const dragg_mpc_hash* hash,
                           const dragg_mpc_classes* classes, const dragg_mpc_plan* plan, void* stream);

/* Lag mode (since v8): run_rbo_mpc's timestep loop (aggregator.py:757-778) has no feedback between
   homes, so a home whose chain needs the slow exact step-function DP need not hold up the others.
   A step is split into two passes the caller puts on two streams:
     dragg_mpc_step_main(t)  on the main stream: every home whose clock is at t (its previous step
                             complete) is solved by the hot / mid / big launches; a home whose clock
                             is behind is listed in `skipped`; chains left for the step-function DP
                             are listed in `narrow` (not solved here);
     dragg_mpc_step_side(t)  on the side stream, AFTER main(t) (an event): the skipped homes' whole
                             step (their own lists and per-block scratch in side_workspace) and the
                             step-function DP of every chain in `narrow`.
   A home's clock becomes t + 1 when its step is complete (a side-pass completion is published to
   the concurrently running main pass with an agent-scope release).  Each step needs its own
   skipped / narrow lists until its side pass has run: with a ring of R list pairs the main pass of
   step t + R must wait for the side pass of step t.  Results are bit-identical to dragg_mpc_step's
   (every home's solve is the same code on the same inputs), but per-step outputs of lagging homes
   land later: the caller reads them (status -- out.status should then be a per-step row --, hist
   rows, vals/fc) only after the side stream has drained, and takes collect_data's sums from the
   history rows (dragg_mpc_aggregate_rows).  Keyed season noise only (the NULL-noise stream);
   int_mode round / fail only. */
typedef struct dragg_mpc_lag {
    int32_t* clock;             /* [N] timesteps completed per home (dragg_mpc_lag_reset) */
    int32_t* skipped;           /* [DRAGG_LAG_LIST_INTS(N)] the step's homes left to the side pass */
    int32_t* narrow;            /* [DRAGG_LAG_LIST_INTS(N)] the step's step-function DP chains   */
    void* side_workspace;       /* dragg_mpc_side_workspace_bytes(dims) bytes, the side pass's own */
} dragg_mpc_lag;
#define DRAGG_LAG_LIST_INTS(n) ((n) + 4)

/* clock[] = timestep for every home (before the first lag-mode step after any other kind of step) */
int dragg_mpc_lag_reset(const dragg_mpc_dims* dims, const dragg_mpc_lag* lag, int32_t timestep, void* stream);
int dragg_mpc_step_main(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob, dragg_mpc_hash* hash,
                        dragg_mpc_out* out, int32_t timestep, const dragg_mpc_lag* lag, void* stream);
int dragg_mpc_step_side(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob, dragg_mpc_hash* hash,
                        dragg_mpc_out* out, int32_t timestep, const dragg_mpc_lag* lag, void* stream);

/* collect_data's sums of n_rows steps from their history rows ([n_rows][DRAGG_NVAL][N], the
   dragg_mpc_out.hist copies): out[r][3] exactly as dragg_mpc_aggregate on row r (bit-identical). */
int dragg_mpc_aggregate_rows(const dragg_mpc_dims* dims, const double* rows, int32_t n_rows, double* out,
                             void* stream);

/* The keyed season-noise stream used when noise == NULL: writes [H][N] normals for
   timestep t (exposed so the host and tests can reproduce the draw); home i of the shard
   draws the stream of global home home_offset + i*home_stride (home_stride 0 = 1); in a grouped
   batch (dims.n_groups > 1) home i draws its base home's, i % Nb in place of i. */
int dragg_mpc_season_noise(const dragg_mpc_dims* dims, uint64_t seed, int32_t home_offset,
                           int32_t home_stride, int32_t timestep, double* noise_out, void* stream);

/* Electric vehicles (since v10, additive): an exact stage-varying storage LP per vehicle, solved beside the homes.
   The reference has no vehicle; the model is this project's.  A vehicle is one more
   separable block of a home: with a = ch_eff / dt, b = 1 / (disch_eff dt) and q_k = S gamma^k price_k (the
   expression of the home kernel's battery cost row),
       minimise sum_k q_k (ch_k + dis_k),   E_{k+1} = E_k + a ch_k + b dis_k - drain_k,
       0 <= ch_k <= rate_ch_k,   -rate_dis_k <= dis_k <= 0,   lo_k <= E_{k+1} <= hi_k        (k = 0 .. H - 1)
   with E_0 fixed.  The cost-to-go is convex piecewise linear; it is carried backward as a sorted segment list
   (the battery LP's recursion with per-stage rates, drift and box) and the optimum is recovered forward: exact,
   no iteration.  One wave per vehicle.  Nothing here reads or writes a home's arrays, and no home entry reads
   these.  M = n_vehicles vehicles; with dims.n_groups = G > 1 they are G consecutive replicas of M / G base
   vehicles (M % G == 0), vehicle r in group r / (M / G).  dims.n_homes is only checked (the usual dims check),
   never read: a fleet passes its own M there.  Episode clocks and price classes reach the vehicles through
   dragg_mpc_ev_step_episodes (below); the three entries before it know one clock and one price row per group. */
enum dragg_ev_param {           /* rows of dragg_mpc_ev.params [DRAGG_NEVP][M] */
    DRAGG_EVP_CAP = 0,          /* ev.capacity (kWh)                              */
    DRAGG_EVP_EMIN,             /* ev.capacity_lower * capacity                   */
    DRAGG_EVP_EMAX,             /* ev.capacity_upper * capacity                   */
    DRAGG_EVP_RATE,             /* ev.max_rate (kW)                               */
    DRAGG_EVP_ETAC, DRAGG_EVP_ETAD,
    DRAGG_EVP_EINIT,            /* ev.e_ev_init * capacity                        */
    DRAGG_EVP_V2G,              /* 1.0: may discharge to the home, 0.0: may not   */
    DRAGG_EVP_DEPART,           /* step of day the vehicle leaves                 */
    DRAGG_EVP_RETURN,           /* step of day it is back (depart < return)       */
    DRAGG_EVP_TRIP,             /* ev.trip_kwh, drained evenly over the away steps */
    DRAGG_EVP_EREQ,             /* ev.depart_soc * capacity                       */
    DRAGG_NEVP
};
/* the vehicle's horizon rows fc[M][DRAGG_NEVK][H] (vehicle-contiguous, like dragg_mpc_hash.fc); rows 0 .. 3 of
   vals[DRAGG_NEVV][M] are their entry 0 */
enum dragg_ev_key {
    DRAGG_EVK_P_CH = 0,         /* p_ev_ch    = ch_k                                        */
    DRAGG_EVK_P_DISCH,          /* p_ev_disch = dis_k (<= 0)                                */
    DRAGG_EVK_E,                /* e_ev_opt   = E_{k+1}: vals' row is the next step's E_0   */
    DRAGG_EVK_COST,             /* cost_ev    = price_k S (ch_k + dis_k), as cost_opt       */
    DRAGG_NEVK
};
enum dragg_ev_val {
    DRAGG_EVV_FORECAST_P = DRAGG_NEVK,   /* forecast_p_ev = ch_1 + dis_1 (0 at H == 1)      */
    DRAGG_NEVV
};
enum dragg_ev_status {
    DRAGG_EV_OPTIMAL = 0,       /* the LP's optimum                                          */
    DRAGG_EV_INFEASIBLE = 1     /* no trajectory: the uncontrolled rule's rows (below)       */
};

typedef struct dragg_mpc_ev {
    const double* params;       /* [DRAGG_NEVP][M]                                           */
    double* vals;               /* [DRAGG_NEVV][M] in/out (the step reads row DRAGG_EVK_E at t > 0) */
    double* fc;                 /* [M][DRAGG_NEVK][H] out                                    */
    int32_t* status;            /* [M] dragg_ev_status                                       */
    double* obj;                /* [M] sum_k q_k (ch_k + dis_k), summed in ascending k without contraction; */
                                /* NaN where infeasible                                      */
    int32_t day_offset;         /* step of day of timestep 0, 0 .. 24 dt - 1                 */
    int32_t n_vehicles;         /* M (0: every entry is a no-op, the sums are zero)          */
} dragg_mpc_ev;

/* explicit per-stage inputs: the general storage LP (parity tests).  Row k of lo / hi is the box of E_{k+1}. */
typedef struct dragg_mpc_ev_explicit {
    const double* price;        /* [H][M] price_k (q_k = S gamma^k price_k)                  */
    const double* rate_ch;      /* [H][M] >= 0                                               */
    const double* rate_dis;     /* [H][M] >= 0                                               */
    const double* drain;        /* [H][M]                                                    */
    const double* lo;           /* [H][M]                                                    */
    const double* hi;           /* [H][M]                                                    */
    const double* E0;           /* [M]                                                       */
} dragg_mpc_ev_explicit;

/* dynamic LDS of one EV workgroup (DRAGG_EV_WAVES vehicles), or DRAGG_E_HORIZON / DRAGG_E_ARG */
#define DRAGG_EV_WAVES 4
int dragg_mpc_ev_lds_bytes(const dragg_mpc_dims* dims);

/* Solve every vehicle's LP on the explicit inputs; reads params rows ETAC, ETAD (the dynamics) and EMAX, CAP (the
   uncontrolled rule) and writes vals, fc, status, obj.  An infeasible LP gets the uncontrolled rule, evaluated
   on one lane in ascending k without contraction:
       ch_k = min(rate_ch_k, max(0, (Emax - E) / a)),  dis_k = 0,  E <- min(max((E + a ch_k) - drain_k, 0), capacity).
   DRAGG_E_ARG for G > 1 (explicit inputs carry no price rows). */
int dragg_mpc_ev_solve_explicit(const dragg_mpc_dims* dims, const dragg_mpc_ev* ev,
                                const dragg_mpc_ev_explicit* in, void* stream);

/* One closed-loop step: the kernel builds the explicit inputs itself -- stage k lies at step of day
   s_k = (day_offset + t + k) mod 24 dt; away iff depart <= s_k < return; rate_ch_k = away ? 0 : max_rate,
   rate_dis_k = v2g ? rate_ch_k : 0, drain_k = away ? trip / (return - depart) : 0, the box of E_{k+1} is
   [s_{k+1} == depart ? max(Emin, Ereq) : Emin, Emax], price_k = reward_price[k] + tou[start_index + t + k] (the
   home prologue's expression; group g reads row g of problem.reward_price), E_0 = params EINIT at t == 0, else
   vals row DRAGG_EVK_E -- and runs dragg_mpc_ev_solve_explicit's code on them.  Reads problem.tou,
   reward_price and start_index only. */
int dragg_mpc_ev_step(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob, const dragg_mpc_ev* ev,
                      int32_t timestep, void* stream);

/* The vehicles' part of collect_data's sums per group: out[g] = [sum (ch_0 + dis_0), sum forecast_p_ev,
   sum cost_ev_0] over group g's M / G vehicles.  One 1024-thread block per group: thread i adds vehicles i,
   i + 1024, ... of the group in ascending order, the 64 lanes of a wave are added in the fixed order of the wave
   sum, the 16 wave partials pairwise as a balanced tree -- an order that depends on neither G nor the batch
   around the group, so a group's sums are those of a fleet of its vehicles alone, bit for bit.  No contraction,
   no atomics.  M == 0: zeros. */
int dragg_mpc_ev_aggregate(const dragg_mpc_dims* dims, const dragg_mpc_ev* ev, double* out, void* stream);

/* A step of a grouped fleet whose groups are episodes: dragg_mpc_ev_step's kernel behind
   another prologue.  G = max(dims.n_groups, 1), Mb = M / G; vehicle r is base vehicle v = r % Mb of group g = r / Mb.
     clock       t_g = ep.timestep ? ep.timestep[g] : timestep.  t_g < 0: the group is idle -- its waves leave
                 before any write, no byte of its columns of vals, fc, status or obj changes.
     start index s_g = ep.start_index ? ep.start_index[g] : problem.start_index.  A group whose window leaves the
                 environment lists (s_g < 0 or s_g + t_g + H >= n_env) is idle too: dragg_mpc_step_episodes' rule,
                 so an episode's homes and vehicles idle together.
     day clock   ev.day_offset stays the step of day of environment index problem.start_index: stage k of group g
                 lies at step of day (day_offset + (s_g - problem.start_index) + t_g + k) mod 24 dt, the
                 non-negative remainder.
     E_0         params EINIT where t_g == 0, else the vehicle's vals row DRAGG_EVK_E (per group).
     price row   classes NULL or n_classes == 1: row g of reward_price [G][n_rp].  P classes: reward_price is
                 [G][P][n_rp] and the vehicle reads row g P + clamp(price_class[v], 0, P - 1); price_class is [Mb]
                 by BASE VEHICLE (its owner home's class).
   ep.seed is not read: a vehicle draws no noise.  With every member of ep NULL and no classes the outputs are
   dragg_mpc_ev_step's, bit for bit.  DRAGG_E_ARG: ep NULL, M % G != 0, n_classes outside 1 .. DRAGG_CLASS_MAX, a
   NULL price_class with P > 1, and wherever dragg_mpc_ev_step returns it (its window check of the shared start
   index and timestep applies where the member array that replaces them is NULL).  M == 0: a no-op. */
int dragg_mpc_ev_step_episodes(const dragg_mpc_dims* dims, const dragg_mpc_problem* prob,
                               const dragg_mpc_episodes* ep, const dragg_mpc_classes* classes,
                               const dragg_mpc_ev* ev, int32_t timestep, void* stream);

/* out[g][j] = base[g][j] + s[g][j], s exactly dragg_mpc_ev_aggregate's row of group g (the same summation order)
   followed by one plain fp64 add, no contraction: homes-only sums plus the fleet's.  out may be base.  ev_out
   (nullable, [G][3]) receives s.  M == 0: out = base, ev_out zeros. */
int dragg_mpc_ev_aggregate_onto(const dragg_mpc_dims* dims, const dragg_mpc_ev* ev, const double* base, double* out,
                                double* ev_out, void* stream);

/* dragg_mpc_adopt for a fleet: the source fleet holds `copies` copies of the destination's E groups, copy-major;
   group e takes from group choice[e] * E + e its Mb columns of vals, its vehicles' fc blocks, status and obj, bit
   for bit.  A choice outside [0, copies) leaves every byte of group e untouched.  dst_dims: the destination
   fleet's (n_homes = its M).  DRAGG_E_ARG: a NULL or misaligned array. */
int dragg_mpc_ev_adopt(const dragg_mpc_dims* dst_dims, int32_t copies, const int32_t* choice,
                       const dragg_mpc_ev* src_ev, const dragg_mpc_ev* dst_ev, void* stream);

/* The masked groups (mask [G] bytes, nonzero: reset) start over: their columns of vals, their fc blocks and obj
   become NaN (0x7ff8000000000000), their status 0; every other group keeps every byte. */
int dragg_mpc_ev_reset(const dragg_mpc_dims* dims, const dragg_mpc_ev* ev, const uint8_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DRAGG_MI355X_H */
