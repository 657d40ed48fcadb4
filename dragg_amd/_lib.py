"""ctypes binding of the C ABI in include/dragg_mi355x.h (libdragg_mi355x.so).

The library is built in-tree (dragg_amd/libdragg_mi355x.so, see dragg_amd/build.py).
There is deliberately no CPU fallback: if the library or a GPU is missing, every
entry point raises.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# DRAGG_LIB: an alternative build of the same library (kernel experiments); default in-tree
LIB_PATH = os.environ.get("DRAGG_LIB") or os.path.join(HERE, "libdragg_mi355x.so")

ABI_VERSION = 10

# enums (mirror include/dragg_mi355x.h)
BASE, PV_ONLY, BATTERY_ONLY, PV_BATTERY = 0, 1, 2, 3
TYPE_CODE = {"base": BASE, "pv_only": PV_ONLY, "battery_only": BATTERY_ONLY, "pv_battery": PV_BATTERY}

PARAMS = ["R", "C", "PC", "PH", "RW", "PW", "CW", "V", "TMIN", "TMAX", "TWMIN", "TWMAX", "TINIT",
          "TWINIT", "BRATE", "EMIN", "EMAX", "ETAC", "ETAD", "EINIT", "PVAREA", "PVEFF"]
NPARAM = len(PARAMS)
P = {k: i for i, k in enumerate(PARAMS)}

FC_KEYS = ["p_grid_opt", "forecast_p_grid_opt", "p_load_opt", "temp_in_ev_opt", "temp_wh_ev_opt",
           "hvac_cool_on_opt", "hvac_heat_on_opt", "wh_heat_on_opt", "cost_opt", "waterdraws",
           "p_pv_opt", "u_pv_curt_opt", "p_batt_ch", "p_batt_disch", "e_batt_opt"]
NFC = len(FC_KEYS)
VAL_KEYS = FC_KEYS + ["temp_in_opt", "temp_wh_opt", "correct_solve", "solve_counter"]
NVAL = len(VAL_KEYS)
K = {k: i for i, k in enumerate(VAL_KEYS)}

(ST_OPTIMAL, ST_INFEASIBLE, ST_INFEASIBLE_CERT, ST_MAX_ITER, ST_ROUND_FAIL, ST_ERR_PARSE, ST_ERR_MISSING,
 ST_SOLVER_ERROR) = range(8)
# int_path bits (dragg_mi355x.h): 0-11 = a chain left the exact front DP (chain bits + reasons);
# PATH_SECOND = the home was solved by the second launch (exact unless bits 0-11 are set)
PATH_APPROX_MASK = 0xFFF
PATH_SECOND = 1 << 12
PATH_FAIL_T, PATH_FAIL_TW = 1 << 13, 1 << 14     # ROUND_FAIL decided by the indoor-air / tank chain
PATH_STEPS = 1 << 15           # solved by the exact step-function DP (DM_NARROW launch)
STATUS_NAMES = ["optimal", "infeasible", "infeasible_cert", "max_iter", "round_fail", "err_parse",
                "err_missing", "solver_error"]

INT_ROUND, INT_RELAX, INT_ROUND_LP, INT_FAIL = 0, 1, 2, 3
FLAG_EXACT = 1                 # dims.flags: the step-function DP for every chain the front DP cannot take
INT_MODES = {"round": INT_ROUND, "relax": INT_RELAX, "round_lp": INT_ROUND_LP, "fail": INT_FAIL}

PHASES = ["setup", "iter", "factor", "polish", "check", "integer", "write", "battery"]
NPHASE = len(PHASES)

c_dp = ctypes.c_void_p  # device pointers are passed as raw integers


class Dims(ctypes.Structure):
    _fields_ = [("n_homes", ctypes.c_int32), ("horizon", ctypes.c_int32), ("sub_steps", ctypes.c_int32),
                ("dt", ctypes.c_int32), ("n_draw_hours", ctypes.c_int32), ("n_env", ctypes.c_int32),
                ("n_rp", ctypes.c_int32), ("int_mode", ctypes.c_int32), ("max_iter", ctypes.c_int32),
                ("check_every", ctypes.c_int32), ("discount", ctypes.c_double), ("flags", ctypes.c_int32),
                ("n_groups", ctypes.c_int32)]


class Problem(ctypes.Structure):
    _fields_ = [("params", c_dp), ("home_type", c_dp), ("draw_hourly", c_dp), ("oat", c_dp), ("ghi", c_dp),
                ("tou", c_dp), ("reward_price", c_dp), ("start_index", ctypes.c_int32),
                ("home_offset", ctypes.c_int32), ("seed", ctypes.c_uint64), ("workspace", c_dp),
                ("home_stride", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Hash(ctypes.Structure):
    _fields_ = [("vals", c_dp), ("fc", c_dp)]


class Out(ctypes.Structure):
    _fields_ = [("status", c_dp), ("iters", c_dp), ("obj", c_dp), ("relax_obj", c_dp), ("hist", c_dp),
                ("cycles", c_dp), ("int_path", c_dp)]


class Explicit(ctypes.Structure):
    _fields_ = [("t", c_dp), ("T0", c_dp), ("Tw0", c_dp), ("E0", c_dp), ("counter", c_dp), ("winter", c_dp),
                ("draw", c_dp), ("oat", c_dp), ("ghi", c_dp), ("price", c_dp)]


class Episodes(ctypes.Structure):
    """dragg_mpc_episodes: the groups' own seeds (uint64), start indices and timesteps (int32), each [G]."""
    _fields_ = [("seed", c_dp), ("start_index", c_dp), ("timestep", c_dp)]


class Env(ctypes.Structure):
    """dragg_mpc_env: a vector environment's device-resident state and history stores (dragg_mpc_env_file,
    dragg_mpc_env_reset)."""
    _fields_ = [("num_timesteps", ctypes.c_int32), ("prev_timesteps", ctypes.c_int32),
                ("max_poss_load", ctypes.c_double), ("start_load", ctypes.c_double), ("ran", c_dp), ("clock", c_dp),
                ("max_load", c_dp), ("min_load", c_dp), ("tracked", c_dp), ("obs", c_dp), ("sums", c_dp),
                ("status_hist", c_dp), ("path_hist", c_dp), ("hist", c_dp), ("agg_hist", c_dp)]


ENV_PREV_MAX = 128             # DRAGG_ENV_PREV_MAX: the tracked loads the device setpoint takes
OBS_KEYS = ("agg_load", "forecast_load", "agg_cost", "agg_setpoint", "timestep")    # rows of dragg_mpc_env.obs


class Plan(ctypes.Structure):
    """dragg_mpc_plan: the masks of the chosen forecast keys and vals rows, and the outputs of
    dragg_mpc_plan_groups (curve / count [G][nk][H], stats [G][nr][4])."""
    _fields_ = [("fc_keys", ctypes.c_uint32), ("val_rows", ctypes.c_uint32), ("curve", c_dp), ("count", c_dp),
                ("stats", c_dp)]


class Paths(ctypes.Structure):
    """dragg_mpc_paths: the K-step rollouts of C candidates per episode and the outputs of dragg_mpc_select_paths
    (choice [E], score [C * E] or NULL)."""
    _fields_ = [("steps", ctypes.c_int32), ("num_timesteps", ctypes.c_int32), ("prev_timesteps", ctypes.c_int32),
                ("fresh_load", ctypes.c_double), ("sums", c_dp), ("ran", c_dp), ("tracked", c_dp), ("target", c_dp),
                ("weights", c_dp), ("prices", c_dp), ("n_rp", ctypes.c_int32), ("choice", c_dp), ("score", c_dp)]


class Classes(ctypes.Structure):
    """dragg_mpc_classes: P price classes and the community's map (device int32 [Nb], by base home)."""
    _fields_ = [("n_classes", ctypes.c_int32), ("price_class", c_dp)]


CLASS_MAX = 64                 # DRAGG_CLASS_MAX: the price classes a community can hold
TYPE_CLASS_NAMES = ("base", "pv_only", "battery_only", "pv_battery")      # price_classes="type": class = home type


def price_class_map(classes, n_homes, n_classes=None):
    """A community's price-class map as host values: `classes` (an int sequence, one per base home) and P
    (`n_classes`; None: the largest class + 1) -> (int32 array [n_homes], P).  ValueError for a wrong length, a
    value outside 0 .. P - 1, or P outside 1 .. CLASS_MAX: no such map reaches the device."""
    c = np.asarray(classes.cpu() if hasattr(classes, "cpu") else classes)
    if c.ndim != 1 or len(c) != int(n_homes):
        raise ValueError(f"price classes: one per base home ({n_homes}), not {list(c.shape)}")
    if len(c) and not np.all(c == np.floor(c.astype(float))):
        raise ValueError("price classes are integers")
    c = c.astype(np.int64)
    P = int(n_classes) if n_classes is not None else (int(c.max()) + 1 if len(c) else 1)
    if not 1 <= P <= CLASS_MAX:
        raise ValueError(f"n_classes must lie in 1..{CLASS_MAX}, not {P}")
    if len(c) and (c.min() < 0 or c.max() >= P):
        raise ValueError(f"price classes must lie in 0..{P - 1}, found {int(c.min())}..{int(c.max())}")
    return c.astype(np.int32), P


# electric vehicles (dragg_ev_param, dragg_ev_key, dragg_ev_val, dragg_ev_status)
EV_PARAMS = ["CAP", "EMIN", "EMAX", "RATE", "ETAC", "ETAD", "EINIT", "V2G", "DEPART", "RETURN", "TRIP", "EREQ"]
NEVP = len(EV_PARAMS)
EVP = {k: i for i, k in enumerate(EV_PARAMS)}
EV_KEYS = ["p_ev_ch", "p_ev_disch", "e_ev_opt", "cost_ev"]
NEVK = len(EV_KEYS)
EV_VAL_KEYS = EV_KEYS + ["forecast_p_ev"]
NEVV = len(EV_VAL_KEYS)
EVK = {k: i for i, k in enumerate(EV_VAL_KEYS)}
EV_OPTIMAL, EV_INFEASIBLE = 0, 1
EV_WAVES = 4                   # DRAGG_EV_WAVES: vehicles per workgroup


class Ev(ctypes.Structure):
    """dragg_mpc_ev: a fleet's parameter rows, state (vals [NEVV][M], fc [M][NEVK][H]), status and objective."""
    _fields_ = [("params", c_dp), ("vals", c_dp), ("fc", c_dp), ("status", c_dp), ("obj", c_dp),
                ("day_offset", ctypes.c_int32), ("n_vehicles", ctypes.c_int32)]


class EvExplicit(ctypes.Structure):
    """dragg_mpc_ev_explicit: per-stage inputs [H][M] (row k of lo / hi: the box of E_{k+1}) and E0 [M]."""
    _fields_ = [("price", c_dp), ("rate_ch", c_dp), ("rate_dis", c_dp), ("drain", c_dp), ("lo", c_dp), ("hi", c_dp),
                ("E0", c_dp)]


PLAN_WAYS = 16                 # DRAGG_PLAN_WAYS: the partial sums of a plan entry (part of its summation order)
# the forecast keys a plan curve can hold (dragg_fc_key, bit k of dragg_mpc_plan.fc_keys) and the vals rows a plan
# statistic can hold (dragg_val, bit r of val_rows), by their short names
PLAN_KEYS = ("p_grid", "forecast_p_grid", "p_load", "temp_in_ev", "temp_wh_ev", "hvac_cool", "hvac_heat", "wh_heat",
             "cost", "waterdraws", "p_pv", "u_pv_curt", "p_batt_ch", "p_batt_disch", "e_batt")
PLAN_ROWS = PLAN_KEYS + ("temp_in_opt", "temp_wh_opt", "correct_solve", "solve_counter")
PLAN_STATS = ("count", "sum", "min", "max")                     # the last axis of dragg_mpc_plan.stats


def plan_select(keys, rows=()):
    """The chosen forecast keys and vals rows -- each a short name (PLAN_KEYS / PLAN_ROWS), a hash field name
    (FC_KEYS / VAL_KEYS) or an index -- as (fc_keys mask, val_rows mask, key indices, row indices).  The indices
    are ascending and without repeats whatever the order given: that is the order of the outputs' key axis."""
    def pick(items, short, long, what):
        if isinstance(items, (str, int)):
            items = (items,)
        idx = set()
        for x in items:
            if isinstance(x, str):
                if x not in short and x not in long:
                    raise ValueError(f"{x!r} is no {what} (one of {list(short)})")
                x = short.index(x) if x in short else long.index(x)
            if not 0 <= int(x) < len(short):
                raise ValueError(f"{what} index {x} outside 0..{len(short) - 1}")
            idx.add(int(x))
        idx = sorted(idx)
        return sum(1 << i for i in idx), idx
    km, ki = pick(keys, PLAN_KEYS, FC_KEYS, "plan key")
    rm, ri = pick(rows, PLAN_ROWS, VAL_KEYS, "plan row")
    return km, rm, ki, ri


def plan_shape(keys, rows=(), G=1, H=1):
    """The shapes of dragg_mpc_plan_groups' outputs for these keys and rows: (curve and count [G][nk][H], stats
    [G][nr][4])."""
    _, _, ki, ri = plan_select(keys, rows)
    return (int(G), len(ki), int(H)), (int(G), len(ri), len(PLAN_STATS))


class Lag(ctypes.Structure):
    _fields_ = [("clock", c_dp), ("skipped", c_dp), ("narrow", c_dp), ("side_workspace", c_dp)]


def lag_list_ints(n):
    """DRAGG_LAG_LIST_INTS(n): a lag-mode list (entries, length, take counter)."""
    return n + 4


# a work-list entry's home field (mpc_kernel.hip's HOME_MASK; bits 28-31: flags and the deferred chain)
LIST_HOME_MASK = 0x0FFFFFFF
WORK_LISTS = ("deferred", "steps_list", "mid_list")


class WorkspaceRegions(ctypes.Structure):
    """dragg_mpc_workspace_regions: byte offsets of the workspace's regions in order, then the total."""
    _fields_ = [(f, ctypes.c_int64) for f in ("back_pointers", "solutions", "deferred", "big_rows", "steps_list",
                                              "steps_pools", "mid_list", "mid_rows", "w_rows", "cell_rows", "total")]


def workspace_regions(dims, H=None, cells=False):
    """Byte offset of every region of the workspace for these dims, in order, and the total, from the library
    (dragg_mpc_workspace_regions_get; dragg_mpc_workspace_bytes is the total, dragg_mpc_side_workspace_bytes
    the span [deferred, w_rows)).  A list is [N] i32 entries, then its length and take counter.
    The earlier call form (N, H, cells) still works: a round-mode batch of N homes, with a reward-price list
    if `cells` (the layout depends on nothing else in the dims)."""
    if H is not None:
        dims = Dims(n_homes=dims, horizon=H, sub_steps=6, dt=1, n_rp=H if cells else 1, int_mode=INT_ROUND)
    r = WorkspaceRegions()
    check(load().dragg_mpc_workspace_regions_get(ctypes.byref(dims), ctypes.byref(r)))
    return {f: getattr(r, f) for f, _ in WorkspaceRegions._fields_}


NLAUNCH = 4                    # DRAGG_NLAUNCH: hot, big, mid, narrow (dragg_mpc_kernel_info)
LAUNCH_NAMES = ["hot", "big", "mid", "narrow"]


class KernelInfo(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int32 * NLAUNCH) for f in ("vgprs", "scratch_bytes", "lds_bytes", "threads",
                                                         "blocks_per_cu")]


EXPORTS = ["dragg_mpc_abi_version", "dragg_mpc_strerror", "dragg_mpc_lds_bytes", "dragg_mpc_workspace_bytes",
           "dragg_mpc_workspace_regions_get", "dragg_mpc_kernel_info_get", "dragg_mpc_step",
           "dragg_mpc_solve_explicit", "dragg_mpc_aggregate", "dragg_mpc_season_noise", "dragg_mpc_reload_knobs",
           "dragg_mpc_lag_reset", "dragg_mpc_step_main", "dragg_mpc_step_side", "dragg_mpc_aggregate_rows",
           "dragg_mpc_side_workspace_bytes", "dragg_mpc_side_grid", "dragg_mpc_source_hash",
           "dragg_mpc_replicate", "dragg_mpc_aggregate_groups", "dragg_mpc_step_episodes",
           "dragg_mpc_season_noise_episodes", "dragg_mpc_adopt", "dragg_mpc_select_groups", "dragg_mpc_env_file",
           "dragg_mpc_env_reset", "dragg_mpc_plan_groups", "dragg_mpc_select_paths", "dragg_mpc_step_classes",
           "dragg_mpc_plan_classes", "dragg_mpc_ev_lds_bytes", "dragg_mpc_ev_solve_explicit", "dragg_mpc_ev_step",
           "dragg_mpc_ev_aggregate", "dragg_mpc_ev_step_episodes", "dragg_mpc_ev_aggregate_onto", "dragg_mpc_ev_adopt",
           "dragg_mpc_ev_reset"]

_LIB = None


class DraggError(RuntimeError):
    pass


def check_stamp(path):
    """The in-tree library must be built from the sources beside it: its source stamp (sha-256 of
    csrc/ and the header, dragg_amd/build.py) must equal theirs.  A stale library -- sources edited,
    checked out or copied after the build -- is refused rather than run.  DRAGG_LIB (an experiment's
    alternative build from other sources) and a tree without the sources are not checked."""
    from . import build as B
    if os.environ.get("DRAGG_LIB") or os.path.abspath(path) != os.path.abspath(B.OUT) or not B.sources_present():
        return
    got, want = B.stamp_of(path), B.source_hash()
    if got != want:
        raise DraggError(f"{path} is stale: built from sources {got}, the sources are now {want}; rebuild it "
                         "with `python -m dragg_amd.build`")


def load(path=LIB_PATH):
    """Load the HIP library (raises if it was not built, or was built from other sources)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise DraggError(f"{path} not found: build it with `python -m dragg_amd.build` "
                         "(there is no CPU fallback)")
    check_stamp(path)
    lib = ctypes.CDLL(path)
    lib.dragg_mpc_abi_version.restype = ctypes.c_int
    lib.dragg_mpc_strerror.restype = ctypes.c_char_p
    lib.dragg_mpc_strerror.argtypes = [ctypes.c_int]
    lib.dragg_mpc_lds_bytes.argtypes = [ctypes.POINTER(Dims)]
    lib.dragg_mpc_workspace_bytes.argtypes = [ctypes.POINTER(Dims)]
    lib.dragg_mpc_workspace_bytes.restype = ctypes.c_int64
    lib.dragg_mpc_side_workspace_bytes.argtypes = [ctypes.POINTER(Dims)]
    lib.dragg_mpc_side_workspace_bytes.restype = ctypes.c_int64
    lib.dragg_mpc_workspace_regions_get.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(WorkspaceRegions)]
    lib.dragg_mpc_side_grid.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(ctypes.c_int32)]
    lib.dragg_mpc_source_hash.restype = ctypes.c_char_p
    lib.dragg_mpc_step.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Problem), ctypes.POINTER(Hash),
                                   ctypes.POINTER(Out), ctypes.c_int32, c_dp, c_dp]
    lib.dragg_mpc_solve_explicit.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Problem),
                                             ctypes.POINTER(Explicit), ctypes.POINTER(Hash),
                                             ctypes.POINTER(Out), c_dp]
    lib.dragg_mpc_kernel_info_get.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(KernelInfo)]
    lib.dragg_mpc_reload_knobs.argtypes = []
    lib.dragg_mpc_reload_knobs.restype = None
    lib.dragg_mpc_aggregate.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Hash), c_dp, c_dp]
    lib.dragg_mpc_season_noise.argtypes = [ctypes.POINTER(Dims), ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32,
                                           ctypes.c_int32, c_dp, c_dp]
    lib.dragg_mpc_lag_reset.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Lag), ctypes.c_int32, c_dp]
    for f in (lib.dragg_mpc_step_main, lib.dragg_mpc_step_side):
        f.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Problem), ctypes.POINTER(Hash), ctypes.POINTER(Out),
                      ctypes.c_int32, ctypes.POINTER(Lag), c_dp]
    lib.dragg_mpc_aggregate_rows.argtypes = [ctypes.POINTER(Dims), c_dp, ctypes.c_int32, c_dp, c_dp]
    lib.dragg_mpc_replicate.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Hash), ctypes.POINTER(Hash), c_dp]
    lib.dragg_mpc_aggregate_groups.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Hash), c_dp, c_dp]
    lib.dragg_mpc_step_episodes.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Problem), ctypes.POINTER(Episodes),
                                            ctypes.POINTER(Hash), ctypes.POINTER(Out), ctypes.c_int32, c_dp, c_dp]
    lib.dragg_mpc_season_noise_episodes.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Episodes), ctypes.c_int32,
                                                    ctypes.c_int32, ctypes.c_int32, c_dp, c_dp]
    lib.dragg_mpc_adopt.argtypes = [ctypes.POINTER(Dims), ctypes.c_int32, c_dp, ctypes.POINTER(Hash), ctypes.POINTER(Out),
                                    ctypes.POINTER(Hash), ctypes.POINTER(Out), c_dp]
    lib.dragg_mpc_select_groups.argtypes = [ctypes.POINTER(Dims), ctypes.c_int32, c_dp, c_dp, c_dp, ctypes.c_int32,
                                            c_dp, c_dp]
    lib.dragg_mpc_env_file.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Env), ctypes.POINTER(Out), c_dp]
    lib.dragg_mpc_env_reset.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Env), c_dp, ctypes.POINTER(Hash), c_dp]
    lib.dragg_mpc_plan_groups.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Hash), ctypes.POINTER(Plan), c_dp]
    lib.dragg_mpc_select_paths.argtypes = [ctypes.POINTER(Dims), ctypes.c_int32, ctypes.POINTER(Paths), c_dp]
    lib.dragg_mpc_step_classes.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Problem), ctypes.POINTER(Episodes),
                                           ctypes.POINTER(Classes), ctypes.POINTER(Hash), ctypes.POINTER(Out),
                                           ctypes.c_int32, c_dp, c_dp]
    lib.dragg_mpc_plan_classes.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Hash), ctypes.POINTER(Classes),
                                           ctypes.POINTER(Plan), c_dp]
    lib.dragg_mpc_ev_lds_bytes.argtypes = [ctypes.POINTER(Dims)]
    lib.dragg_mpc_ev_solve_explicit.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Ev), ctypes.POINTER(EvExplicit), c_dp]
    lib.dragg_mpc_ev_step.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Problem), ctypes.POINTER(Ev), ctypes.c_int32,
                                      c_dp]
    lib.dragg_mpc_ev_aggregate.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Ev), c_dp, c_dp]
    lib.dragg_mpc_ev_step_episodes.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Problem), ctypes.POINTER(Episodes),
                                               ctypes.POINTER(Classes), ctypes.POINTER(Ev), ctypes.c_int32, c_dp]
    lib.dragg_mpc_ev_aggregate_onto.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Ev), c_dp, c_dp, c_dp, c_dp]
    lib.dragg_mpc_ev_adopt.argtypes = [ctypes.POINTER(Dims), ctypes.c_int32, c_dp, ctypes.POINTER(Ev),
                                       ctypes.POINTER(Ev), c_dp]
    lib.dragg_mpc_ev_reset.argtypes = [ctypes.POINTER(Dims), ctypes.POINTER(Ev), c_dp, c_dp]
    if lib.dragg_mpc_abi_version() != ABI_VERSION:
        raise DraggError("ABI version mismatch between dragg_amd and libdragg_mi355x.so")
    if not os.environ.get("DRAGG_LIB"):
        from . import build as B
        if B.sources_present() and lib.dragg_mpc_source_hash().decode() != B.source_hash():
            raise DraggError(f"{path}: the loaded library's source stamp is not the sources'")
    _LIB = lib
    return lib


def side_grid(dims):
    """The lag mode's side-pass grids (hot, mid, big, step-function) for these dims under the current
    knobs (DRAGG_SIDE_GRID clamped to each launch's per-block scratch; host-only query)."""
    g = (ctypes.c_int32 * 4)()
    check(load().dragg_mpc_side_grid(ctypes.byref(dims), g))
    return list(g)


def reload_knobs():
    """Re-read the diagnostic environment knobs (DRAGG_WAVES_PER_HOME, DRAGG_FORCE_STEP_DP): the library
    reads them once when it loads, never per step."""
    load().dragg_mpc_reload_knobs()


def kernel_info(dims):
    """The launches' registers, spills, LDS and resident workgroups per CU on the current device
    (dragg_mpc_kernel_info_get): {launch name: dict} for the hot, big, mid and narrow launches."""
    info = KernelInfo()
    check(load().dragg_mpc_kernel_info_get(ctypes.byref(dims), ctypes.byref(info)))
    return {LAUNCH_NAMES[i]: {"vgprs": info.vgprs[i], "scratch_bytes_per_lane": info.scratch_bytes[i],
                              "lds_bytes": info.lds_bytes[i], "threads": info.threads[i],
                              "blocks_per_cu": info.blocks_per_cu[i]} for i in range(NLAUNCH)}


PATH_COUNT_KEYS = ("approx_solves", "step_dp_solves", "later_launch_solves")


def path_counts(paths, dim=None):
    """The solves of an int_path tensor by kind, stacked in the order of PATH_COUNT_KEYS (bits 0-11 set, solved
    by the step-function DP, finished by a later launch), summed over `dim` (None: everything) -> int64 [3][...]."""
    import torch
    hits = [(paths & m) != 0 for m in (PATH_APPROX_MASK, PATH_STEPS, PATH_SECOND)]
    return torch.stack([h.sum() if dim is None else h.sum(dim) for h in hits])


def device_f64(x, device):
    """Host values (a list, a numpy array) or a tensor of any dtype, wherever it lives -> a float64 tensor on
    `device` (a tensor already there: no host round trip)."""
    import torch
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x, dtype=float))
    return x.detach().to(device=device, dtype=torch.float64)


def price_rows(rp, G, P, H, device, what="a batch"):
    """A reward price for G groups of P price classes at horizon H -> (the rows flat, as a contiguous float64
    tensor on `device`, and n, the entries per row).  P > 1: [G][P][n], [G][P] (class scalars; a 2-D tensor of
    that shape always means this), or one [P] / [P][n] for every group.  Else G > 1: [G][n], or one list for every
    group.  Else one list.  Host values, or a tensor: a contiguous float64 tensor already on `device` comes back
    as it is (no copy).  ValueError for another shape, or for n != 1 and n < H."""
    rp = device_f64(rp if hasattr(rp, "shape") else list(rp), device)
    G = max(G, 1)
    if P > 1:
        shape = list(rp.shape)
        if shape == [G, P]:
            rp = rp.reshape(G, P, 1)
        elif shape == [P] or (len(shape) == 2 and shape[0] == P):
            rp = rp.reshape(1, P, -1).expand(G, P, -1)
        if rp.dim() != 3 or list(rp.shape[:2]) != [G, P] or rp.shape[2] < 1:
            raise ValueError(f"{what} of {G} groups and {P} price classes takes reward prices [{G}][{P}], "
                             f"[{G}][{P}][n], [{P}] or [{P}][n], not {shape}")
    elif G > 1:
        if rp.dim() < 2:
            rp = rp.reshape(1, -1).expand(G, -1)
        if rp.dim() != 2 or rp.shape[0] != G:
            raise ValueError(f"{what} of {G} groups takes reward prices [{G}][n] or [n], not {list(rp.shape)}")
    n = rp.numel() // (G * P)
    if n != 1 and n < H:
        # np.array(rp[:H]) + tou[:H] raises in the reference (mpc_calc.py:353)
        raise ValueError(f"operands could not be broadcast together: reward_price has {n} entries, horizon is {H}")
    return rp.reshape(-1).contiguous(), n


def device_arg(x, name, device, dtype, shape=None, numel=None):
    """`x` if it is what a launch reads where it lies: a contiguous tensor on `device` of `dtype` (or of one of a
    tuple of dtypes), of `shape` or of `numel` entries where given.  ValueError otherwise."""
    import torch
    dtypes = dtype if type(dtype) is tuple else (dtype,)
    if not torch.is_tensor(x) or x.dtype not in dtypes or (shape is not None and x.shape != shape) \
            or (numel is not None and x.numel() != numel) or x.device != device or not x.is_contiguous():
        size = list(shape) if shape is not None else (f"of {numel} entries" if numel is not None else "")
        raise ValueError(f"{name} must be a contiguous device tensor {size} of {dtypes[0]}, not "
                         f"{getattr(x, 'dtype', type(x))} {list(getattr(x, 'shape', []))}")
    return x


def episode_mask(mask, E):
    """None (every episode), a bool sequence / array / tensor [E], or episode indices -> bool [E]: a bool
    tensor as it is (wherever it lives: no host round trip), anything else as a numpy array."""
    if mask is None:
        return np.ones(E, dtype=bool)
    m = mask
    if str(getattr(mask, "dtype", "")) != "torch.bool":
        m = np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask)
        if m.dtype != bool:
            idx, m = m.reshape(-1).astype(np.int64), np.zeros(E, dtype=bool)
            m[idx] = True
    if tuple(m.shape) != (E,):
        raise ValueError(f"a mask of {E} episodes, not {list(m.shape)}")
    return m


def check(rc):
    if rc != 0:
        raise DraggError(f"dragg_mpc error {rc}: {load().dragg_mpc_strerror(rc).decode()}")
    return rc


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(stream=None, device=None):
    """The launch stream: `stream`, else the current stream of `device` (of the current device
    when None)."""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return ctypes.c_void_p(s.cuda_stream)
