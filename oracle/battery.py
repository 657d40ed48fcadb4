"""The battery LP of one solve, alone -- TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

The reference's model (`mpc_calc.py:355-373` with the battery's share of p_grid and cost,
`:405-446`; assembled whole by `oracle.mpc.build_problem`) separates into the thermal integer
programme, the PV LP and this block:

    minimise   sum_k q_k (ch_k + dis_k),                 q_k = S gamma^k price_k
    subject to E_{k+1} = E_k + (eta_c ch_k + dis_k / eta_d) / dt,   k = 0 .. H-1
               0 <= ch_k <= r,   -r <= dis_k <= 0,   Emin <= E_1 .. E_H <= Emax,

E_0 fixed and not boxed.  It is solved here as a sparse LP by scipy's HiGHS with the primal and
dual feasibility tolerances at 1e-10: the independent checker of the GPU's piecewise-linear
value-function DP (`storage_lp` in dragg_amd/csrc/mpc_kernel.hip, the one recursion under the
battery and the vehicle, here through its battery view), which shares nothing with it but the
statement above.  `dragg_amd` never imports this module.
"""
from dataclasses import dataclass

import numpy as np

METHODS = {"simplex": "highs-ds", "ipm": "highs-ipm"}
FEAS_TOL = 1e-10


@dataclass
class BatterySolution:
    feasible: bool
    cost: float = None          # sum_k q_k (ch_k + dis_k) at the optimum
    ch: np.ndarray = None       # [H]
    dis: np.ndarray = None      # [H]
    E: np.ndarray = None        # [H] E_1 .. E_H
    q: np.ndarray = None        # [H] the stage weights


def weights(hc, price):
    """q_k = S gamma^k price_k (`mpc_calc.py:441-446`: cost_k = price_k p_grid_k, p_grid carries
    S (ch + dis), the objective weighs cost_k by gamma^k)."""
    H = hc.H
    return np.power(hc.discount * np.ones(H), np.arange(H)) * np.asarray(price, float)[:H] * hc.S


def soc_step(hc, E, ch, dis):
    """E_{k+1} of the reference's recursion (`mpc_calc.py:363-365`)."""
    b = hc.batt
    return E + (b["eta_c"] * ch + dis / b["eta_d"]) / hc.dt


def battery_lp(hc, E0, price, method="simplex"):
    """The battery block of home `hc` (an `oracle.mpc.HomeConst` with a battery) from the state of
    charge `E0` under the total prices `price` [H].  method: "simplex" (HiGHS dual simplex) or "ipm"
    (HiGHS interior point with crossover).  -> BatterySolution (feasible False: no trajectory)."""
    from scipy.optimize import linprog
    from scipy.sparse import coo_matrix
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, not {method!r}")
    H, dt, b = hc.H, hc.dt, hc.batt
    q = weights(hc, price)
    a_c, a_d = b["eta_c"] / dt, (1.0 / b["eta_d"]) / dt
    # columns: ch [0, H), dis [H, 2H), E_1 .. E_H [2H, 3H); row k: E_{k+1} - E_k - a_c ch_k - a_d dis_k = 0
    k = np.arange(H)
    rows = np.r_[k, k, k, k[1:]]
    cols = np.r_[2 * H + k, k, H + k, 2 * H + k[1:] - 1]
    vals = np.r_[np.ones(H), np.full(H, -a_c), np.full(H, -a_d), -np.ones(H - 1)]
    A = coo_matrix((vals, (rows, cols)), shape=(H, 3 * H)).tocsr()
    rhs = np.zeros(H)
    rhs[0] = float(E0)
    bounds = [(0.0, b["rate"])] * H + [(-b["rate"], 0.0)] * H + [(b["Emin"], b["Emax"])] * H
    opts = {"primal_feasibility_tolerance": FEAS_TOL, "dual_feasibility_tolerance": FEAS_TOL}
    if method == "ipm":
        opts["ipm_optimality_tolerance"] = FEAS_TOL
    res = linprog(np.r_[q, q, np.zeros(H)], A_eq=A, b_eq=rhs, bounds=bounds, method=METHODS[method], options=opts)
    if res.status == 2:
        return BatterySolution(False, q=q)
    if res.status != 0:
        raise RuntimeError(f"HiGHS ({method}) ended with status {res.status}: {res.message}")
    ch, dis, E = res.x[:H], res.x[H:2 * H], res.x[2 * H:]
    return BatterySolution(True, float(q @ (ch + dis)), ch.copy(), dis.copy(), E.copy(), q)
