"""Hard cases for the EV storage LP and its independent reference.

The kernel side is `storage_lp` in dragg_amd/csrc/mpc_kernel.hip, the one recursion under the home's battery and
the vehicle, here through the vehicle's stage view (per-stage rates, drain and box).

One deterministic generator, shared by tests/test_ev_host.py (CPU: the reference pinned, the generator's own
conditions, a float64 restatement of the kernel's recursion) and tests/test_gpu_ev.py (the kernel against the
reference).  A plain helper module: no fixtures, no pytest hooks.

The model is DESIGN.md section 3.13's (the project's own: the reference has no vehicle), assembled here for
scipy's HiGHS with oracle/battery.py's METHODS and FEAS_TOL -- it shares nothing with the kernel but that
statement:

    minimise   sum_k q_k (ch_k + dis_k),                        q_k = S gamma^k price_k
    subject to E_{k+1} = E_k + a ch_k + b dis_k - drain_k,      a = ch_eff / dt,  b = 1 / (disch_eff dt)
               0 <= ch_k <= rc_k,  -rd_k <= dis_k <= 0,  lo_{k+1} <= E_{k+1} <= Emax,     k = 0 .. H - 1

A batch is one horizon at dt = 4: the cross of 5 price families and 17 vehicle families, 85 vehicles.  Every
case but the `exact_reach` family keeps its status when its E boxes move by MARGIN * capacity (narrowed where
feasible, widened where not: asserted by `cases`), so no status hangs on a tolerance.
"""
import functools
from dataclasses import dataclass

import numpy as np

from oracle.battery import FEAS_TOL, METHODS

DT, S, DISCOUNT = 4, 6, 0.92
D = 24 * DT
# 31 / 32 / 33 straddle a 64-entry segment list (2H + 1 entries); from H = 48 the clip scan takes more than one
# entry per lane; 96 is a whole day (two departures)
HORIZONS = [1, 2, 31, 32, 33, 48, 96]
PRICE_FAMILIES = ["positive", "negative", "alternating", "constant", "zero"]
VEHICLE_FAMILIES = ["typical", "typical_b", "always_home", "away_at_0", "depart_at_1", "depart_at_H", "wrap_midnight",
                    "two_departures", "v2g_off", "rate_zero", "eta_one", "at_emin", "at_emax", "trip_too_large",
                    "ereq_out_of_reach", "exact_reach", "huge"]
UNASSERTED = ("exact_reach",)          # status not asserted: feasible only with exactly full-rate charging
MARGIN = 1e-6
EV_FIELDS = ("capacity", "capacity_lower", "capacity_upper", "max_rate", "ch_eff", "disch_eff", "e_ev_init", "v2g",
             "depart_step", "return_step", "trip_kwh", "depart_soc")


def batch_id(H):
    return f"H{H}"


def stage_arrays(ev, dt, c0, H):
    """The restatement of the schedule: stage k lies at step of day (c0 + k) mod 24 dt.
    -> rc, rd, drain [H], lo, hi [H] (the box of E_{k+1})."""
    cap = float(ev["capacity"])
    emin, emax, ereq = ev["capacity_lower"] * cap, ev["capacity_upper"] * cap, ev["depart_soc"] * cap
    dep, ret = ev["depart_step"], ev["return_step"]
    s = [(c0 + k) % (24 * dt) for k in range(H + 1)]
    away = np.array([dep <= s[k] < ret for k in range(H)])
    rc = np.where(away, 0.0, float(ev["max_rate"]))
    rd = rc if ev["v2g"] else np.zeros(H)
    drain = np.where(away, ev["trip_kwh"] / float(ret - dep), 0.0)
    lo = np.array([max(emin, ereq) if s[k + 1] == dep else emin for k in range(H)])
    return rc, rd, drain, lo, np.full(H, emax)


@dataclass
class Case:
    name: str
    price_family: str
    vehicle_family: str
    ev: dict
    c0: int                       # step of day of stage 0
    E0: float
    price: np.ndarray             # [H]
    rc: np.ndarray
    rd: np.ndarray
    drain: np.ndarray
    lo: np.ndarray
    hi: np.ndarray
    feasible: bool = None         # the reference's word (None: not asserted)

    @property
    def H(self):
        return len(self.price)

    @property
    def a(self):
        return self.ev["ch_eff"] / DT

    @property
    def b(self):
        return (1.0 / self.ev["disch_eff"]) / DT

    @property
    def q(self):
        H = self.H
        return np.power(DISCOUNT * np.ones(H), np.arange(H)) * self.price * S


@dataclass
class Solution:
    feasible: bool
    cost: float = None
    ch: np.ndarray = None
    dis: np.ndarray = None
    E: np.ndarray = None


def storage_lp(q, a, b, rc, rd, drain, lo, hi, E0, method="simplex", widen=0.0):
    """The stage-varying storage LP by HiGHS; `widen` moves every E box outward (negative: inward)."""
    from scipy.optimize import linprog
    from scipy.sparse import coo_matrix
    H = len(q)
    k = np.arange(H)
    rows = np.r_[k, k, k, k[1:]]
    cols = np.r_[2 * H + k, k, H + k, 2 * H + k[1:] - 1]
    vals = np.r_[np.ones(H), np.full(H, -a), np.full(H, -b), -np.ones(H - 1)]
    A = coo_matrix((vals, (rows, cols)), shape=(H, 3 * H)).tocsr()
    rhs = -np.asarray(drain, float)
    rhs[0] += float(E0)
    bounds = ([(0.0, float(r)) for r in rc] + [(-float(r), 0.0) for r in rd] +
              [(float(l) - widen, float(h) + widen) for l, h in zip(lo, hi)])
    if any(l > h for l, h in bounds):
        return Solution(False)
    opts = {"primal_feasibility_tolerance": FEAS_TOL, "dual_feasibility_tolerance": FEAS_TOL}
    if method == "ipm":
        opts["ipm_optimality_tolerance"] = FEAS_TOL
    res = linprog(np.r_[q, q, np.zeros(H)], A_eq=A, b_eq=rhs, bounds=bounds, method=METHODS[method], options=opts)
    if res.status == 2:
        return Solution(False)
    if res.status != 0:
        raise RuntimeError(f"HiGHS ({method}) ended with status {res.status}: {res.message}")
    ch, dis, E = res.x[:H], res.x[H:2 * H], res.x[2 * H:]
    return Solution(True, float(q @ (ch + dis)), ch.copy(), dis.copy(), E.copy())


def ev_lp(c, method="simplex", widen=0.0):
    return storage_lp(c.q, c.a, c.b, c.rc, c.rd, c.drain, c.lo, c.hi, c.E0, method, widen)


def _price(fam, H, rng):
    mag = rng.uniform(0.05, 0.15, H)
    if fam == "positive":
        return mag
    if fam == "negative":
        return -mag
    if fam == "alternating":
        return mag * np.where(np.arange(H) % 2 == 0, 1.0, -1.0) * (1.0 if rng.integers(2) else -1.0)
    if fam == "constant":
        return np.full(H, 0.1)
    if fam == "zero":
        return np.zeros(H)
    raise ValueError(fam)


def _vehicle(fam, H, rng):
    """-> (ev dict, c0, E0)"""
    u = rng.uniform
    ev = {"capacity": float(u(40.0, 80.0)), "capacity_lower": float(u(0.05, 0.15)), "capacity_upper": float(u(0.85, 0.95)),
          "max_rate": float(u(6.0, 11.0)), "ch_eff": float(u(0.88, 0.95)), "disch_eff": float(u(0.90, 0.97)),
          "e_ev_init": 0.5, "v2g": bool(rng.integers(2)), "depart_step": int(rng.integers(24, 37)),
          "return_step": int(rng.integers(64, 77)), "trip_kwh": float(u(5.0, 15.0)), "depart_soc": float(u(0.5, 0.8))}
    cap, dep, ret = ev["capacity"], ev["depart_step"], ev["return_step"]
    emin, emax = ev["capacity_lower"] * cap, ev["capacity_upper"] * cap
    c0, E0 = int(rng.integers(0, D)), float(u(0.4, 0.8)) * cap
    if fam == "always_home":                   # the degenerate vehicle: the battery LP
        ev.update(trip_kwh=0.0, depart_soc=0.0, v2g=True)
        ev["depart_step"], ev["return_step"] = D + 1, D + 2        # never reached (stage_arrays only: not packed)
    elif fam == "huge":                        # always home and never clipped: the list reaches 2H + 1 entries
        ev.update(trip_kwh=0.0, depart_soc=0.0, v2g=True, capacity=1e4, max_rate=0.5)
        ev["depart_step"], ev["return_step"] = D + 1, D + 2
        E0 = 0.5 * 1e4
    elif fam == "away_at_0":
        c0, E0 = dep + 5, 0.7 * cap
    elif fam == "depart_at_1":
        c0, E0 = dep - 1, (ev["depart_soc"] + 0.05) * cap
    elif fam == "depart_at_H":
        c0 = (dep - H) % D
        E0 = ev["depart_soc"] * cap - 0.5 * min(H, 4) * ev["ch_eff"] / DT * ev["max_rate"]
    elif fam == "wrap_midnight":
        c0, E0 = D - 1 - (3 if H > 8 else 0), 0.7 * cap
    elif fam == "two_departures":              # leaving now and, at H = 96, again at k = H
        c0, E0 = dep, 0.8 * cap
    elif fam == "v2g_off":
        ev["v2g"] = False
    elif fam == "rate_zero":
        ev.update(max_rate=0.0, depart_soc=0.4, trip_kwh=float(u(0.05, 0.2)) * cap)
        E0 = 0.4 * cap + ev["trip_kwh"] + 0.05 * cap
    elif fam == "eta_one":
        ev["ch_eff"] = ev["disch_eff"] = 1.0
    elif fam == "at_emin":
        c0, E0 = (ret + 1) % D, emin
    elif fam == "at_emax":
        ev["v2g"] = True
        c0, E0 = (ret + 1) % D, emax
    elif fam == "trip_too_large":              # leaves now, three usable capacities to drive
        ev["trip_kwh"] = 3.0 * (emax - emin)
        c0 = dep
        E0 = emin + 0.5 * ev["trip_kwh"] / (ret - dep)
    elif fam == "ereq_out_of_reach":           # leaves at k = 1, a full-rate stage and 0.1 capacity short
        c0 = dep - 1
        E0 = ev["depart_soc"] * cap - ev["ch_eff"] / DT * ev["max_rate"] - 0.1 * cap
    elif fam == "exact_reach":                 # Ereq met by exactly full-rate charging until departure
        m = min(H, 3)
        ev["depart_soc"] = 0.6
        c0 = dep - m
        E0 = 0.6 * cap - m * (ev["ch_eff"] / DT * ev["max_rate"])
    return ev, c0 % D, float(E0)


@functools.lru_cache(maxsize=None)
def cases(H):
    """The cases of horizon H, in the order of the fleet's vehicles, each with the reference's status."""
    out = []
    for pi, pf in enumerate(PRICE_FAMILIES):
        for vi, vf in enumerate(VEHICLE_FAMILIES):
            rng = np.random.default_rng([H, pi, vi])
            ev, c0, E0 = _vehicle(vf, H, rng)
            rc, rd, drain, lo, hi = stage_arrays(ev, DT, c0, H)
            c = Case(f"{pf}-{vf}", pf, vf, ev, c0, E0, _price(pf, H, rng), rc, rd, drain, lo, hi)
            if vf not in UNASSERTED:
                # the status, and that it does not hang on a tolerance
                w = MARGIN * ev["capacity"]
                c.feasible = ev_lp(c).feasible
                moved = ev_lp(c, widen=-w if c.feasible else w).feasible
                assert moved == c.feasible, (c.name, H, c.feasible)
            out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(H, method="simplex"):
    return tuple(ev_lp(c, method) for c in cases(H))


def explicit_inputs(cs):
    """The [H][M] arrays and E0 [M] of EVFleet.solve_explicit for the cases `cs`."""
    col = lambda k: np.array([getattr(c, k) for c in cs]).T     # noqa: E731
    return dict(price=col("price"), rate_ch=col("rc"), rate_dis=col("rd"), drain=col("drain"), lo=col("lo"),
                hi=col("hi"), E0=np.array([c.E0 for c in cs]))


def fleet_homes(cs, H):
    """One home per case (its `ev` section; the thermal side is never solved by the fleet)."""
    homes = []
    for c in cs:
        ev = dict(c.ev)
        if not 0 <= ev["depart_step"] < ev["return_step"] <= D:     # (the degenerate vehicle: explicit inputs only)
            ev["depart_step"], ev["return_step"] = 0, 1
        homes.append({"name": c.name, "type": "base", "ev": ev,
                      "hems": {"horizon": H / DT, "hourly_agg_steps": DT, "sub_subhourly_steps": S,
                               "solver": "MI355X", "discount_factor": DISCOUNT}})
    return homes


# --------------------------------------------------------------------------------------
# A float64 restatement of the kernel's recursion (sequential numpy): the convex piecewise-linear cost-to-go as
# a sorted (slope, length) list, psi_k's two segments merged in, the origin shifted, the list cut to the box;
# recovery forward.  -> Solution
# --------------------------------------------------------------------------------------
def recursion(q, a, b, rc, rd, drain, lo, hi, E0, tol=1e-9):
    H = len(q)

    def psi(k):
        if q[k] >= 0.0:
            return (-q[k] / a, a * rc[k]), (-q[k] / b, b * rd[k])
        return (-q[k] / b, b * rd[k]), (-q[k] / a, a * rc[k])

    if not lo[H - 1] <= hi[H - 1] + tol * (1 + abs(hi[H - 1])):
        return Solution(False)
    segs = [(0.0, max(0.0, hi[H - 1] - lo[H - 1]))]
    x0 = lo[H - 1]
    rec = [None] * H
    for k in range(H - 1, -1, -1):
        (s1, l1), (s2, l2) = psi(k)
        p1 = sum(l for s, l in segs if s <= s1)
        p2 = sum(l for s, l in segs if s <= s2) + l1
        merged = sorted(segs + [(s1, l1), (s2, l2)], key=lambda t: t[0])    # stable: psi after equal slopes
        X0M = x0 + -a * rc[k] + drain[k]
        rec[k] = (X0M, p1, p2)
        tot = sum(l for _, l in merged)
        if k == 0:
            p = E0 - X0M
            if not (p >= -tol * (1 + abs(E0)) and p <= tot + tol * (1 + abs(E0))):
                return Solution(False)
            break
        cl, chi = max(0.0, lo[k - 1] - X0M), min(tot, hi[k - 1] - X0M)
        if not cl <= chi + tol * (1 + abs(hi[k - 1])):
            return Solution(False)
        pre, cut = 0.0, []
        for s, l in merged:
            ns, ne = max(pre, cl), min(pre + l, chi)
            if ne > ns:
                cut.append((s, ne - ns))
            pre += l
        segs = cut or [(0.0, 0.0)]
        x0 = X0M + cl
    E, ch, dis, Es = E0, np.zeros(H), np.zeros(H), np.zeros(H)
    for k in range(H):
        (s1, l1), (s2, l2) = psi(k)
        X0M, p1, p2 = rec[k]
        p = E - X0M
        z = -a * rc[k] + min(max(p - p1, 0.0), l1) + min(max(p - p2, 0.0), l2)
        dlt = -z
        if q[k] >= 0.0:
            c, d = (min(dlt / a, rc[k]), 0.0) if dlt >= 0.0 else (0.0, max(dlt / b, -rd[k]))
        else:
            c = min(rc[k], (dlt + b * rd[k]) / a)
            d = max(-rd[k], min(0.0, (dlt - a * c) / b))
        E = E + (a * c + b * d) - drain[k]
        ch[k], dis[k], Es[k] = c, d, E
    return Solution(True, float(q @ (ch + dis)), ch, dis, Es)


def list_length(c):
    """The longest segment list the kernel holds for case `c` at a cut (the merged list, with the zero-length
    entries the kernel keeps between the first and the last positive one): past 64, the clip scan takes more than
    one entry per lane."""
    q, a, b, H = c.q, c.a, c.b, c.H
    segs, x0, longest = [(0.0, max(0.0, c.hi[H - 1] - c.lo[H - 1]))], c.lo[H - 1], 0
    for k in range(H - 1, 0, -1):
        ar, br = (-q[k] / a, a * c.rc[k]), (-q[k] / b, b * c.rd[k])
        merged = sorted(segs + ([ar, br] if q[k] >= 0.0 else [br, ar]), key=lambda t: t[0])
        longest = max(longest, len(merged))
        X0M = x0 - a * c.rc[k] + c.drain[k]
        tot = sum(l for _, l in merged)
        cl, chi = max(0.0, c.lo[k - 1] - X0M), min(tot, c.hi[k - 1] - X0M)
        if cl > chi + 1e-9 * (1 + abs(c.hi[k - 1])):
            break
        pre, cut = 0.0, []
        for s, l in merged:
            cut.append((s, max(0.0, min(pre + l, chi) - max(pre, cl))))
            pre += l
        pos = [i for i, (_, l) in enumerate(cut) if l > 0.0]
        segs = cut[pos[0]:pos[-1] + 1] if pos else [(0.0, 0.0)]
        x0 = X0M + cl
    return longest
