"""The EV storage LP kernel (`storage_lp` through the vehicle's stage view, dragg_mpc_ev_*) on the GPU -- the one
recursion that also solves the home's battery, through the battery's view: against the independent LP of
tests/ev_cases.py, against the home kernel's battery LP on the degenerate vehicle, the closed-loop step against
the explicit entry, groups, and the entries' edges.

The cost bar is test_gpu_battery.py's: 1e-9 * max(1, |ref|).  tests/test_ev_host.py confirms on the CPU that a
float64 restatement of the recursion stays within it on every case (worst 7.8e-15) and that the reference's two
HiGHS methods agree, so no family is left out.  Measured on the MI355X, worst |kernel - reference| /
max(1, |reference|) per batch: see DESIGN.md section 3.13.
"""
import ctypes

import numpy as np
import pytest

from tests import battery_cases as BC
from tests import ev_cases as EC

pytestmark = pytest.mark.gpu

COST_TOL = 1e-9
EPS = 2.0 ** -52
_SOLVED = {}


def _state(f):
    import torch
    torch.cuda.synchronize()
    return dict(vals=f.vals.cpu().numpy(), fc=f.fc.cpu().numpy(), status=f.status.cpu().numpy(), obj=f.obj.cpu().numpy())


def _same(a, b, what):
    for k in ("status", "vals", "fc", "obj"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _solved(H):
    if H not in _SOLVED:
        from dragg_amd.ev import EVFleet
        cs = EC.cases(H)
        f = EVFleet(EC.fleet_homes(cs, H))
        f.solve_explicit(**EC.explicit_inputs(cs))
        _SOLVED[H] = _state(f)
    return _SOLVED[H]


@pytest.mark.parametrize("H", EC.HORIZONS, ids=EC.batch_id)
def test_ev_lp_against_independent_lp(H, gpu):
    """One solve_explicit of the batch's 85 vehicles.  Per case: optimal iff the LP is feasible (the exact_reach
    family: not asserted); the cost within 1e-9 * max(1, |ref|); the trajectory inside its bounds and on the
    recursion within 8 H eps max(1, Emax, max_rate); the reported objective equal to the one recomputed from the
    trajectory (to the rounding of the sum); the vals rows equal to entry 0 of their fields."""
    from dragg_amd import _lib as L
    res, cs, ref = _solved(H), EC.cases(H), EC.reference(H)
    ch_a, dis_a, e_a, cost_a = (res["fc"][L.EVK[k]] for k in L.EV_KEYS)
    worst, n = 0.0, 0
    for i, (c, rf) in enumerate(zip(cs, ref)):
        st = res["status"][i]
        if c.feasible is not None:
            assert st == (L.EV_OPTIMAL if rf.feasible else L.EV_INFEASIBLE), (c.name, st, rf.feasible)
        if st != L.EV_OPTIMAL or not rf.feasible:
            if st != L.EV_OPTIMAL:
                assert np.isnan(res["obj"][i]), c.name
            continue
        ch, dis, E = ch_a[:, i], dis_a[:, i], e_a[:, i]
        ours = float(c.q @ (ch + dis))
        gap = abs(ours - rf.cost) / max(1.0, abs(rf.cost))
        worst = max(worst, gap)
        assert gap <= COST_TOL, (c.name, ours, rf.cost, gap)
        ftol = 8 * H * EPS * max(1.0, c.hi.max(), c.ev["max_rate"])
        assert (ch >= -ftol).all() and (ch <= c.rc + ftol).all(), c.name
        assert (dis <= ftol).all() and (dis >= -c.rd - ftol).all(), c.name
        assert (E >= c.lo - ftol).all() and (E <= c.hi + ftol).all(), (c.name, (c.lo - E).max(), (E - c.hi).max())
        rec = np.r_[c.E0, E[:-1]] + c.a * ch + c.b * dis - c.drain
        assert np.abs(rec - E).max() <= ftol, (c.name, np.abs(rec - E).max())
        # the reported objective: the same sum with the device's q_k (its pow may differ from numpy's in the last
        # place: 2 eps per weight, one per product, H for the sum)
        terms = c.q * (ch + dis)
        assert abs(terms.sum() - res["obj"][i]) <= (H + 4) * EPS * np.abs(terms).sum(), (c.name, terms.sum(), res["obj"][i])
        assert np.array_equal(cost_a[:, i], c.price * (EC.S * (ch + dis))), c.name
        for key, row in zip(L.EV_KEYS, (ch, dis, E, cost_a[:, i])):
            assert res["vals"][L.EVK[key], i] == row[0], (c.name, key)
        assert res["vals"][L.EVK["forecast_p_ev"], i] == (ch[1] + dis[1] if H > 1 else 0.0), c.name
        n += 1
    print(f"{EC.batch_id(H)}: {n} feasible cases at the LP optimum, worst cost gap {worst:.2e}")
    assert n >= len(cs) // 2


@pytest.mark.parametrize("H", EC.HORIZONS, ids=EC.batch_id)
def test_fallback_rows_equal_the_numpy_rule(H, gpu):
    """The infeasible cases' rows are the uncontrolled rule's, bit for bit."""
    from dragg_amd import _lib as L
    from dragg_amd.ev import ev_fallback, pack_evs
    res, cs = _solved(H), EC.cases(H)
    P, _ = pack_evs(EC.fleet_homes(cs, H))
    x = EC.explicit_inputs(cs)
    ch, E = ev_fallback(P, EC.DT, x["rate_ch"], x["drain"], x["E0"])
    bad = res["status"] == L.EV_INFEASIBLE
    assert bad.sum() >= 8
    assert np.array_equal(res["fc"][L.EVK["p_ev_ch"]][:, bad], ch[:, bad])
    assert np.array_equal(res["fc"][L.EVK["e_ev_opt"]][:, bad], E[:, bad])
    assert (res["fc"][L.EVK["p_ev_disch"]][:, bad] == 0.0).all()


@pytest.mark.parametrize("batch", BC.BATCHES, ids=BC.batch_id)
def test_degenerate_vehicle_is_the_battery(batch, gpu):
    """The two stage views of the one recursion agree where they state the same problem.  An always-home,
    zero-trip, v2g vehicle with Ereq <= Emin is the home kernel's battery LP: on the cases of
    tests/battery_cases.py the explicit EV entry's p_ev_ch, p_ev_disch and e_ev_opt equal the home kernel's
    p_batt_ch, p_batt_disch and e_batt_opt bit for bit at every home whose status is optimal, and the vehicle is
    infeasible exactly where the home is not optimal.  On the discount = 1 batches the reported objective equals the
    recomputed one exactly (elsewhere the device's pow may differ from numpy's in the last place, and
    test_ev_lp_against_independent_lp holds the two to the rounding of the sum)."""
    from dragg_amd import _lib as L
    from dragg_amd.ev import EVFleet
    from tests.test_gpu_battery import _battery_fields, _solved as home_solved
    H, dt, disc = batch
    cs = BC.cases(batch)
    home = home_solved(batch)
    homes = []
    for c in cs:
        b = c.home["battery"]
        homes.append({"name": c.name, "type": "base", "hems": c.home["hems"],
                      "ev": dict(capacity=b["capacity"], capacity_lower=b["capacity_lower"],
                                 capacity_upper=b["capacity_upper"], max_rate=b["max_rate"], ch_eff=b["ch_eff"],
                                 disch_eff=b["disch_eff"], e_ev_init=b["e_batt_init"], v2g=True, depart_step=0,
                                 return_step=1, trip_kwh=0.0, depart_soc=0.0)})
    f = EVFleet(homes)
    assert (f.H, f.dt, f.S) == (H, dt, home["S"])
    n = len(cs)
    # (the home kernel's own parameter values: pack_homes' expressions)
    batt = [c.home["battery"] for c in cs]
    col = lambda fn: np.tile(np.array([fn(b) for b in batt]), (H, 1))     # noqa: E731
    rate = col(lambda b: float(b["max_rate"]))
    f.solve_explicit(price=np.array([c.price for c in cs]).T, rate_ch=rate, rate_dis=rate, drain=np.zeros((H, n)),
                     lo=col(lambda b: float(b["capacity_lower"]) * float(b["capacity"])),
                     hi=col(lambda b: float(b["capacity_upper"]) * float(b["capacity"])),
                     E0=np.array([c.E0 for c in cs]))
    ev = _state(f)
    (bf, bv) = _battery_fields(home)
    opt = home["status"] == L.ST_OPTIMAL
    assert np.array_equal(ev["status"] == L.EV_OPTIMAL, opt), [c.name for c, a, b in
                                                                zip(cs, ev["status"], opt) if (a == 0) != b]
    assert opt.sum() >= n // 2
    for j, key in enumerate(("p_ev_ch", "p_ev_disch", "e_ev_opt")):
        x, y = ev["fc"][L.EVK[key]], bf[j]
        diff = [(cs[i].name, int(k), float(x[k, i]).hex(), float(y[k, i]).hex())
                for k, i in np.argwhere((x != y) & opt[None, :])]
        assert not diff, (key, len(diff), diff[:6])
        assert np.array_equal(ev["vals"][L.EVK[key]][opt], bv[j][opt]), key
    if disc == 1.0:
        # gamma^k is exactly 1: q_k = price_k S on the host as on the device, so the reported objective EQUALS the
        # one recomputed from the trajectory (ascending k, no contraction), bit for bit
        ch, dis = ev["fc"][L.EVK["p_ev_ch"]], ev["fc"][L.EVK["p_ev_disch"]]
        for i in np.flatnonzero(opt):
            obj = 0.0
            for k in range(H):
                obj += (1.0 * cs[i].price[k] * home["S"]) * (ch[k, i] + dis[k, i])
            assert obj == ev["obj"][i], (cs[i].name, obj, ev["obj"][i])


# ---------------------------------------------------------------------------------------- the closed loop
LOOP_H, LOOP_STEPS, LOOP_OFFSET = 24, 100, 95      # midnight falls at t = 1 and t = 97


def _loop_homes():
    rng = np.random.default_rng(2024)
    homes = []
    for i in range(16):
        ev, _, _ = EC._vehicle("typical", LOOP_H, rng)
        ev["e_ev_init"] = float(rng.uniform(0.4, 0.8))
        if i % 8 == 3:
            ev["trip_kwh"] = 3.0 * ev["capacity"]           # no trajectory once the trip is in sight
        if i % 8 == 5:
            ev["depart_soc"] = 0.99                          # above Emax: out of reach
        homes.append({"name": f"ev-{i}", "type": "base", "ev": ev,
                      "hems": {"horizon": LOOP_H / EC.DT, "hourly_agg_steps": EC.DT, "sub_subhourly_steps": EC.S,
                               "solver": "MI355X", "discount_factor": EC.DISCOUNT}})
    return homes


@pytest.fixture(scope="module")
def loop(gpu):
    """16 vehicles x 100 steps at H = 24 across two midnights, the step entry beside the explicit one: per step
    the state both left, the host-built inputs and the state before."""
    from dragg_amd import _lib as L
    from dragg_amd.ev import EVFleet, pack_evs
    homes = _loop_homes()
    rng = np.random.default_rng(7)
    tou = 0.07 + 0.04 * rng.standard_normal(LOOP_STEPS + LOOP_H + 8)        # some negative
    rp = 0.02 * rng.standard_normal(LOOP_H)
    start = 3
    a = EVFleet(homes, tou, start, rp, day_offset=LOOP_OFFSET)
    b = EVFleet(homes, tou, start, rp, day_offset=LOOP_OFFSET)
    P, _ = pack_evs(homes)
    E, steps = P[L.EVP["EINIT"]].copy(), []
    for t in range(LOOP_STEPS):
        rows = [EC.stage_arrays(h["ev"], EC.DT, (LOOP_OFFSET + t) % EC.D, LOOP_H) for h in homes]
        x = {k: np.array([r[j] for r in rows]).T for j, k in enumerate(("rate_ch", "rate_dis", "drain", "lo", "hi"))}
        x["price"] = np.tile((rp + tou[start + t:start + t + LOOP_H])[:, None], (1, len(homes)))
        a.step(t)
        b.solve_explicit(E0=E, **x)
        sa, sb = _state(a), _state(b)
        steps.append(dict(t=t, a=sa, b=sb, x=x, E0=E.copy()))
        E = sa["vals"][L.EVK["e_ev_opt"]].copy()
    return dict(homes=homes, P=P, steps=steps)


def test_step_equals_explicit(loop):
    """Each step's state equals solve_explicit on inputs rebuilt on the host from the previous state, bit for
    bit; the fallback rows equal the numpy rule bit for bit."""
    from dragg_amd import _lib as L
    from dragg_amd.ev import ev_fallback
    n_bad = 0
    for s in loop["steps"]:
        _same(s["a"], s["b"], f"step {s['t']}")
        bad = s["a"]["status"] == L.EV_INFEASIBLE
        if bad.any():
            ch, E = ev_fallback(loop["P"], EC.DT, s["x"]["rate_ch"], s["x"]["drain"], s["E0"])
            assert np.array_equal(s["a"]["fc"][L.EVK["p_ev_ch"]][:, bad], ch[:, bad]), s["t"]
            assert np.array_equal(s["a"]["fc"][L.EVK["e_ev_opt"]][:, bad], E[:, bad]), s["t"]
            n_bad += int(bad.sum())
    assert n_bad > 0
    assert sum(int((s["a"]["status"] == L.EV_OPTIMAL).sum()) for s in loop["steps"]) > 8 * LOOP_STEPS


def test_closed_loop(loop):
    """Every away stage played has ch = dis = 0 and E falling by the drain; every optimal step keeps E in
    [Emin, Emax]; a vehicle whose steps were all optimal since its departure entered the horizon leaves with
    E >= Ereq."""
    from dragg_amd import _lib as L
    P, steps = loop["P"], loop["steps"]
    emin, emax, ereq = P[L.EVP["EMIN"]], P[L.EVP["EMAX"]], P[L.EVP["EREQ"]]
    ftol = 8 * LOOP_H * EPS * np.maximum(1.0, np.maximum(emax, P[L.EVP["RATE"]]))
    n_away = n_leave = 0
    for s in steps:
        v, opt = s["a"]["vals"], s["a"]["status"] == L.EV_OPTIMAL
        away = s["x"]["rate_ch"][0] == 0.0
        E1 = v[L.EVK["e_ev_opt"]]
        assert (v[L.EVK["p_ev_ch"]][away] == 0.0).all() and (v[L.EVK["p_ev_disch"]][away] == 0.0).all(), s["t"]
        fall = s["E0"] - s["x"]["drain"][0]
        assert (np.abs(E1 - np.where(opt, fall, np.clip(fall, 0.0, P[L.EVP["CAP"]])))[away] <= ftol[away]).all(), s["t"]
        n_away += int(away.sum())
        assert (E1[opt] >= emin[opt] - ftol[opt]).all() and (E1[opt] <= emax[opt] + ftol[opt]).all(), s["t"]
        # leaving now: stage 0 lies at the departure step
        t = s["t"]
        if t >= LOOP_H:
            leaving = np.array([(LOOP_OFFSET + t) % EC.D == h["ev"]["depart_step"] for h in loop["homes"]])
            since = np.all([steps[u]["a"]["status"] == L.EV_OPTIMAL for u in range(t - LOOP_H, t)], axis=0)
            ok = leaving & since
            assert (s["E0"][ok] >= np.maximum(emin, ereq)[ok] - ftol[ok]).all(), t
            n_leave += int(ok.sum())
    assert n_away > 100 and n_leave >= 4, (n_away, n_leave)


# ---------------------------------------------------------------------------------------- groups
@pytest.mark.parametrize("Mb", [1, 5, 77])
def test_groups_equal_single_fleets(Mb, gpu):
    """A G = 3 fleet under three price rows equals three single fleets, state and sums bit for bit; a
    workgroup's four vehicles straddle groups and the last block is ragged."""
    import torch
    from dragg_amd.ev import EVFleet
    H = 32
    homes = EC.fleet_homes(EC.cases(H), H)[:Mb]
    rng = np.random.default_rng(Mb)
    tou = 0.07 + 0.03 * rng.standard_normal(H + 8)
    rows = 0.03 * rng.standard_normal((3, H))
    g = EVFleet(homes, tou, 0, rows, day_offset=20, groups=3)
    singles = [EVFleet(homes, tou, 0, rows[i], day_offset=20) for i in range(3)]
    assert g.M == 3 * Mb
    for t in range(3):
        g.step(t)
        sums = g.aggregate().clone()
        sg = _state(g)
        for i, f in enumerate(singles):
            f.step(t)
            s1 = _state(f)
            sl = slice(i * Mb, (i + 1) * Mb)
            assert np.array_equal(sg["vals"][:, sl], s1["vals"], equal_nan=True), (t, i)
            assert np.array_equal(sg["fc"][:, :, sl], s1["fc"], equal_nan=True), (t, i)
            assert np.array_equal(sg["status"][sl], s1["status"]) and np.array_equal(sg["obj"][sl], s1["obj"], equal_nan=True)
            assert torch.equal(sums[i], f.aggregate()), (t, i)
    # the sums are the three fields' sums (to rounding: the kernel's order is its own)
    v = sg["vals"][:, :Mb]
    from dragg_amd import _lib as L
    want = [(v[L.EVK["p_ev_ch"]] + v[L.EVK["p_ev_disch"]]).sum(), v[L.EVK["forecast_p_ev"]].sum(), v[L.EVK["cost_ev"]].sum()]
    assert np.allclose(sums[0].cpu().numpy(), want, rtol=1e-12, atol=1e-12)
    # replicate_from: every group the base fleet's state
    g.replicate_from(singles[1])
    sg, s1 = _state(g), _state(singles[1])
    for i in range(3):
        assert np.array_equal(sg["vals"][:, i * Mb:(i + 1) * Mb], s1["vals"], equal_nan=True)


# ---------------------------------------------------------------------------------------- edges
def test_edges(gpu):
    """M = 0: every entry a no-op, zero sums; H = 160: every EV entry answers DRAGG_E_HORIZON and leaves the state
    as it was; a community without ev sections builds no fleet."""
    import torch
    from dragg_amd import _lib as L
    from dragg_amd.ev import EVFleet, build_fleet
    H = 32
    homes = EC.fleet_homes(EC.cases(H), H)[:6]
    bare = [{k: v for k, v in h.items() if k != "ev"} for h in homes]
    assert build_fleet(bare) is None
    e = EVFleet(bare, [0.1] * 64, template_home=bare[0])
    assert e.M == 0
    e.step(0)
    e.solve_explicit(*[np.zeros((H, 0))] * 6, np.zeros(0))
    assert torch.equal(e.aggregate(), torch.zeros(3, dtype=torch.float64, device=e.device))
    f = build_fleet(homes, tou=[0.1] * 64)
    f.step(0)
    before = _state(f)
    lib = L.load()
    d = L.Dims.from_buffer_copy(f.dims)
    d.horizon = 160
    z = torch.zeros((160, f.M), dtype=torch.float64, device=f.device)
    ex = L.EvExplicit(*[L.ptr(z)] * 6, L.ptr(z[0]))
    out = torch.full((3,), 7.0, dtype=torch.float64, device=f.device)
    assert lib.dragg_mpc_ev_lds_bytes(ctypes.byref(d)) == -4
    assert lib.dragg_mpc_ev_step(d, f._problem(), f._ev(), 1, None) == -4
    assert lib.dragg_mpc_ev_solve_explicit(d, f._ev(), ex, None) == -4
    assert lib.dragg_mpc_ev_aggregate(d, f._ev(), L.ptr(out), None) == -4
    _same(before, _state(f), "H = 160")
    assert (out == 7.0).all()
