"""The battery LP reference (oracle/battery.py) and the hard cases of tests/battery_cases.py (CPU only).

oracle/battery.py is the checker of the kernel's battery DP in tests/test_gpu_battery.py.  Here it
is pinned to the reference's own recorded LP relaxations, and the generator's conditions -- the
share of feasible and infeasible cases, that the reference agrees with itself far below the GPU
test's bar, that the thermal side of every case has a schedule -- are checked without a GPU.
"""
import math

import numpy as np
import pytest

from oracle import battery as B
from oracle import mpc as M
from oracle import thermal as TH
from tests import battery_cases as BC
from tests import fixtures as F

# The two HiGHS methods against each other on the fixtures' battery records, measured: 0 on 1,030
# of the 1,031 records and 1.24e-16 (one rounding of the cost) on one.  The pin's tolerance is
# ten times that, relative to max(1, |optimum|).
PIN_SELF_MEASURED = 1.24e-16
PIN_TOL = 10 * PIN_SELF_MEASURED

# tests/test_gpu_battery.py holds the kernel's battery cost to COST_TOL * max(1, |reference|); the
# reference's own two methods must agree to a tenth of it on every case
COST_TOL = 1e-9


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _cost(q, ch, dis):
    """sum_k q_k (ch_k + dis_k), correctly rounded (no dependence on a summation order)."""
    return math.fsum(float(w) * (float(c) + float(d)) for w, c, d in zip(q, ch, dis))


@pytest.mark.parametrize("name", F.scenarios())
def test_battery_lp_reproduces_recorded_relaxations(name):
    """Every battery record of the golden fixtures whose recorded LP relaxation is optimal: the
    model is separable (test_oracle_golden.py::test_model_is_separable), so the battery share
    q.(ch + dis) of the recorded optimum is the optimum of the battery LP alone.  Measured over the
    1,031 such records: dual simplex against interior point at most 1.24e-16, the recorded
    trajectory against either at most 1.24e-16 (relative to max(1, |optimum|); the optima are
    bang-bang vertices HiGHS reproduces to the last bit).  Tolerance: 10 x the self-agreement."""
    d = F.load(name)
    homes = {h["name"]: h for h in d["homes"]}
    n, worst_self, worst_rec = 0, 0.0, 0.0
    for r in d["records"]:
        if r["E0"] is None or r["lp_status"] != 0:
            continue
        hc = M.home_const(homes[r["name"]])
        ds = B.battery_lp(hc, r["E0"], r["total_price"], method="simplex")
        ip = B.battery_lp(hc, r["E0"], r["total_price"], method="ipm")
        assert ds.feasible and ip.feasible, (name, r["name"], r["t"])
        c_ds, c_ip = _cost(ds.q, ds.ch, ds.dis), _cost(ip.q, ip.ch, ip.dis)
        c_rec = _cost(ds.q, r["lp"]["p_batt_ch"], r["lp"]["p_batt_disch"])
        worst_self = max(worst_self, _rel(c_ip, c_ds))
        worst_rec = max(worst_rec, _rel(c_rec, c_ds))
        assert _rel(c_ip, c_ds) <= PIN_TOL, (name, r["name"], r["t"], c_ds, c_ip)
        assert _rel(c_rec, c_ds) <= PIN_TOL, (name, r["name"], r["t"], c_ds, c_rec)
        n += 1
    print(f"{name}: {n} battery records; simplex vs ipm {worst_self:.2e}, recorded vs simplex {worst_rec:.2e}")


def test_batches_are_the_issue_table():
    assert sorted(BC.BATCHES) == sorted([(1, 1, 0.92), (2, 1, 0.92), (31, 1, 0.92), (32, 4, 0.92), (32, 4, 1.0),
                                         (33, 1, 0.92), (48, 4, 0.92), (95, 5, 0.92), (95, 5, 1.0), (96, 4, 0.92)])


@pytest.mark.parametrize("batch", BC.BATCHES, ids=BC.batch_id)
def test_generator_conditions(batch):
    """Per batch: 76 homes, half of the cross battery_only and half pv_battery, every price and
    battery family and every E0 choice present; at least 60 % of the cases feasible and 10 %
    infeasible; no status within a quarter of a stage's reach of the limit (unless E0 sits exactly
    on Emin or Emax); dual simplex and interior point agree on every status and on every optimum to
    a tenth of the GPU test's bar.  Measured self-agreement, worst case of each batch, relative to
    max(1, |optimum|): H1 0, H2 2.2e-16, H31 1.7e-13, H32 5.4e-16 (discount 1: 3.7e-15), H33
    7.6e-16, H48 1.2e-15, H95 1.5e-15 (discount 1: 7.9e-12), H96 4.2e-13 -- the worst, 7.9e-12,
    leaves a factor of 126 under the GPU test's 1e-9, so that bar stands as the issue states it."""
    H, dt, disc = batch
    cs = BC.cases(batch)
    assert len(cs) == 76
    cross = [c for c in cs if c.price_family != BC.WIDE]
    assert len(cross) == 72 and sum(c.home["type"] == "pv_battery" for c in cross) == 36
    assert {c.price_family for c in cross} == set(BC.PRICE_FAMILIES)
    assert {c.battery_family for c in cross} == set(BC.BATTERY_FAMILIES)
    assert {c.e0_choice for c in cross} == set(BC.E0_CHOICES)
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        assert (c.hc.H, c.hc.dt, c.hc.discount, c.hc.S) == (H, dt, disc, 6)
        assert len(c.price) == H and len(c.ghi) == H + 1
        b = c.hc.batt
        a, g, r = b["eta_c"] / dt, (1.0 / b["eta_d"]) / dt, b["rate"]
        # distance of E0 from the limits of the set a trajectory exists from: [Emin - a r, Emax + g r]
        lo, hi = b["Emin"] - a * r, b["Emax"] + g * r
        on_box = c.E0 == b["Emin"] or c.E0 == b["Emax"]
        assert on_box or min(abs(c.E0 - lo), abs(c.E0 - hi)) >= 0.25 * a * r, (c.name, c.E0, lo, hi)
        if c.battery_family == "eta_one":
            assert b["eta_c"] == 1.0 and b["eta_d"] == 1.0
        if c.battery_family == "narrow":
            assert b["Emax"] - b["Emin"] < a * r
        if c.battery_family == "point_box":
            assert b["Emin"] == b["Emax"]
        if c.battery_family == "rate_zero":
            assert r == 0.0
        if c.battery_family == "at_emin":
            assert c.E0 == b["Emin"]
        if c.battery_family == "at_emax":
            assert c.E0 == b["Emax"]
    ds, ip = BC.reference(batch, "simplex"), BC.reference(batch, "ipm")
    worst = 0.0
    for c, x, y in zip(cs, ds, ip):
        b = c.hc.batt
        a, g, r = b["eta_c"] / dt, (1.0 / b["eta_d"]) / dt, b["rate"]
        assert x.feasible == y.feasible, c.name
        assert x.feasible == (b["Emin"] - a * r <= c.E0 <= b["Emax"] + g * r), c.name     # one stage decides
        if x.feasible:
            worst = max(worst, _rel(y.cost, x.cost))
            assert _rel(y.cost, x.cost) <= 0.1 * COST_TOL, (c.name, x.cost, y.cost)
    feasible = sum(x.feasible for x in ds)
    print(f"{BC.batch_id(batch)}: {feasible} feasible, {len(cs) - feasible} infeasible; simplex vs ipm {worst:.2e}")
    assert feasible >= 0.6 * len(cs) and len(cs) - feasible >= 0.1 * len(cs)


@pytest.mark.parametrize("batch", [b for b in BC.BATCHES if b[0] >= 31], ids=BC.batch_id)
def test_pv_inputs_cover_every_tie_and_sign(batch):
    """Every pair of a price sign (+, -, 0, -0.0) and ghi = 0 or > 0 occurs at a stage of a
    pv_battery home, in every batch with H >= 31."""
    seen = set()
    for c in BC.cases(batch):
        if c.home["type"] != "pv_battery":
            continue
        for p, g in zip(c.price, c.ghi[:c.hc.H]):
            sign = "+" if p > 0 else "-" if p < 0 else "-0" if math.copysign(1.0, p) < 0 else "0"
            seen.add((sign, bool(g > 0)))
    assert seen == {(s, g) for s in ("+", "-", "0", "-0") for g in (False, True)}


@pytest.mark.parametrize("batch", [b for b in BC.BATCHES if b[0] >= 32], ids=BC.batch_id)
def test_huge_battery_moves_at_more_than_32_stages(batch):
    """The 1e4 kWh battery's optimum under the alternating and the normal prices changes E at more
    than 32 distinct stages (at H = 32, where no more exist, at all 32): every stage adds psi's two
    segments to a list that is never cut back, so its value functions really carry segment lists
    past 64 entries (2H + 1 = 65 at H = 32)."""
    for c, x in zip(BC.cases(batch), BC.reference(batch)):
        if c.battery_family == "huge" and c.price_family in ("alternating", "normal"):
            assert x.feasible, c.name
            assert BC.moving_stages(c, x) >= min(c.hc.H, 33), (c.name, BC.moving_stages(c, x))


@pytest.mark.parametrize("batch", [b for b in BC.BATCHES if b[0] <= 33], ids=BC.batch_id)
def test_thermal_side_has_a_schedule(batch):
    """The exact thermal oracle finds a schedule for every case of the batches with H <= 33, so
    none of them can leave the GPU test as ROUND_FAIL."""
    for c in BC.cases(batch):
        assert TH.thermal_optimum(c.hc, c.step_input()) is not None, c.name
