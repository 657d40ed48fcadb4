"""The kernel's battery LP (`storage_lp` through its battery view) and PV rule (`pv_curt`) against an
independent LP.  `storage_lp` is the one recursion under the battery and the vehicle (test_gpu_ev.py).

The default path (int_mode round) solves every battery home's storage problem with a one-wave
piecewise-linear value-function DP whose segment lists alias the thermal DP's dead LDS buffers.
The cases of tests/battery_cases.py drive it where the generator's batteries never do: lists that
grow to 2H + 1 entries (more than one entry per lane from H = 32), the tightest aliasing (the
compact layout's last horizon, H = 95, and the first of the other, H = 96), tied slopes (eta = 1,
discount 1 with a constant price), zero and -0.0 prices, a box of one point, a rate of zero, E0 on
and outside the box, and batteries with no trajectory at all.  The reference is oracle/battery.py
(HiGHS at 1e-10), pinned and measured by tests/test_oracle_battery.py: its two methods agree to
7.9e-12 at worst on these cases, a factor of 126 under the cost bar below, so the bar is the
1e-9 * max(1, |ref|) of test_gpu_parity.py::test_battery_lp_exact, unchanged.

Measured on the MI355X, worst |kernel - reference| / max(1, |reference|) of the battery cost per
batch: H1 8.2e-11, H2 4.0e-11, H31 3.4e-12, H32 6.4e-12 (discount 1: 4.5e-12), H33 1.7e-12, H48
7.6e-13, H95 9.1e-12 (discount 1: 7.5e-12), H96 6.2e-13; no case left out as ROUND_FAIL.  The two
largest are absolute errors against an optimum of 0 under the +-1e3 / +-1e-12 prices: at H = 1 the
kernel's own rounding (one ulp of E = 472 kWh charged at q = 6e3), at H = 2 the reference's (HiGHS
takes the cost 6e-12 for zero within its dual tolerance and charges at it).
"""
import os

import numpy as np
import pytest

from tests import battery_cases as BC

pytestmark = pytest.mark.gpu

COST_TOL = 1e-9
EPS = 2.0 ** -52
BATT_KEYS = ("p_batt_ch", "p_batt_disch", "e_batt_opt")
_SOLVED = {}


def _solve(batch):
    import torch
    from dragg_amd import _lib as L
    from dragg_amd.mpc import MPCBatch
    cs = BC.cases(batch)
    b = MPCBatch([c.home for c in cs], int_mode="round")
    b.solve_explicit(**BC.explicit_inputs(cs))
    torch.cuda.synchronize()
    ip = b.int_path.cpu().numpy()
    return dict(status=b.status.cpu().numpy(), fc=b.fc.cpu().numpy(), vals=b.vals.cpu().numpy(),
                obj=b.obj.cpu().numpy(), raw_path=ip, path=ip & L.PATH_APPROX_MASK, S=b.S)


def _solved(batch):
    """The batch's unforced solve (one per process)."""
    if batch not in _SOLVED:
        _SOLVED[batch] = _solve(batch)
    return _SOLVED[batch]


def _battery_fields(res):
    """The battery's forecast fields [3][H][N] and vals entries [3][N]."""
    from dragg_amd import _lib as L
    return (np.stack([res["fc"][L.FC_KEYS.index(k)] for k in BATT_KEYS]),
            np.stack([res["vals"][L.K[k]] for k in BATT_KEYS]))


def check_battery(batch, res, names=None):
    """Status, cost, feasibility and entry 0 of every case of `res` against oracle/battery.py.
    -> (cases compared, cases left out as ROUND_FAIL, worst cost gap)."""
    from dragg_amd import _lib as L
    from oracle import battery as B
    H, dt, _ = batch
    all_cs, ref = BC.cases(batch), BC.reference(batch)
    (ch_a, dis_a, e_a), v0 = _battery_fields(res)
    n = n_fail = 0
    worst = 0.0
    for i, (c, rf) in enumerate(zip(all_cs, ref)):
        if names is not None and c.name not in names:
            continue
        st = res["status"][i]
        if st == L.ST_ROUND_FAIL:           # the thermal side found no schedule: the battery never ran
            n_fail += 1
            continue
        assert st == (L.ST_OPTIMAL if rf.feasible else L.ST_INFEASIBLE), (c.name, L.STATUS_NAMES[st], rf.feasible)
        if not rf.feasible:
            continue
        b = c.hc.batt
        ch, dis, E = ch_a[:, i], dis_a[:, i], e_a[:, i]
        ours = float(rf.q @ (ch + dis))
        gap = abs(ours - rf.cost) / max(1.0, abs(rf.cost))
        worst = max(worst, gap)
        assert gap <= COST_TOL, (c.name, ours, rf.cost, gap)
        # H accumulated roundings of the recursion at the magnitude of the state, with a factor of 8
        ftol = 8 * H * EPS * max(1.0, b["Emax"], b["rate"])
        assert ch.min() >= -ftol and ch.max() <= b["rate"] + ftol, (c.name, ch.min(), ch.max())
        assert dis.max() <= ftol and dis.min() >= -b["rate"] - ftol, (c.name, dis.min(), dis.max())
        assert E.min() >= b["Emin"] - ftol and E.max() <= b["Emax"] + ftol, (c.name, E.min(), E.max(), b)
        rec = B.soc_step(c.hc, np.r_[c.E0, E[:-1]], ch, dis)
        assert np.abs(rec - E).max() <= ftol, (c.name, np.abs(rec - E).max())
        for j in range(3):
            assert v0[j, i] == (ch, dis, E)[j][0], (c.name, BATT_KEYS[j])
        n += 1
    return n, n_fail, worst


def check_pv(batch, res):
    """p_pv: 0 where the price is negative and the sun is up, the whole array output where the
    price is positive (to 4 ulp); price 0, -0.0 or ghi = 0 is a tie and is not compared."""
    from dragg_amd import _lib as L
    H = batch[0]
    pv = res["fc"][L.FC_KEYS.index("p_pv_opt")]
    n_curt = n_full = 0
    for i, c in enumerate(BC.cases(batch)):
        if c.home["type"] != "pv_battery" or res["status"][i] != L.ST_OPTIMAL:
            continue
        full = c.hc.pv["area"] * c.hc.pv["eff"] * c.ghi[:H] / 1000        # mpc_calc.py:380-385
        for k in range(H):
            if c.price[k] < 0 and c.ghi[k] > 0:
                assert pv[k, i] == 0.0, (c.name, k, pv[k, i])
                n_curt += 1
            elif c.price[k] > 0:
                assert abs(pv[k, i] - full[k]) <= 4 * np.spacing(full[k]), (c.name, k, pv[k, i], full[k])
                n_full += 1
    return n_curt, n_full


def check_objective(batch, res):
    """The whole objective of the uniform-sign price families against oracle.thermal.exact_milp."""
    from dragg_amd import _lib as L
    from oracle import thermal as TH
    n = 0
    for i, c in enumerate(BC.cases(batch)):
        if c.price_family not in BC.UNIFORM_SIGN or res["status"][i] != L.ST_OPTIMAL:
            continue
        opt = TH.exact_milp(c.hc, c.step_input())
        assert opt is not None, c.name
        assert abs(res["obj"][i] - opt) <= 1e-6 * max(1.0, abs(opt)), (c.name, res["obj"][i], opt)
        n += 1
    return n


@pytest.mark.parametrize("batch", BC.BATCHES, ids=BC.batch_id)
def test_battery_and_pv_against_independent_lp(batch, gpu):
    """One solve_explicit of the batch's 76 homes.  Per case: ST_OPTIMAL iff the battery LP is
    feasible, else ST_INFEASIBLE (ROUND_FAIL, the thermal side without a schedule, is the only way
    out: at most 5 % of a batch, none at H <= 33); the cost of the p_batt_ch / p_batt_disch fields
    within 1e-9 * max(1, |ref|) of the LP optimum; the trajectory inside its bounds and on the
    reference's SoC recursion within 8 H eps max(1, Emax, r); the vals entries equal to entry 0 of
    their fields.  Per batch: the PV fields, and at H <= 33 the whole objective of the uniform-sign
    families against the exact MILP optimum (1e-6 relative)."""
    H = batch[0]
    res = _solved(batch)
    cs = BC.cases(batch)
    n, n_fail, worst = check_battery(batch, res)
    assert n_fail <= (0 if H <= 33 else 0.05 * len(cs)), (n_fail, len(cs))
    n_curt, n_full = check_pv(batch, res)
    assert n_full > 0 and (H < 31 or n_curt > 0)
    n_obj = check_objective(batch, res) if H <= 33 else 0
    if H >= 32:
        # asserted on the reference's trajectory, not on the kernel's word: these lists pass 64 entries
        for c, rf in zip(cs, BC.reference(batch)):
            if c.battery_family == "huge" and c.price_family in ("alternating", "normal"):
                assert rf.feasible and BC.moving_stages(c, rf) >= min(H, 33), c.name
    print(f"{BC.batch_id(batch)}: {n} feasible cases at the LP optimum, worst cost gap {worst:.2e}; {n_fail} ROUND_FAIL; "
          f"p_pv checked at {n_curt} curtailed and {n_full} full stages; {n_obj} whole objectives exact")


@pytest.mark.parametrize("batch", [b for b in BC.BATCHES if b[0] == 32], ids=BC.batch_id)
def test_battery_after_second_launch(batch, gpu):
    """The wide-band family (a 12-32 C comfort band under a stage-varying price) is solved by the
    second launch; the battery that runs after it there meets the same bars."""
    from dragg_amd import _lib as L
    res = _solved(batch)
    wide = {c.name for c in BC.cases(batch) if c.price_family == BC.WIDE}
    assert len(wide) == 4
    for i, c in enumerate(BC.cases(batch)):
        if c.name in wide:
            assert res["status"][i] == L.ST_OPTIMAL and res["raw_path"][i] & L.PATH_SECOND, (c.name, res["raw_path"][i])
    n, n_fail, _ = check_battery(batch, res, wide)
    assert (n, n_fail) == (4, 0)


def _identical(batch, res, other, what):
    from dragg_amd import _lib as L
    (f0, v0), (f1, v1) = _battery_fields(res), _battery_fields(other)
    assert np.array_equal(res["status"], other["status"]), what
    assert np.array_equal(f0, f1, equal_nan=True) and np.array_equal(v0, v1, equal_nan=True), what
    pv = [np.stack([r["fc"][L.FC_KEYS.index(k)] for k in ("p_pv_opt", "u_pv_curt_opt")]) for r in (res, other)]
    assert np.array_equal(pv[0], pv[1], equal_nan=True), what


@pytest.mark.parametrize("batch", [b for b in BC.BATCHES if b[0] == 32], ids=BC.batch_id)
def test_battery_after_forced_step_function_dp(batch, gpu):
    """DRAGG_FORCE_STEP_DP=1 sends every home to the step-function DP launch (DM_NARROW, a multi-wave
    block): every solved case carries PATH_STEPS, and the battery and PV fields are bit-identical
    to the unforced run's -- the inputs are the same and the same one-wave routine runs."""
    from dragg_amd import _lib as L
    res = _solved(batch)
    os.environ["DRAGG_FORCE_STEP_DP"] = "1"
    L.reload_knobs()                     # (the library reads its knobs at load, never per step)
    try:
        forced = _solve(batch)
    finally:
        os.environ.pop("DRAGG_FORCE_STEP_DP", None)
        L.reload_knobs()
    for i, c in enumerate(BC.cases(batch)):
        if forced["status"][i] == L.ST_OPTIMAL:      # (an infeasible battery is decided before any DP)
            assert forced["raw_path"][i] & L.PATH_STEPS, (c.name, forced["raw_path"][i])
    assert (forced["status"] == L.ST_OPTIMAL).sum() >= 0.6 * len(forced["status"])
    _identical(batch, res, forced, "forced step-function DP")
    n, n_fail, _ = check_battery(batch, forced)
    assert n_fail == 0


@pytest.mark.parametrize("batch", [b for b in BC.BATCHES if b[0] == 95], ids=BC.batch_id)
def test_battery_waves_per_home_bit_identical(batch, gpu):
    """The H = 95 batches (the compact layout's tightest aliasing) under the waves-per-home settings
    of test_gpu_step.py::test_waves_per_home_bit_identical: 2 and 4 waves per home, and one wave
    with one 64-child chunk per pass, give the same battery and PV fields bit for bit."""
    from dragg_amd import _lib as L
    out = {}
    try:
        for nw in ("1", "2", "4", "1/ilp1"):
            os.environ["DRAGG_WAVES_PER_HOME"] = nw[0]
            if nw.endswith("ilp1"):
                os.environ["DRAGG_HOT_ILP"] = "1"
            L.reload_knobs()
            out[nw] = _solve(batch)
    finally:
        os.environ.pop("DRAGG_WAVES_PER_HOME", None)
        os.environ.pop("DRAGG_HOT_ILP", None)
        L.reload_knobs()
    _identical(batch, _solved(batch), out["1"], "1 wave per home")
    for nw in ("2", "4", "1/ilp1"):
        _identical(batch, out["1"], out[nw], nw)
        check_battery(batch, out[nw])
