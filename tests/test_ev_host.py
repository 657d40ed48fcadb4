"""The EV model on the CPU: the independent LP of tests/ev_cases.py pinned, the generator's conditions, a float64
restatement of the kernel's recursion against the LP, and the host side (packing, schedule, shards, limits)."""
import copy

import numpy as np
import pytest

from tests import battery_cases as BC
from tests import ev_cases as EC

COST_TOL = 1e-9


@pytest.mark.parametrize("batch", BC.BATCHES, ids=BC.batch_id)
def test_degenerate_vehicle_lp_is_the_battery_lp(batch):
    """rc = rd = r, no drain, the constant box: the stage-varying LP is oracle.battery.battery_lp on every case of
    tests/battery_cases.py -- the same status, the same optimum (1e-9 * max(1, |ref|), the bar of every cost here)."""
    from oracle import battery as B
    H, dt, _ = batch
    n = 0
    for c, rf in zip(BC.cases(batch), BC.reference(batch)):
        b = c.hc.batt
        a, bb = b["eta_c"] / dt, (1.0 / b["eta_d"]) / dt
        full = np.full(H, b["rate"])
        s = EC.storage_lp(B.weights(c.hc, c.price), a, bb, full, full, np.zeros(H), np.full(H, b["Emin"]),
                          np.full(H, b["Emax"]), c.E0)
        assert s.feasible == rf.feasible, c.name
        if rf.feasible:
            assert abs(s.cost - rf.cost) <= COST_TOL * max(1.0, abs(rf.cost)), (c.name, s.cost, rf.cost)
            n += 1
    assert n >= 30


@pytest.mark.parametrize("H", EC.HORIZONS, ids=EC.batch_id)
def test_cases_and_reference(H):
    """The generator's conditions (the status margins are asserted by `cases` itself): every family present, at
    least half of the batch feasible and at least eight cases infeasible; the reference's two HiGHS methods agree
    on status and, within the cost bar, on the optimum; the float64 restatement of the kernel's recursion stays
    within the bar on every case (so no family is dropped)."""
    cs = EC.cases(H)
    assert len(cs) == len(EC.PRICE_FAMILIES) * len(EC.VEHICLE_FAMILIES)
    assert {c.vehicle_family for c in cs if c.feasible is None} == set(EC.UNASSERTED)
    assert sum(1 for c in cs if c.feasible) >= len(cs) // 2
    assert sum(1 for c in cs if c.feasible is False) >= 8
    worst_m = worst_r = 0.0
    for c, r1, r2 in zip(cs, EC.reference(H), EC.reference(H, "ipm")):
        rec = EC.recursion(c.q, c.a, c.b, c.rc, c.rd, c.drain, c.lo, c.hi, c.E0)
        if c.feasible is not None:
            assert r1.feasible == r2.feasible == rec.feasible == c.feasible, c.name
        if r1.feasible and r2.feasible:
            worst_m = max(worst_m, abs(r1.cost - r2.cost) / max(1.0, abs(r1.cost)))
        if r1.feasible and rec.feasible:
            worst_r = max(worst_r, abs(rec.cost - r1.cost) / max(1.0, abs(r1.cost)))
            assert np.abs(np.r_[c.E0, rec.E[:-1]] + c.a * rec.ch + c.b * rec.dis - c.drain - rec.E).max() <= 1e-9
    print(f"{EC.batch_id(H)}: methods agree to {worst_m:.2e}, the recursion to {worst_r:.2e}")
    assert worst_m <= COST_TOL and worst_r <= COST_TOL
    if H >= 48:
        # feasible cases whose list passes 64 entries at a cut: the clip scan's more-than-one-entry-per-lane path
        long = [c.name for c, r in zip(cs, EC.reference(H)) if r.feasible and EC.list_length(c) > 64]
        assert len(long) >= 2, long
    if H == 96:
        two = [c for c in cs if c.vehicle_family == "two_departures"]
        assert all((c.lo > c.lo.min()).sum() == 1 and c.rc[0] == 0.0 and c.lo[-1] > c.lo.min() for c in two)
    if H >= 31:
        assert any((np.diff(np.r_[c.c0 + np.arange(H)] % EC.D) < 0).any() for c in cs if c.vehicle_family == "wrap_midnight")


def test_pack_and_schedule_against_the_restatement():
    """pack_evs' rows and ev_schedule's stage arrays equal the restatement of tests/ev_cases.py (stage_arrays) for
    every packable case, at several clocks."""
    from dragg_amd import _lib as L
    from dragg_amd.ev import ev_schedule, pack_evs
    H = 33
    cs = [c for c in EC.cases(H) if c.vehicle_family not in ("always_home", "huge")]      # (never packed)
    homes = EC.fleet_homes(cs, H)
    P, owners = pack_evs(homes)
    assert P.shape == (L.NEVP, len(cs)) and owners.tolist() == list(range(len(cs)))
    for j, c in enumerate(cs):
        e = c.ev
        want = [e["capacity"], e["capacity_lower"] * e["capacity"], e["capacity_upper"] * e["capacity"], e["max_rate"],
                e["ch_eff"], e["disch_eff"], e["e_ev_init"] * e["capacity"], float(e["v2g"]), e["depart_step"],
                e["return_step"], e["trip_kwh"], e["depart_soc"] * e["capacity"]]
        assert P[:, j].tolist() == want, c.name
    for day_offset, t in ((0, 0), (5, 3), (90, 7), (95, 100)):
        s = ev_schedule(P, EC.DT, day_offset, t, H)
        for j, c in enumerate(cs):
            rc, rd, drain, lo, hi = EC.stage_arrays(c.ev, EC.DT, (day_offset + t) % EC.D, H)
            for k, w in (("rate_ch", rc), ("rate_dis", rd), ("drain", drain), ("lo", lo), ("hi", hi)):
                assert np.array_equal(s[k][:, j], w), (c.name, k, day_offset, t)
    bad = copy.deepcopy(homes[0])
    bad["ev"]["return_step"] = bad["ev"]["depart_step"]
    with pytest.raises(ValueError, match="depart_step"):
        pack_evs([bad])
    del bad["ev"]["trip_kwh"]
    with pytest.raises(ValueError, match="trip_kwh"):
        pack_evs([bad])


def test_synthetic_homes_unchanged_without_vehicles():
    from dragg_amd.community import synthetic_homes
    a = synthetic_homes(40, seed=5)
    assert synthetic_homes(40, seed=5, ev_share=0.0) == a and not any("ev" in h for h in a)
    b = synthetic_homes(40, seed=5, ev_share=0.25)
    with_ev = [i for i, h in enumerate(b) if "ev" in h]
    assert len(with_ev) == 10 and with_ev == [4 * j for j in range(10)]
    assert [{k: v for k, v in h.items() if k != "ev"} for h in b] == a
    assert b == synthetic_homes(40, seed=5, ev_share=0.25)
    for i in with_ev:
        e = b[i]["ev"]
        assert set(e) == set(EC.EV_FIELDS) and 0 <= e["depart_step"] < e["return_step"] <= 96


def test_fleet_shards_are_strided():
    """A vehicle lives on its home's rank (the homes' shard_index): the shards' vehicles partition the fleet."""
    from dragg_amd.aggregator import shard_index
    from dragg_amd.community import synthetic_homes
    from dragg_amd.ev import pack_evs, shard_evs
    homes = synthetic_homes(23, seed=3, ev_share=0.6)
    P, owners = pack_evs(homes)
    seen = {}
    for rank in range(4):
        Pr, own, mine = shard_evs(homes, rank, 4)
        assert [h["name"] for h in mine] == [homes[i]["name"] for i in shard_index(len(homes), rank, 4)]
        assert all(i % 4 == rank for i in own)
        for j, i in enumerate(own):
            seen[int(i)] = Pr[:, j]
    assert sorted(seen) == owners.tolist()
    assert all(np.array_equal(seen[int(i)], P[:, j]) for j, i in enumerate(owners))
    assert shard_evs(homes[:2], 3, 4)[0].shape[1] == 0


def test_paths_without_vehicles_yet_say_so():
    """sweep, commit and the vector environments name the limit when a fleet is attached."""
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.vector import VectorAggregator
    a = DeviceAggregator.__new__(DeviceAggregator)
    a.ev = object()
    with pytest.raises(NotImplementedError, match="EV fleet"):
        a.sweep([[0.0]], 1)
    with pytest.raises(NotImplementedError, match="EV fleet"):
        a.commit(0)
    with pytest.raises(NotImplementedError, match="EV fleet"):
        VectorAggregator([], [0.0], [0.0], [0.0], 1, [0], [0], 1, ev=object())
    # a config with a [home.ev] section: rl_vector says so rather than leaving the vehicles out
    from dragg_amd.runner import Aggregator
    r = Aggregator.__new__(Aggregator)
    r.world, r.config = 1, {"home": {"ev": {"share": 0.5}}}
    with pytest.raises(NotImplementedError, match="EV fleet"):
        r.rl_vector(2)


def test_ev_share_outside_0_1_is_refused():
    from dragg_amd.community import ev_sections, synthetic_homes
    assert len(ev_sections(10, 1.0, 4, 3)) == 10
    for share in (1.5, -0.1):
        with pytest.raises(ValueError, match="share"):
            ev_sections(10, share, 4, 3)
    with pytest.raises(ValueError, match="share"):
        synthetic_homes(8, ev_share=2.0)
