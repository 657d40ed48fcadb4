"""EV fleets in the vector environments, host side (CPU): the ABI surface of dragg_mpc_ev_step_episodes /
dragg_mpc_ev_aggregate_onto / dragg_mpc_ev_adopt / dragg_mpc_ev_reset, the day-clock rule, and
`VectorAggregator(vehicles=True)` on a stand-in batch (tests/test_classes_host.py's) and a stand-in fleet whose step
depends on everything a group owns: start index, clock, day clock, price row, class and previous state.  Every
value of the stand-ins is a small dyadic rational, so sums are exact in any order."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from dragg_amd.ev import ev_episode_day_step
from tests.test_classes_host import CFG, CPU, ENV, ClassBatch
from tests.test_classes_host import HOMES as PLAIN_HOMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")
NEW = ["dragg_mpc_ev_step_episodes", "dragg_mpc_ev_aggregate_onto", "dragg_mpc_ev_adopt", "dragg_mpc_ev_reset"]

OWNERS = [1, 2, 4]                      # the homes with a vehicle
RATES = {1: 7.0, 2: 11.0, 4: 3.5}
HOMES = [dict(h, ev={"max_rate": RATES[i]}) if i in RATES else dict(h) for i, h in enumerate(PLAIN_HOMES)]
CLASSES = [0, 1, 0, 1, 1, 0]            # by home: the vehicles' classes are [1, 0, 1]
DAY0 = 5                                # the step of day of environment index 0
DT = 1                                  # the stand-in's day has 24 steps
SEEDS = [1000, 2000, 3000]              # (0.001 * seed is exact)


def _home_step(prev, seed, start, clock, price, i):
    """ClassBatch's closed loop for one home."""
    prev = 0.0 if clock == 0 else prev
    return prev + (i + 1) * (1 + price) * (clock + 1) + 0.001 * seed + start


def _car_step(prev, start, clock, price, v):
    """The stand-in fleet's closed loop for one vehicle: the new state from everything its group owns."""
    prev = 0.0 if clock == 0 else prev
    day = ev_episode_day_step(DAY0, 0, start, clock, DT)
    return prev + 0.5 * (v + 1) * (1 + price) * (clock + 1) + 0.25 * start + 0.125 * day


def _car_rows(x, price):
    """vals' five rows of a vehicle in state x: ch, dis, E, cost, forecast."""
    return [x, -0.25 * x, x, x * price, 3.0 * x]


class StandInFleet:
    """Stand-in for EVFleet with the surface VectorAggregator uses."""
    H = 4

    def __init__(self, homes, tou, start_index=0, groups=1, day_offset=0, device=None, **kw):
        self.owners = np.asarray([i for i, h in enumerate(homes) if h.get("ev") is not None], dtype=np.int64)
        self.groups, self.Mb = int(groups), len(self.owners)
        self.M = self.groups * self.Mb
        self.tou, self.start_index, self.day_offset = tou, int(start_index), int(day_offset)
        assert self.start_index == 0 and self.day_offset == DAY0
        nan = float("nan")
        self.vals = torch.full((L.NEVV, self.M), nan, dtype=torch.float64)
        self.fc_store = torch.full((self.M, L.NEVK, self.H), nan, dtype=torch.float64)
        self.status = torch.zeros(self.M, dtype=torch.int32)
        self.obj = torch.full((self.M,), nan, dtype=torch.float64)
        self.sums = torch.zeros((self.groups, 3), dtype=torch.float64)
        self.n_classes, self.cls = 1, [0] * self.Mb
        self.rp = torch.zeros((self.groups, 1, 1), dtype=torch.float64)
        self.calls = []

    def set_price_classes(self, classes, n_classes=None):
        cm, self.n_classes = L.price_class_map(classes, self.Mb, n_classes)
        self.cls = cm.tolist()
        self.rp = torch.zeros((self.groups, self.n_classes, 1), dtype=torch.float64)

    def set_reward_price(self, rp):
        self.rp = rp.clone().reshape(self.groups, self.n_classes, -1)

    def step_episodes(self, starts, clocks, stream=None):
        assert starts.dtype == torch.int32 and clocks.dtype == torch.int32
        assert tuple(starts.shape) == tuple(clocks.shape) == (self.groups,)
        self.calls.append(clocks.tolist())
        for g in range(self.groups):
            c = int(clocks[g])
            if c < 0:                               # idle: nothing of the group is written
                continue
            for v in range(self.Mb):
                r = g * self.Mb + v
                p = float(self.rp[g, self.cls[v], 0])
                x = _car_step(float(self.vals[L.EVK["e_ev_opt"], r]), int(starts[g]), c, p, v)
                self.vals[:, r] = torch.tensor(_car_rows(x, p), dtype=torch.float64)
                self.fc_store[r] = x
                self.status[r] = (v + c) % 2
                self.obj[r] = -x

    def aggregate_onto(self, base, out=None, stream=None):
        out = base if out is None else out
        v = self.vals.view(L.NEVV, self.groups, self.Mb)
        s = torch.stack([(v[0] + v[1]).sum(1), v[L.EVK["forecast_p_ev"]].sum(1), v[L.EVK["cost_ev"]].sum(1)], dim=1)
        self.sums.copy_(s)
        out.copy_(base.reshape(self.groups, 3) + s)
        return out

    def reset_groups(self, mask, stream=None):
        assert mask.dtype == torch.bool and tuple(mask.shape) == (self.groups,)
        m = mask.repeat_interleave(self.Mb)
        self.vals[:, m] = float("nan")
        self.fc_store[m] = float("nan")
        self.obj[m] = float("nan")
        self.status[m] = 0

    def replicate_from(self, base):
        C = self.M // base.M
        assert C * base.M == self.M
        self.vals.copy_(base.vals.repeat(1, C))
        self.fc_store.copy_(base.fc_store.repeat(C, 1, 1))
        self.status.copy_(base.status.repeat(C))
        self.obj.copy_(base.obj.repeat(C))

    def adopt_from(self, src, choice, stream=None):
        assert choice.dtype == torch.int32 and tuple(choice.shape) == (self.groups,)
        C, Mb = src.M // self.M, self.Mb
        for e, c in enumerate(choice.tolist()):
            if not 0 <= c < C:
                continue
            d, s = slice(e * Mb, (e + 1) * Mb), slice(c * self.M + e * Mb, c * self.M + (e + 1) * Mb)
            self.vals[:, d] = src.vals[:, s]
            for k in ("fc_store", "status", "obj"):
                getattr(self, k)[d] = getattr(src, k)[s]


def _va(E=3, T=5, starts=(0, 7, 12), classes=True, vehicles=True, homes=HOMES, **kw):
    from dragg_amd.vector import VectorAggregator
    cls = dict(price_classes=CLASSES, n_classes=2) if classes else {}
    ev = dict(vehicles=True, day_offset=DAY0, fleet_cls=StandInFleet) if vehicles else {}
    return VectorAggregator(homes, ENV, ENV, ENV, E, SEEDS[:E], list(starts)[:E], T, device=CPU, batch_cls=ClassBatch,
                            **cls, **ev, **kw)


class Episode:
    """One episode as a single run of the stand-in homes plus the stand-in fleet: the reference."""

    def __init__(self, seed, start):
        self.seed, self.start, self.t = seed, start, 0
        self.homes, self.cars = [0.0] * len(HOMES), [0.0] * len(OWNERS)
        self.rows, self.ev_rows = [], []

    def step(self, prices):
        """`prices`: the class prices [2] of this step -> the filed sums (homes plus vehicles)."""
        hp = [prices[CLASSES[i]] for i in range(len(HOMES))]
        cp = [prices[CLASSES[o]] for o in OWNERS]
        self.homes = [_home_step(self.homes[i], self.seed, self.start, self.t, hp[i], i) for i in range(len(HOMES))]
        self.cars = [_car_step(self.cars[v], self.start, self.t, cp[v], v) for v in range(len(OWNERS))]
        h = [sum(self.homes), sum(2 * x for x in self.homes), sum(x * p for x, p in zip(self.homes, hp))]
        rows = [_car_rows(x, p) for x, p in zip(self.cars, cp)]
        e = [sum(r[0] + r[1] for r in rows), sum(r[4] for r in rows), sum(r[3] for r in rows)]
        self.t += 1
        self.rows.append([a + b for a, b in zip(h, e)])
        self.ev_rows.append(e)
        return self.rows[-1]


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def _fleet_equal(a, b, groups=None):
    """The two fleets' state, bit for bit (of the groups given: all)."""
    for k in ("vals", "fc_store", "status", "obj"):
        x, y = getattr(a, k), getattr(b, k)
        if k == "vals":
            x, y = x.t(), y.t()
        if groups is not None:
            rows = torch.cat([torch.arange(g * a.Mb, (g + 1) * a.Mb) for g in groups])
            x, y = x[rows], y[rows]
        if not torch.equal(_bits(x), _bits(y)):
            return False
    return True


# ------------------------------------------------------------------ ABI surface
def test_abi_surface_of_the_fleet_entries():
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    assert all(n in names and n in L.EXPORTS for n in NEW)
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and L.ABI_VERSION == 10
    assert set(names) == set(L.EXPORTS)


def test_argument_errors_that_need_no_device():
    """On a built library: the checks made before anything touches the device."""
    from dragg_amd import build
    build.build()
    lib = L.load()
    assert all(hasattr(lib, n) for n in NEW) and lib.dragg_mpc_abi_version() == 10
    E_ARG = -1
    dims = L.Dims(n_homes=6, horizon=4, sub_steps=6, dt=4, n_draw_hours=1, n_env=64, n_rp=1, int_mode=L.INT_ROUND,
                  max_iter=0, check_every=0, discount=0.9, flags=0, n_groups=3)
    one = ctypes.c_void_p(8)            # (non-NULL; never dereferenced by the checks)
    ev = L.Ev(params=one, vals=one, fc=one, status=one, obj=one, day_offset=0, n_vehicles=6)
    prob = L.Problem(tou=one, reward_price=one, start_index=0)
    ep, none = L.Episodes(), None
    step = lib.dragg_mpc_ev_step_episodes
    assert step(dims, prob, none, none, ev, 0, none) == E_ARG                       # ep NULL
    assert step(dims, none, ep, none, ev, 0, none) == E_ARG
    for P in (0, -1, L.CLASS_MAX + 1):
        assert step(dims, prob, ep, L.Classes(n_classes=P, price_class=one), ev, 0, none) == E_ARG
    assert step(dims, prob, ep, L.Classes(n_classes=2, price_class=None), ev, 0, none) == E_ARG
    bad = L.Ev(params=one, vals=one, fc=one, status=one, obj=one, day_offset=0, n_vehicles=7)
    assert step(dims, prob, ep, none, bad, 0, none) == E_ARG                        # M % G
    assert step(dims, prob, ep, none, ev, -1, none) == E_ARG                        # the shared timestep
    assert step(dims, prob, ep, none, ev, 60, none) == E_ARG                        # the shared window
    off = L.Ev(params=one, vals=one, fc=one, status=one, obj=one, day_offset=96, n_vehicles=6)
    assert step(dims, prob, ep, none, off, 0, none) == E_ARG                        # day_offset >= 24 dt
    empty = L.Ev(day_offset=0, n_vehicles=0)
    assert step(dims, prob, ep, none, empty, 0, none) == 0                          # M == 0: a no-op
    assert lib.dragg_mpc_ev_aggregate_onto(dims, ev, none, one, none, none) == E_ARG
    assert lib.dragg_mpc_ev_aggregate_onto(dims, bad, one, one, none, none) == E_ARG
    assert lib.dragg_mpc_ev_reset(dims, ev, none, none) == E_ARG
    assert lib.dragg_mpc_ev_reset(dims, bad, one, none) == E_ARG
    assert lib.dragg_mpc_ev_reset(dims, empty, one, none) == 0
    assert lib.dragg_mpc_ev_adopt(dims, 2, none, ev, ev, none) == E_ARG             # choice NULL
    assert lib.dragg_mpc_ev_adopt(dims, 0, one, ev, ev, none) == E_ARG              # copies < 1
    assert lib.dragg_mpc_ev_adopt(dims, 2, one, ev, ev, none) == E_ARG              # the source is not 2 copies
    src = L.Ev(params=one, vals=ctypes.c_void_p(12), fc=one, status=one, obj=one, day_offset=0, n_vehicles=12)
    assert lib.dragg_mpc_ev_adopt(dims, 2, one, src, ev, none) == E_ARG             # a misaligned double array


# ------------------------------------------------------------------ the day clock
def test_episode_day_step_is_the_non_negative_remainder():
    for dt in (1, 4, 6):
        D = 24 * dt
        for day_offset in (0, 5, D - 1):
            for start0 in (0, 40, 3 * D + 7):
                for start in (0, 7, start0 - D - 3, start0 - 1, start0, start0 + 1, start0 + 5 * D + 2, 8759 * dt):
                    for t in (0, 1, D - 1, D, 3 * D):
                        want = (day_offset + start - start0 + t) % D
                        got = ev_episode_day_step(day_offset, start0, start, t, dt)
                        assert isinstance(got, int) and got == want and 0 <= got < D
    got = ev_episode_day_step(5, 40, np.array([0, 40, 500]), np.array([3, 0, 288]), 4)
    assert got.tolist() == [(5 - 40 + 3) % 96, 5, (5 + 460 + 288) % 96]


# ------------------------------------------------------------------ VectorAggregator with vehicles
def test_the_doors():
    from dragg_amd.vector import VectorAggregator
    with pytest.raises(ValueError, match="ev"):
        _va(homes=PLAIN_HOMES)                                  # vehicles=True without any "ev" section
    with pytest.raises(NotImplementedError, match="EV fleet"):
        VectorAggregator(HOMES, ENV, ENV, ENV, 1, [0], [0], 1, device=CPU, batch_cls=ClassBatch, ev=object())
    with pytest.raises(NotImplementedError, match="EV fleet"):
        VectorAggregator(HOMES, ENV, ENV, ENV, 1, [0], [0], 1, device=CPU, batch_cls=ClassBatch, ev=object(),
                         vehicles=True, fleet_cls=StandInFleet)
    va = _va(vehicles=False)
    assert va.fleet is None and va.ev_sums is None and va.ev_agg_hist is None and va.vehicle_max_rate == 0.0
    va = _va()
    assert va.fleet.owners.tolist() == OWNERS and va.fleet.cls == [1, 0, 1] and va.fleet.groups == 3
    assert va.vehicle_max_rate == sum(RATES.values())
    assert tuple(va.ev_agg_hist.shape) == (5, 3, 3) and _va(keep_history=False).ev_agg_hist is None


def test_episodes_equal_single_runs_of_homes_plus_vehicles():
    """E = 3, T = 5: a parked episode, staggered resets and a finished one; every filed row is the single run's."""
    starts = [0, 7, 12]
    va, plain = _va(), _va(vehicles=False)
    eps = [Episode(SEEDS[e], starts[e]) for e in range(3)]
    P = [[[0.0, 0.5], [0.5, -0.25], [-0.25, 0.25]], [[0.25, 0.0], [0.5, 0.5], [0.0, -0.5]],
         [[0.5, 0.25], [0.25, 0.75], [0.0, 0.0]], [[-0.5, 0.5], [0.5, 0.25], [0.25, 0.25]],
         [[0.0, 0.0], [0.75, 0.5], [0.5, -0.25]], [[0.25, 0.5], [0.0, 0.25], [0.5, 0.5]],
         [[0.5, 0.5], [0.5, 0.0], [0.25, 0.0]]]
    out = va.step(P[0])
    plain.step(P[0])
    for e in range(3):
        assert out[e].tolist() == eps[e].step(P[0][e])
    # park episode 1: its fleet columns keep every byte, the others go on
    va.park([1])
    plain.park([1])
    keep = [x.clone() for x in (va.fleet.vals, va.fleet.fc_store, va.fleet.status, va.fleet.obj)]
    out = va.step(P[1])
    plain.step(P[1])
    assert va.fleet.calls[-1] == [1, -1, 1]
    for k, x in zip(("vals", "fc_store", "status", "obj"), keep):
        now = getattr(va.fleet, k)
        cols = slice(3, 6)
        assert torch.equal(_bits(now[:, cols] if k == "vals" else now[cols]), _bits(x[:, cols] if k == "vals" else x[cols]))
    assert out[0].tolist() == eps[0].step(P[1][0]) and out[2].tolist() == eps[2].step(P[1][2])
    assert out[1].tolist() == eps[1].rows[-1]                   # (an idle episode's sums: its last step's)
    va.resume([1])
    plain.resume([1])
    # reset episode 2 alone at a new start: only its fleet group is cleared
    before = StandInFleet.__new__(StandInFleet)
    for k in ("vals", "fc_store", "status", "obj"):
        setattr(before, k, getattr(va.fleet, k).clone())
    before.Mb = 3
    va.reset([2], start_indices=[0, 0, 20])
    plain.reset([2], start_indices=[0, 0, 20])
    assert _fleet_equal(va.fleet, before, groups=[0, 1])
    assert bool(torch.isnan(va.fleet.vals[:, 6:]).all()) and bool(torch.isnan(va.fleet.fc_store[6:]).all())
    assert bool(torch.isnan(va.fleet.obj[6:]).all()) and int(va.fleet.status[6:].abs().sum()) == 0
    assert float(va.ev_agg_hist[:, 2].abs().sum()) == 0.0 and float(va.ev_agg_hist[:, 0].abs().sum()) > 0.0
    eps[2] = Episode(SEEDS[2], 20)
    for p in P[2:5]:
        out = va.step(p)
        plain.step(p)
        for e in range(3):
            assert out[e].tolist() == eps[e].step(p[e]), e
    assert va.clocks_host() == [5, 4, 3] and va.done().tolist() == [True, False, False]
    # episode 0 is finished and sits idle: the fleet sees its clock as -1
    out = va.step(P[5])
    plain.step(P[5])
    assert va.fleet.calls[-1] == [-1, 4, 3]
    assert out[0].tolist() == eps[0].rows[-1]
    for e in (1, 2):
        assert out[e].tolist() == eps[e].step(P[5][e])
    # the filed rows, by each episode's own clock; the homes never saw the fleet
    for e in range(3):
        n = va.clocks_host()[e]
        assert va.episode_sums(e).tolist() == eps[e].rows[:n]
        assert va.ev_agg_hist[:n, e].tolist() == eps[e].ev_rows[:n]
        assert float(va.ev_agg_hist[n:, e].abs().sum()) == 0.0
    assert torch.equal(_bits(va.hist), _bits(plain.hist)) and torch.equal(va.status_hist, plain.status_hist)
    assert torch.equal(_bits(va.batch.vals), _bits(plain.batch.vals))
    assert torch.equal(_bits(va.agg_hist), _bits(plain.agg_hist + va.ev_agg_hist))
    assert va.ev_sums is va.fleet.sums and va.ev_sums[1].tolist() == eps[1].ev_rows[-1]
    # reset everything
    va.reset()
    assert bool(torch.isnan(va.fleet.vals).all()) and float(va.ev_agg_hist.abs().sum()) == 0.0


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("classes", [False, True])
def test_sweep_and_commit_equal_step_under_the_chosen_rows(K, classes):
    def fresh():
        va = _va(classes=classes)
        va.step([[0.25, 0.5]] * 3 if classes else [0.25] * 3)
        va.park([1])
        return va
    cand = torch.tensor([[[0.5, -0.25], [0.0, 0.75]], [[0.25, 0.25], [0.5, 0.0]], [[-0.5, 0.5], [0.25, -0.25]]],
                        dtype=torch.float64)                     # [E][C][P]
    if not classes:
        cand = cand[..., 0]
    va = fresh()
    live = [x.clone() for x in (va.fleet.vals, va.fleet.fc_store, va.fleet.status, va.fleet.obj)]
    sums = va.sweep(cand, steps=K)
    assert tuple(sums.shape) == ((3, 2, K, 3) if K > 1 else (3, 2, 3))
    for k, x in zip(("vals", "fc_store", "status", "obj"), live):       # the live fleet is only read
        assert torch.equal(_bits(getattr(va.fleet, k)), _bits(x))
    for c in range(2):
        twin = fresh()
        for j in range(K):
            want = twin.step(cand[:, c])
            got = sums[:, c, j] if K > 1 else sums[:, c]
            assert torch.equal(_bits(got[[0, 2]]), _bits(want[[0, 2]])), (c, j)
    choice = torch.tensor([1, 0, 0], dtype=torch.int32)
    out = va.commit(choice)
    twin = fresh()
    want = twin.step(torch.stack([cand[0, 1], cand[1, 0], cand[2, 0]]))
    assert torch.equal(_bits(out), _bits(want))
    assert _fleet_equal(va.fleet, twin.fleet) and torch.equal(_bits(va.batch.vals), _bits(twin.batch.vals))
    assert torch.equal(_bits(va.agg_hist), _bits(twin.agg_hist)) and torch.equal(_bits(va.ev_agg_hist), _bits(twin.ev_agg_hist))
    assert torch.equal(va.clocks, twin.clocks) and va.clocks_host() == [2, 1, 2]
    # a choice outside [0, C) adopts nothing, for the fleet too
    va.sweep(cand, steps=K)
    keep = [x.clone() for x in (va.fleet.vals, va.fleet.fc_store, va.fleet.status, va.fleet.obj)]
    va.commit(torch.tensor([-1, 5, 2], dtype=torch.int32))
    for k, x in zip(("vals", "fc_store", "status", "obj"), keep):
        assert torch.equal(_bits(getattr(va.fleet, k)), _bits(x))
    # a step voids a held sweep, for the fleet too
    va.sweep(cand, steps=K)
    va.step(cand[:, 0])
    twin.step(cand[:, 0])
    with pytest.raises(ValueError, match="no sweep"):
        va.commit(choice)
    assert _fleet_equal(va.fleet, twin.fleet)


def test_device_paths_file_the_same_sums_on_a_stand_in():
    """step_env / commit_env / reset_env (the stand-in batch serves the env kernels with their restatements)."""
    va, host = _va(), _va()
    st = va.env_state(3, 40.0, 9.0)
    p = [[0.25, 0.5], [0.0, -0.25], [0.5, 0.5]]
    for _ in range(2):
        a, b = va.step_env(st, p), host.step(p)
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(va.agg_hist), _bits(host.agg_hist)) and torch.equal(_bits(va.ev_agg_hist), _bits(host.ev_agg_hist))
    assert st.obs[0].tolist() == host.agg_hist[1, :, 0].tolist()
    va.reset_env(st, [1])
    host.reset([1])
    assert _fleet_equal(va.fleet, host.fleet) and torch.equal(_bits(va.ev_agg_hist), _bits(host.ev_agg_hist))
    cand = torch.tensor([[[0.5, -0.25], [0.0, 0.75]]] * 3, dtype=torch.float64)
    va.sweep(cand, steps=2)
    host.sweep(cand, steps=2)
    ch = torch.tensor([1, 0, 1], dtype=torch.int32)
    assert torch.equal(_bits(va.commit_env(st, ch)), _bits(host.commit(ch)))
    assert _fleet_equal(va.fleet, host.fleet) and torch.equal(_bits(va.ev_agg_hist), _bits(host.ev_agg_hist))
    assert torch.equal(va.clocks, host.clocks)


# ------------------------------------------------------------------ the environments' max_poss_load
def test_max_poss_load_counts_the_vehicles_only_when_they_are_on():
    from dragg_amd import inputs as I
    from dragg_amd.rl import DeviceVectorEnv, VectorEnv
    parts = {"hems": {"sub_subhourly_steps": 6}, "hvac": {"p_c": 3.5, "p_h": 3.0}, "wh": {"p": 2.5}}
    homes = [dict(h, **parts) for h in HOMES]
    own = sum(I.max_load(h) for h in homes)
    on, off = _va(homes=homes), _va(homes=homes, vehicles=False)
    for cls in (VectorEnv, DeviceVectorEnv):
        assert cls(off, CFG).max_poss_load == own
        assert cls(on, CFG).max_poss_load == own + sum(RATES.values())
        assert cls(on, CFG, max_poss_load=40.0).max_poss_load == 40.0
    assert DeviceVectorEnv(on, CFG).state.max_poss_load == own + sum(RATES.values())


def test_rl_vector_asks_the_caller_to_choose():
    from dragg_amd.runner import Aggregator
    r = Aggregator.__new__(Aggregator)
    r.world, r.config = 1, {"home": {"ev": {"share": 0.5}}}
    with pytest.raises(NotImplementedError, match="EV fleet.*vehicles=True"):
        r.rl_vector(2)
