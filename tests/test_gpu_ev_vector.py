"""EV fleets in the vector environments on the GPU: dragg_mpc_ev_step_episodes, dragg_mpc_ev_aggregate_onto,
dragg_mpc_ev_adopt, dragg_mpc_ev_reset and `VectorAggregator(vehicles=True)` on top of them.

Every comparison is bit for bit against an entry that is already pinned to the independent LP
(tests/test_gpu_ev.py): a plain `EVFleet` stepped by dragg_mpc_ev_step, or a single `DeviceAggregator(ev=...)` run.
dt = 4, so a day has D = 96 steps."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ev_cases as EC
from tests.arena import Arena, same_bytes
from tests.test_gpu_vector import SEEDS, STARTS, T, community  # noqa: F401  (community: the fixture)

pytestmark = pytest.mark.gpu

N_ENV = 160
START0 = 40                     # the fleet's own start index: one group's start lies below it
DAY0 = 29                       # the step of day of environment index START0 (departures lie in 24 .. 36)
CLOCKS = [0, 3, -1, 7, 2]
KEYS = ("vals", "fc_store", "status", "obj")


def _bits(x):
    return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x


def _i32(x, dev):
    return torch.tensor(list(x), dtype=torch.int32, device=dev)


def _state(f):
    return {k: getattr(f, k).clone() for k in KEYS}


def _group(s, g, Mb):
    """Group g's part of a fleet's state (a dict of `_state`), vehicle-major."""
    sl = slice(g * Mb, (g + 1) * Mb)
    return {k: (v[:, sl] if k == "vals" else v[sl]) for k, v in s.items()}


def _same(a, b, what):
    for k in KEYS:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


def _put(f, s):
    for k in KEYS:
        getattr(f, k).copy_(s[k])


# ------------------------------------------------------------------ 1. groups equal single fleets
@pytest.mark.parametrize("Mb", [1, 5, 85])
@pytest.mark.parametrize("H", [2, 33, 48], ids=EC.batch_id)
def test_groups_equal_single_fleets(H, Mb, gpu):
    """E = 5 groups with their own clocks, starts and price rows; the previous state seeded by twelve shared steps in
    the middle of the day (every vehicle away: the too-large trips run empty, so infeasible vehicles exist whatever
    the day clock).  Group 2 is idle by its clock, group 4 by the device rule (its window leaves the lists)."""
    from dragg_amd import _lib as L
    from dragg_amd.ev import EVFleet, ev_episode_day_step
    cs = EC.cases(H)
    assert len(cs) == 85
    homes = EC.fleet_homes(cs, H)[:Mb]
    rng = np.random.default_rng([H, Mb])
    tou = 0.07 + 0.03 * rng.standard_normal(N_ENV)
    rows = 0.03 * rng.standard_normal((5, H))
    starts = [40, 0, 7, 95, N_ENV - H - 2]
    g = EVFleet(homes, tou, START0, rows, day_offset=DAY0, groups=5)
    dev = g.device
    g.day_offset = 40                                   # seeding: day steps 40 .. 51, between every departure and return
    for t in range(12):
        g.step(t)
    g.day_offset = DAY0
    # the idle groups hold a pattern that is neither NaN nor a result
    for e, tag in ((2, 1234.5), (4, -77.25)):
        sl = slice(e * Mb, (e + 1) * Mb)
        g.vals[:, sl] = tag
        g.fc_store[sl] = tag + 1
        g.obj[sl] = tag + 2
        g.status[sl] = 77 + e
    before = _state(g)
    g.step_episodes(_i32(starts, dev), _i32(CLOCKS, dev))
    after = _state(g)
    for e in (2, 4):
        _same(_group(after, e, Mb), _group(before, e, Mb), ("idle", e))
    for e in (0, 1, 3):
        f = EVFleet(homes, tou, starts[e], rows[e],
                    day_offset=ev_episode_day_step(DAY0, START0, starts[e], 0, EC.DT))
        _put(f, _group(before, e, Mb))
        f.step(CLOCKS[e])
        got = _group(after, e, Mb)
        _same(got, _state(f), ("group", e))
        st = got["status"].cpu().numpy()
        moved = (got["vals"][L.EVK["p_ev_ch"]] + got["vals"][L.EVK["p_ev_disch"]] != 0).any().item()
        print(f"H {H} Mb {Mb} group {e}: optimal {(st == L.EV_OPTIMAL).sum()}, infeasible {(st == L.EV_INFEASIBLE).sum()}, "
              f"moved {moved}")
        if Mb == 85:
            assert (st == L.EV_OPTIMAL).any() and (st == L.EV_INFEASIBLE).any() and moved, e
    # the day clocks: one start below the fleet's own, one clock that wraps past midnight inside the horizon
    days = [ev_episode_day_step(DAY0, START0, starts[e], CLOCKS[e], EC.DT) for e in (0, 1, 3)]
    assert days == [29, 88, 91]


# ------------------------------------------------------------------ 2. shared keys
@pytest.mark.parametrize("G", [1, 3])
def test_shared_keys_are_the_plain_step(G, gpu):
    from dragg_amd.ev import EVFleet
    H = 33
    homes = EC.fleet_homes(EC.cases(H), H)[:21]
    rng = np.random.default_rng(G)
    tou = 0.07 + 0.03 * rng.standard_normal(H + 12)
    rows = 0.03 * rng.standard_normal((G, H))
    a, b = (EVFleet(homes, tou, 2, rows if G > 1 else rows[0], day_offset=20, groups=G) for _ in range(2))
    for t in range(3):
        a.step(t)
        b.step_episodes(None, None, t=t)
        _same(_state(a), _state(b), t)


# ------------------------------------------------------------------ 3. classes
def test_classes_pick_the_row(gpu):
    """P = 2, Mb = 5, E = 2; the map on the device holds one value out of range on each side (clamped to 0 / P - 1)."""
    from dragg_amd.ev import EVFleet
    H, Mb, E = 33, 5, 2
    homes = EC.fleet_homes(EC.cases(H), H)[:Mb]
    rng = np.random.default_rng(33)
    tou = 0.07 + 0.03 * rng.standard_normal(N_ENV)
    rows = 0.03 * rng.standard_normal((E, 2, H))
    f = EVFleet(homes, tou, START0, day_offset=DAY0, groups=E)
    f.set_price_classes([0, 1, 0, 1, 1], 2)
    f.price_class = torch.tensor([0, 1, -3, 7, 1], dtype=torch.int32, device=f.device)
    f.set_reward_price(rows)
    eff = [0, 1, 0, 1, 1]
    starts, clocks = _i32([7, 95], f.device), _i32([0, 0], f.device)
    plain = []
    for c in range(2):
        p = EVFleet(homes, tou, START0, rows[:, c], day_offset=DAY0, groups=E)
        plain.append(p)
    for t in range(2):
        clocks = _i32([t, t], f.device)
        f.step_episodes(starts, clocks)
        for p in plain:
            p.step_episodes(starts, clocks)
        got = _state(f)
        for e in range(E):
            for v in range(Mb):
                r = e * Mb + v
                want = _state(plain[eff[v]])
                for k in KEYS:
                    x, y = (got[k][:, r], want[k][:, r]) if k == "vals" else (got[k][r], want[k][r])
                    assert torch.equal(_bits(x), _bits(y)), (t, e, v, k)
    assert not torch.equal(_bits(plain[0].vals), _bits(plain[1].vals))        # (the rows matter)


# ------------------------------------------------------------------ 4. aggregate_onto
@pytest.mark.parametrize("Mb", [1, 5, 1100])
def test_aggregate_onto(Mb, gpu):
    from dragg_amd.ev import EVFleet
    H, G = 2, 3
    cs = EC.fleet_homes(EC.cases(H), H)
    homes = (cs * (Mb // len(cs) + 1))[:Mb]
    rng = np.random.default_rng(Mb)
    f = EVFleet(homes, 0.07 + 0.03 * rng.standard_normal(16), 0, 0.03 * rng.standard_normal((G, H)), day_offset=30, groups=G)
    f.step(0)
    s = f.aggregate_groups().clone()
    base = torch.tensor(rng.standard_normal((G, 3)) * 10, dtype=torch.float64, device=f.device)
    base[1, 2] = float("nan")
    want = base + s
    nan = torch.isnan(want)
    assert nan.sum().item() == 1 and nan[1, 2]
    out = torch.zeros_like(base)
    keep = base.clone()
    assert f.aggregate_onto(base, out) is out
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(base), _bits(keep))
    assert torch.equal(_bits(f.sums), _bits(s))                               # the fleet-only rows
    assert f.aggregate_onto(base) is base                                     # in place
    assert torch.equal(_bits(base), _bits(want))


def test_aggregate_onto_of_an_empty_fleet_is_the_base(gpu):
    from dragg_amd.ev import EVFleet
    H = 2
    bare = [{k: v for k, v in h.items() if k != "ev"} for h in EC.fleet_homes(EC.cases(H), H)[:3]]
    f = EVFleet(bare, [0.1] * 16, groups=3, template_home=bare[0])
    assert f.M == 0
    base = torch.tensor([[1.5, -0.0, float("nan")], [0.0, -2.0, 3.0], [-0.0, 0.0, 1e300]], dtype=torch.float64,
                        device=f.device)
    out = torch.full_like(base, 7.0)
    f.sums.fill_(5.0)
    f.aggregate_onto(base, out)
    assert torch.equal(_bits(out), _bits(base)) and float(f.sums.abs().sum()) == 0.0
    f.step_episodes(None, None)                                               # a no-op


# ------------------------------------------------------------------ 5. adopt and reset, byte for byte
def _fleet_arena(E, C, Mb, H, off):
    from dragg_amd import _lib as L
    a = Arena()
    for side, G, (od, oi) in (("src", C * E, (off[0], off[2])), ("dst", E, (off[1], off[3]))):
        M = G * Mb
        a.add(f"{side}_vals", np.float64, (L.NEVV, M), od)
        a.add(f"{side}_fc", np.float64, (M, L.NEVK, H), od)
        a.add(f"{side}_obj", np.float64, (M,), od)
        a.add(f"{side}_status", np.int32, (M,), oi)
    return a


def _ev_struct(a, dev, side, M):
    from dragg_amd import _lib as L
    p = lambda k: ctypes.c_void_p(a.ptr(dev, f"{side}_{k}"))   # noqa: E731
    return L.Ev(params=None, vals=p("vals"), fc=p("fc"), status=p("status"), obj=p("obj"), day_offset=0, n_vehicles=M)


@pytest.mark.parametrize("off", [(0, 0, 0, 0), (8, 8, 4, 4), (0, 8, 8, 12)])
@pytest.mark.parametrize("choice", [[1, -1, 0], [0, 2, 1]])
def test_adopt_and_reset_move_the_groups_bytes_alone(choice, off, gpu):
    """E = 3, C = 2, Mb = 5, H = 2: the whole allocation (arrays and guard bytes) against the numpy restatement."""
    from dragg_amd import _lib as L
    E, C, Mb, H = 3, 2, 5, 2
    lib = L.load()
    a = _fleet_arena(E, C, Mb, H, off)
    host = a.random(np.random.default_rng(sum(off) + choice[0]))
    dev = a.upload(host.copy(), "cuda")
    dims = L.Dims(n_homes=E * Mb, horizon=H, sub_steps=6, dt=4, n_draw_hours=1, n_env=0, n_rp=1, int_mode=L.INT_ROUND,
                  max_iter=0, check_every=0, discount=0.9, flags=0, n_groups=E)
    src, dst = _ev_struct(a, dev, "src", C * E * Mb), _ev_struct(a, dev, "dst", E * Mb)
    ch = torch.tensor(choice, dtype=torch.int32, device="cuda")
    L.check(lib.dragg_mpc_ev_adopt(dims, C, L.ptr(ch), src, dst, None))
    torch.cuda.synchronize()
    want = host.copy()
    for e, c in enumerate(choice):
        if not 0 <= c < C:
            continue
        d, s = slice(e * Mb, (e + 1) * Mb), slice((c * E + e) * Mb, (c * E + e + 1) * Mb)
        a.view(want, "dst_vals")[:, d] = a.view(host, "src_vals")[:, s]
        for k in ("fc", "obj", "status"):
            a.view(want, f"dst_{k}")[d] = a.view(host, f"src_{k}")[s]
    got = dev.cpu().numpy()
    assert same_bytes(got, want, a)
    # reset: the masked groups alone
    mask = torch.tensor([True, False, True], device="cuda")
    L.check(lib.dragg_mpc_ev_reset(dims, dst, L.ptr(mask), None))
    torch.cuda.synchronize()
    nan = np.uint64(0x7FF8000000000000)
    for e in (0, 2):
        d = slice(e * Mb, (e + 1) * Mb)
        a.view(want, "dst_vals").view(np.uint64)[:, d] = nan
        a.view(want, "dst_fc").view(np.uint64)[d] = nan
        a.view(want, "dst_obj").view(np.uint64)[d] = nan
        a.view(want, "dst_status")[d] = 0
    got = dev.cpu().numpy()
    assert same_bytes(got, want, a)
    # a double array 4 bytes off: DRAGG_E_ARG, nothing written
    bad = _ev_struct(a, dev, "dst", E * Mb)
    bad.vals = ctypes.c_void_p(a.ptr(dev, "dst_vals") + 4)
    assert lib.dragg_mpc_ev_adopt(dims, C, L.ptr(ch), src, bad, None) == -1
    assert lib.dragg_mpc_ev_reset(dims, bad, L.ptr(mask), None) == -1
    torch.cuda.synchronize()
    assert same_bytes(dev.cpu().numpy(), want, a)


def test_fleet_methods_equal_the_entries_restated(gpu):
    """EVFleet.adopt_from / reset_groups / replicate_from (E-group base) on a live fleet."""
    from dragg_amd.ev import EVFleet
    H, Mb, E, C = 2, 5, 3, 2
    homes = EC.fleet_homes(EC.cases(H), H)[:Mb]
    rng = np.random.default_rng(5)
    tou = 0.07 + 0.03 * rng.standard_normal(16)
    live = EVFleet(homes, tou, 0, 0.03 * rng.standard_normal((E, H)), day_offset=30, groups=E)
    rep = EVFleet(homes, tou, 0, 0.03 * rng.standard_normal((C * E, H)), day_offset=30, groups=C * E)
    live.step(0)
    rep.replicate_from(live)
    s, r = _state(live), _state(rep)
    for c in range(C):
        for e in range(E):
            _same(_group(r, c * E + e, Mb), _group(s, e, Mb), ("replicate", c, e))
    rep.step(1)
    r = _state(rep)
    live.adopt_from(rep, _i32([1, -1, 0], live.device))
    got = _state(live)
    _same(_group(got, 0, Mb), _group(r, E + 0, Mb), "adopt 0")
    _same(_group(got, 1, Mb), _group(s, 1, Mb), "adopt 1")
    _same(_group(got, 2, Mb), _group(r, 2, Mb), "adopt 2")
    live.reset_groups(torch.tensor([False, True, False], device=live.device))
    now = _state(live)
    _same(_group(now, 0, Mb), _group(got, 0, Mb), "reset 0")
    _same(_group(now, 2, Mb), _group(got, 2, Mb), "reset 2")
    fresh = _state(EVFleet(homes, tou, 0, day_offset=30))
    _same(_group(now, 1, Mb), fresh, "reset 1")


# ------------------------------------------------------------------ 6. end to end
DAY_ENV0 = 26                   # the step of day of environment index 0 (06:30)


@pytest.fixture(scope="module")
def ev_community(community):   # noqa: F811
    from dragg_amd.community import ev_sections
    homes, weather = community
    homes = [dict(h) for h in homes]
    for i, sec in ev_sections(len(homes), 0.5, 4, 9).items():
        homes[i]["ev"] = sec
    return homes, weather


def _trajectory(steps=T + 2):
    """Nonzero per-episode price lists: [steps][3][24]."""
    from tests.test_gpu_sweep import _prices
    base = _prices()
    return np.stack([base * (1.0 + 0.25 * t) + 0.01 * (t + 1) * np.array([[1.0], [-1.0], [0.5]]) for t in range(steps)])


def _vector(ev_community, vehicles=True, steps=T, **kw):
    from dragg_amd.vector import VectorAggregator
    homes, (oat, ghi, tou) = ev_community
    ev = dict(vehicles=True, day_offset=DAY_ENV0) if vehicles else {}
    return VectorAggregator(homes, oat, ghi, tou, 3, list(SEEDS), list(STARTS), steps, **ev, **kw)


_RUNS = {}


def _single(ev_community, seed, start, prices):
    """A single DeviceAggregator(ev=...) run (existing code) under the price lists `prices` -> per step the sums,
    and the final state of homes and fleet.  Cached and never written."""
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.ev import EVFleet, ev_episode_day_step
    key = (seed, start, np.asarray(prices).tobytes())
    if key in _RUNS:
        return _RUNS[key]
    homes, (oat, ghi, tou) = ev_community
    fleet = EVFleet(homes, tou, start, prices[0], day_offset=ev_episode_day_step(DAY_ENV0, 0, start, 0, 4))
    agg = DeviceAggregator(homes, oat, ghi, tou, start, len(prices), reward_price=prices[0], seed=seed, ev=fleet)
    sums = []
    for p in prices:
        agg.set_reward_price(p)
        agg.run_iteration()
        sums.append(agg.collect_data().clone())
    _RUNS[key] = dict(sums=torch.stack(sums), fleet=_state(fleet), vals=agg.batch.vals.clone(),
                      ev_sums=agg.ev_agg_hist.clone())
    return _RUNS[key]


def test_episodes_equal_single_runs_with_a_fleet(gpu, ev_community):
    """E = 3 under their own price trajectories; episode 1 starts over after two steps at a new start.  Rows and
    fleet state are the single runs'; the homes' rows are those of the aggregator without vehicles."""
    P = _trajectory()
    va, plain = _vector(ev_community), _vector(ev_community, vehicles=False)
    Mb = va.fleet.Mb
    assert Mb == 8 and va.fleet.groups == 3
    for t in range(2):
        for x in (va, plain):
            x.step(P[t])
    first = _single(ev_community, SEEDS[1], STARTS[1], P[:2, 1])
    assert torch.equal(_bits(va.agg_hist[:2, 1]), _bits(first["sums"]))
    _same(_group(_state(va.fleet), 1, Mb), first["fleet"], "episode 1 before its reset")
    for x in (va, plain):
        x.reset([1], start_indices=[0, 3, 0])
    for t in range(2, T):
        plain.step(P[t])
        out = va.step(P[t])
    refs = [_single(ev_community, SEEDS[0], STARTS[0], P[:T, 0]), _single(ev_community, SEEDS[1], 3, P[2:T, 1]),
            _single(ev_community, SEEDS[2], STARTS[2], P[:T, 2])]
    assert va.clocks_host() == [T, T - 2, T]
    state = _state(va.fleet)
    for e, ref in enumerate(refs):
        n = va.clocks_host()[e]
        assert torch.equal(_bits(va.agg_hist[:n, e]), _bits(ref["sums"])), e
        assert torch.equal(_bits(va.ev_agg_hist[:n, e]), _bits(ref["ev_sums"])), e
        assert torch.equal(_bits(out[e]), _bits(ref["sums"][-1])), e
        _same(_group(state, e, Mb), ref["fleet"], ("fleet", e))
        assert torch.equal(_bits(va.batch.vals[:, e * va.Nb:(e + 1) * va.Nb]), _bits(ref["vals"])), e
    assert float(va.ev_agg_hist[T - 2:, 1].abs().sum()) == 0.0                 # (cleared by the reset)
    assert (va.ev_agg_hist[:, :, 0] != 0).any()
    # the homes never see the fleet
    for k in ("hist", "status_hist", "path_hist"):
        assert torch.equal(_bits(getattr(va, k)), _bits(getattr(plain, k))), k
    assert torch.equal(_bits(va.batch.vals), _bits(plain.batch.vals))
    assert torch.equal(_bits(va.batch.fc_store), _bits(plain.batch.fc_store))
    assert torch.equal(_bits(va.agg_hist), _bits(plain.agg_hist + va.ev_agg_hist))


@pytest.mark.parametrize("K", [1, 2])
def test_sweep_rows_and_commit_equal_steps(K, gpu, ev_community):
    P = _trajectory()

    def fresh():
        va = _vector(ev_community)
        va.step(P[0])
        return va
    cand = torch.as_tensor(np.stack([P[1], P[2]], axis=1))                     # [E][C = 2][24]
    va = fresh()
    live = _state(va.fleet)
    sums = va.sweep(cand, steps=K)
    _same(_state(va.fleet), live, "the live fleet is only read")
    for c in range(2):
        twin = fresh()
        for j in range(K):
            want = twin.step(cand[:, c])
            got = sums[:, c, j] if K > 1 else sums[:, c]
            assert torch.equal(_bits(got), _bits(want)), (c, j)
    choice = torch.tensor([1, 0, 1], dtype=torch.int32, device=va.device)
    out = va.commit(choice)
    twin = fresh()
    want = twin.step(torch.stack([cand[0, 1], cand[1, 0], cand[2, 1]]))
    assert torch.equal(_bits(out), _bits(want))
    _same(_state(va.fleet), _state(twin.fleet), "commit")
    for k in ("hist", "status_hist", "agg_hist", "ev_agg_hist"):
        assert torch.equal(_bits(getattr(va, k)), _bits(getattr(twin, k))), k
    assert torch.equal(_bits(va.batch.vals), _bits(twin.batch.vals)) and torch.equal(va.clocks, twin.clocks)


def test_device_and_host_environments_agree_with_vehicles(gpu, ev_community):
    from dragg_amd import inputs as I
    from dragg_amd.rl import DeviceVectorEnv, SweepAgent, VectorEnv
    from tests.test_gpu_env import _cfg, _same_obs, _same_state
    homes = ev_community[0]
    host, dev = VectorEnv(_vector(ev_community), _cfg()), DeviceVectorEnv(_vector(ev_community), _cfg())
    rates = sum(h["ev"]["max_rate"] for h in homes if "ev" in h)
    assert host.max_poss_load == dev.max_poss_load == sum(I.max_load(h) for h in homes) + rates
    agent = SweepAgent(_cfg(), n_candidates=3, lookahead=2)
    obs_h, obs_d = host.reset(), dev.reset()
    P = _trajectory()
    for k in range(T):
        if k == 1:
            obs_h, done_h = host.step_swept(agent.act_vector(obs_h), lookahead=2)
            obs_d, done_d = dev.step_swept(agent.act_device(obs_d), lookahead=2)
            assert host.choice.tolist() == dev.choice.cpu().tolist()
        else:
            obs_h, done_h = host.step(P[k])
            obs_d, done_d = dev.step(P[k])
        assert done_h.tolist() == done_d.cpu().tolist()
        _same_obs(obs_h, obs_d, k)
        _same_state(host, dev, k)
        _same(_state(host.va.fleet), _state(dev.va.fleet), k)
        assert torch.equal(_bits(host.va.ev_agg_hist), _bits(dev.va.ev_agg_hist)), k
    assert done_h.all()


def test_rl_vector_with_and_without_the_vehicles(gpu, tmp_path):
    from dragg_amd import runner
    from tests import fixtures as F
    from tests.test_gpu_commit import _synthetic_data
    params = dict(n=12, batt=3, pv=3, pvb=2, start="2015-01-01 00", end="2015-01-01 03", dt=2, horizon=6,
                  action_horizon=6, seed=21)
    envs = {}
    for name, extra in (("ev", "\n[home.ev]\nshare = 0.5\ndepart_hour = [0.5, 1.5]\n"), ("bare", "")):
        data = tmp_path / f"data_{name}"
        data.mkdir()
        _synthetic_data(str(data))
        with open(data / "config.toml", "w") as f:
            f.write(F.config_text(params) + extra)
        a = runner.Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / f"outputs_{name}"))
        a.get_homes()
        if name == "ev":
            with pytest.raises(NotImplementedError, match="EV fleet"):
                a.rl_vector(2)
            envs["on"] = a.rl_vector(2, vehicles=True)
            envs["off"] = a.rl_vector(2, vehicles=False)
        else:
            envs["bare"] = a.rl_vector(2)
    on, off, bare = envs["on"], envs["off"], envs["bare"]
    fleet = on.va.fleet
    assert fleet is not None and fleet.Mb == 6 and fleet.groups == 2 and off.va.fleet is None
    assert fleet.day_offset == (0 - on.va.starts[0].item()) % 48
    assert on.max_poss_load > off.max_poss_load == bare.max_poss_load
    for env in envs.values():
        env.reset()
    price = np.full((2, 1), 0.01)
    obs = {k: env.step(price)[0] for k, env in envs.items()}
    for k in ("agg_load", "forecast_load", "agg_cost"):
        assert np.array_equal(obs["off"][k], obs["bare"][k]), k
    assert torch.equal(_bits(on.va.batch.vals), _bits(off.va.batch.vals))
    assert torch.equal(_bits(on.va.agg_hist), _bits(off.va.agg_hist + on.va.ev_agg_hist))
    assert int((fleet.status == 0).sum()) > 0
