"""Plan observations on the GPU: dragg_mpc_plan_groups alone on patterned hash arrays against its numpy
restatement (`vector.plan_groups_reference`), bit for bit; its argument checks; `rl.DeviceVectorEnv`'s plan
observations over the closed loop of tests/test_gpu_env.py (E = 4, its community of 16 homes, T = 27, a masked
reset and a park); `DeviceAggregator.sweep_plan` of a held sweep against the restatement and against `plan()`
after `commit(g)`; and the environment's calls under torch's synchronisation debug mode."""
import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from tests.test_gpu_env import SEEDS, STARTS, _cfg
from tests.test_gpu_vector import community                       # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

CNT = L.K["solve_counter"]
NAN = float("nan")
ROWS4 = ("temp_in_opt", "e_batt", "correct_solve", "solve_counter")
KEY_MASKS = ((2,), (0, 14), tuple(range(L.NFC)))                  # one key, two non-adjacent keys, all 15
# The closed loop's episodes.  With tests/test_gpu_env.py's own keys (seeds 5, 6, 2^40 + 7, 9; starts 0, 7, 12, 3) no
# group-step of the loop has every home solved (measured: none; run undisturbed, each of the four reaches 14 of 16 at best), so the shift property would never be
# checked.  A search over seeds {5, 6, 2^40 + 7, 9, 77, 11} x starts 0..12 under the same policy found three
# episodes that have one: (seed 6, start 0) at step 10, (seed 11, start 0) at step 7 and (seed 11, start 1) at
# step 7.  Episodes 0 and 3 -- the two the loop neither restarts nor parks -- take the first two.
LOOP_SEEDS = (6, 5, 2 ** 40 + 7, 11)
LOOP_STARTS = (0, 7, 12, 0)


def _bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int64) if x.dtype == np.float64 else x


def _patterned(G, Nb, H, seed):
    """Hash arrays of G x Nb homes: values of both signs and very different magnitudes (so that the order of the
    adds shows in the last bits), NaN fields scattered over both arrays, the PV keys of every third home NaN
    throughout, one home all NaN, and the counters 0, 1, H-1, H, H+3 and NaN scattered over the homes."""
    rng = np.random.default_rng(seed)
    N = G * Nb
    vals = rng.uniform(-1.0, 1.0, (L.NVAL, N)) * 10.0 ** rng.integers(-3, 6, (L.NVAL, N))
    fc = rng.uniform(-1.0, 1.0, (N, L.NFC, H)) * 10.0 ** rng.integers(-3, 6, (N, L.NFC, H))
    vals[rng.random(vals.shape) < 0.1] = NAN
    fc[rng.random(fc.shape) < 0.1] = NAN
    pv = [L.K["p_pv_opt"], L.K["u_pv_curt_opt"]]
    vals[np.ix_(pv, np.arange(0, N, 3))] = NAN
    fc[0::3, pv] = NAN
    if N > 4:
        vals[:, 4], fc[4] = NAN, NAN
    counters = np.array([0.0, 1.0, H - 1.0, float(H), H + 3.0, NAN, 0.0, 2.0])
    vals[CNT] = counters[rng.permutation(N) % len(counters)]
    return vals, fc


def _launch(dev, vals, fc, G, keys, rows, H):
    """dragg_mpc_plan_groups on device copies of the arrays -> (curve, count, stats, the device copies)."""
    lib = L.load()
    km, rm, ki, ri = L.plan_select(keys, rows)
    N = vals.shape[1]
    d_vals, d_fc = torch.as_tensor(vals).to(dev).contiguous(), torch.as_tensor(fc).to(dev).contiguous()
    dims = L.Dims(n_homes=N, horizon=H, sub_steps=6, dt=1, n_groups=G if G > 1 else 0)
    curve = torch.full((G, len(ki), H), -7.0, dtype=torch.float64, device=dev)
    count = torch.full((G, len(ki), H), -7, dtype=torch.int32, device=dev)
    stats = torch.full((G, len(ri), 4), -7.0, dtype=torch.float64, device=dev)
    plan = L.Plan(fc_keys=km, val_rows=rm, curve=L.ptr(curve), count=L.ptr(count), stats=L.ptr(stats))
    rc = lib.dragg_mpc_plan_groups(dims, L.Hash(vals=L.ptr(d_vals), fc=L.ptr(d_fc)), plan, L.stream_ptr(None, dev))
    assert rc == 0
    torch.cuda.synchronize()
    return curve, count, stats, (d_vals, d_fc)


def _same(got, ref, ki_all, ki, ri_all, ri, what):
    """The launch's outputs against the rows of the full reference (every key, every row) it asked for."""
    curve, count, stats = got[:3]
    a = [ki_all.index(k) for k in ki]
    r = [ri_all.index(x) for x in ri]
    assert np.array_equal(_bits(curve), _bits(ref[0][:, a])), (what, "curve")
    assert np.array_equal(count.cpu().numpy(), ref[1][:, a]), (what, "count")
    s, s_ref = stats.cpu().numpy(), ref[2][:, r]
    assert np.array_equal(_bits(s[..., :2]), _bits(s_ref[..., :2])), (what, "stats count, sum")
    assert np.array_equal(s[..., 2:], s_ref[..., 2:]), (what, "stats min, max")        # (by value: a zero's sign is free)


# ------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("H", [6, 7, 24])
@pytest.mark.parametrize("Nb", [1, 15, 16, 17, 33])
def test_kernel_alone_equals_the_restatement(gpu, Nb, H):
    """Nb below, at and past one and two rounds of the 16 ways; an odd H leaves the homes' rows 8-byte aligned
    only; G = 1 and 3; the three key masks with the empty and the four-row mask.  int64 views throughout."""
    from dragg_amd.vector import plan_groups_reference
    all_keys, all_rows = list(range(L.NFC)), list(range(L.NVAL))
    rows4 = L.plan_select((), ROWS4)[3]
    for G in (1, 3):
        vals, fc = _patterned(G, Nb, H, seed=100 * Nb + H + G)
        ref = plan_groups_reference(vals, fc, G, all_keys, all_rows)
        for keys in KEY_MASKS:
            for rows in ((), rows4):
                got = _launch(gpu, vals, fc, G, keys, rows, H)
                _same(got, ref, all_keys, list(keys), all_rows, list(rows), (G, keys, rows))
                d_vals, d_fc = got[3]
                assert np.array_equal(_bits(d_vals), _bits(vals)) and np.array_equal(_bits(d_fc), _bits(fc)), "read only"
        # rows alone (no key: the curve outputs may be NULL)
        got = _launch(gpu, vals, fc, G, (), rows4, H)
        _same(got, ref, all_keys, [], all_rows, rows4, (G, "rows alone"))
        if G == 3:                                              # group g equals a G = 1 batch of its homes
            whole = _launch(gpu, vals, fc, G, all_keys, rows4, H)
            for g in range(G):
                cols = slice(g * Nb, (g + 1) * Nb)
                alone = _launch(gpu, np.ascontiguousarray(vals[:, cols]), np.ascontiguousarray(fc[cols]), 1, all_keys, rows4, H)
                for x, y in zip(whole[:3], alone[:3]):
                    assert np.array_equal(_bits(x[g]), _bits(y[0])), g


def test_bad_arguments_and_the_empty_batch(gpu):
    lib, dev = L.load(), gpu
    G, Nb, H = 2, 5, 6
    vals, fc = _patterned(G, Nb, H, seed=1)
    d_vals, d_fc = torch.as_tensor(vals).to(dev), torch.as_tensor(fc).to(dev)
    curve = torch.full((G, 2, H), -7.0, dtype=torch.float64, device=dev)
    count = torch.full((G, 2, H), -7, dtype=torch.int32, device=dev)
    stats = torch.full((G, 1, 4), -7.0, dtype=torch.float64, device=dev)
    stream = L.stream_ptr(None, dev)
    hsh = L.Hash(vals=L.ptr(d_vals), fc=L.ptr(d_fc))

    def dims(**kw):
        d = L.Dims(n_homes=G * Nb, horizon=H, sub_steps=6, dt=1, n_groups=G)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def plan(**kw):
        p = L.Plan(fc_keys=0b101, val_rows=1 << CNT, curve=L.ptr(curve), count=L.ptr(count), stats=L.ptr(stats))
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    E_ARG = -1
    assert lib.dragg_mpc_plan_groups(None, hsh, plan(), stream) == E_ARG
    assert lib.dragg_mpc_plan_groups(dims(), None, plan(), stream) == E_ARG
    assert lib.dragg_mpc_plan_groups(dims(), hsh, None, stream) == E_ARG
    for bad in (dict(fc_keys=1 << L.NFC), dict(fc_keys=0b101 | 1 << 31), dict(val_rows=1 << L.NVAL), dict(curve=None),
                dict(count=None), dict(stats=None)):
        assert lib.dragg_mpc_plan_groups(dims(), hsh, plan(**bad), stream) == E_ARG, bad
    for bad in (dict(horizon=0), dict(n_groups=3), dict(n_groups=-1), dict(n_homes=-1),
                dict(n_homes=65536 * 2, n_groups=65536)):
        assert lib.dragg_mpc_plan_groups(dims(**bad), hsh, plan(), stream) == E_ARG, bad
    assert lib.dragg_mpc_plan_groups(dims(), L.Hash(vals=None, fc=L.ptr(d_fc)), plan(), stream) == E_ARG
    assert lib.dragg_mpc_plan_groups(dims(), L.Hash(vals=L.ptr(d_vals), fc=None), plan(), stream) == E_ARG
    torch.cuda.synchronize()
    assert bool((curve == -7.0).all()) and bool((count == -7).all()) and bool((stats == -7.0).all())     # untouched
    # a zero mask with a NULL output is fine (and writes nothing of it); both masks zero: nothing at all
    assert lib.dragg_mpc_plan_groups(dims(), hsh, plan(fc_keys=0, curve=None, count=None), stream) == 0
    assert lib.dragg_mpc_plan_groups(dims(), L.Hash(vals=L.ptr(d_vals), fc=None), plan(fc_keys=0, curve=None, count=None),
                                     stream) == 0
    torch.cuda.synchronize()
    assert bool((curve == -7.0).all()) and bool((count == -7).all()) and float(stats[0, 0, 0]) >= 0.0
    stats.fill_(-7.0)
    assert lib.dragg_mpc_plan_groups(dims(), hsh, plan(fc_keys=0, val_rows=0, curve=None, count=None, stats=None), stream) == 0
    assert lib.dragg_mpc_plan_groups(dims(), hsh, plan(val_rows=0, stats=None), stream) == 0
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all()) and not bool((count == -7).any())
    # the empty batch: every group gets the empty result, the hash pointers may be NULL
    curve.fill_(-7.0)
    count.fill_(-7)
    assert lib.dragg_mpc_plan_groups(dims(n_homes=0), L.Hash(vals=None, fc=None), plan(), stream) == 0
    torch.cuda.synchronize()
    assert not curve.any() and not torch.signbit(curve).any() and not count.any()
    assert stats.cpu().tolist() == [[[0.0, 0.0, float("inf"), -float("inf")]]] * G
    # the Python layer names its own mistakes
    with pytest.raises(ValueError):
        L.plan_select(("no_such_key",))


# ------------------------------------------------------------------ the closed loop
def test_closed_loop_plan_observations(gpu, community):
    """tests/test_gpu_env.py's loop (E = 4, its community of 16 homes, T = 27, episode 1 started over at step 3
    with a new seed, episode 2 parked during steps 5-7; the seeds and starts: LOOP_SEEDS, LOOP_STARTS above) with
    plan observations: at every step they equal the restatement on the downloaded hash arrays bit for bit, entry 0 of
    p_grid is the step's agg_load to 1e-12, and where every home of a group solved (counter max 0, every count
    Nb) the forecast_p_grid curve is the p_grid curve shifted by one stage, bit for bit."""
    from dragg_amd.rl import DeviceVectorEnv, SetpointAgent
    from dragg_amd.vector import VectorAggregator, plan_groups_reference
    homes, (oat, ghi, tou) = community
    E, T, Nb = 4, 27, len(homes)
    va = VectorAggregator(homes, oat, ghi, tou, E, list(LOOP_SEEDS), list(LOOP_STARTS), T)
    keys = ("p_grid", "forecast_p_grid", "p_load", "p_pv")
    env = DeviceVectorEnv(va, _cfg(), plan_keys=keys, plan_rows=ROWS4)
    assert env.plan_key_names == list(keys)
    agent = SetpointAgent(_cfg())
    H = va.H
    one = torch.tensor([False, True, False, False], device=gpu)
    two = torch.tensor([False, False, True, False], device=gpu)
    n_zero = n_late = n_all_zero = n_shift = n_ran = 0

    def check(obs, what):
        nonlocal n_shift
        torch.cuda.synchronize()
        vals, fc = va.batch.vals.cpu().numpy(), va.batch.fc_store.cpu().numpy()
        ref = plan_groups_reference(vals, fc, E, keys, ROWS4)
        plan, count, stats = obs["plan"], obs["plan_count"], obs["plan_stats"]
        assert plan.is_cuda and tuple(plan.shape) == (E, len(keys), H) and count.dtype == torch.int32
        assert np.array_equal(_bits(plan), _bits(ref[0])), (what, "plan")
        assert np.array_equal(count.cpu().numpy(), ref[1]), (what, "plan_count")
        s = stats.cpu().numpy()
        assert np.array_equal(_bits(s[..., :2]), _bits(ref[2][..., :2])) and np.array_equal(s[..., 2:], ref[2][..., 2:]), what
        plan, count = plan.cpu().numpy(), count.cpu().numpy()
        load, ts = obs["agg_load"].cpu().numpy(), obs["timestep"].cpu().numpy()
        for e in range(E):
            if ts[e] == 0:                                       # a fresh episode: nothing planned, nothing collected
                assert not count[e].any() and s[e, 3, 0] == 0
                continue
            assert count[e, 0, 0] == Nb, (what, e)
            assert abs(plan[e, 0, 0] - load[e]) <= 1e-12 * abs(load[e]), (what, e, plan[e, 0, 0], load[e])
            if s[e, 3, 0] == Nb and s[e, 3, 3] == 0.0 and (count[e, 0] == Nb).all():       # every home solved
                n_shift += 1
                assert np.array_equal(_bits(plan[e, 1, :H - 1]), _bits(plan[e, 0, 1:])), (what, e)
        return vals[CNT].reshape(E, Nb)

    obs = env.reset()
    check(obs, "reset")
    k = 0
    while not bool(env.done().all()):
        if k == 3:
            obs = env.reset(one, seeds=torch.tensor([0, 77, 0, 0], device=gpu))
            agent.reset_device(one)
            check(obs, "masked reset")
        if k == 5:
            env.park(two)
        if k == 8:
            env.resume(two)
        ran = va.active().cpu().numpy()
        obs, done = env.step(agent.act_device(obs))
        cnt = check(obs, k)
        for e in np.flatnonzero(ran):                            # the home-steps this step took
            n_ran += Nb
            n_zero += int((cnt[e] == 0).sum())
            n_late += int((cnt[e] >= 1).sum())
            n_all_zero += int((cnt[e] == 0).all())
        k += 1
        assert k <= T + 3
    assert k == T + 3 and va.clocks_host() == [T] * E
    print(f"home-steps with counter 0: {n_zero}, with counter >= 1: {n_late}; group-steps with every home at "
          f"counter 0: {n_all_zero}; group-observations checked for the shift: {n_shift}")
    assert n_zero > 0 and n_late > 0 and n_zero + n_late == n_ran == (E * T + 3) * Nb     # (episode 1: 3 steps twice)
    assert n_all_zero > 0 and n_shift > 0


# ------------------------------------------------------------------ the held sweep
@pytest.fixture(scope="module")
def community20():
    from dragg_amd.community import synthetic_homes, synthetic_weather
    homes = synthetic_homes(80, seed=5, days=2, dt=4, horizon_hours=6)[::4]
    assert len(homes) == 20 and {h["type"] for h in homes} == {"base", "pv_only", "battery_only", "pv_battery"}
    return homes, synthetic_weather(2, 4, 24, seed=5, month=7)


@pytest.mark.parametrize("steps", [1, 2])
def test_sweep_plan_of_a_held_sweep(gpu, community20, steps):
    """G = 3 candidates against 20 homes after two committed steps; steps = 2 holds a `Held`."""
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.members import Held
    from dragg_amd.vector import plan_groups_reference
    homes, (oat, ghi, tou) = community20
    agg = DeviceAggregator(homes, oat, ghi, tou, 0, 8, reward_price=[0.0] * 24, seed=5)
    for _ in range(2):
        agg.run_iteration()
        agg.collect_data()
    keys = ("p_grid", "p_load", "cost", "e_batt")
    with pytest.raises(ValueError):
        agg.sweep_plan(keys)
    P = np.stack([np.full(24, 0.05), np.full(24, -0.03), -0.03 * np.cos(np.arange(24))])
    sums = agg.sweep(P, steps, hold=True)
    src = agg._hold["src"]
    assert isinstance(src, Held) == (steps == 2)
    curve, count, stats = (x.clone() for x in agg.sweep_plan(keys, ROWS4))
    torch.cuda.synchronize()
    H = agg.batch.H
    assert tuple(curve.shape) == (3, 4, H) and tuple(stats.shape) == (3, 4, 4)
    ref = plan_groups_reference(src.vals.cpu().numpy(), src.fc_store.cpu().numpy(), 3, keys, ROWS4)
    assert np.array_equal(_bits(curve), _bits(ref[0])) and np.array_equal(count.cpu().numpy(), ref[1])
    s = stats.cpu().numpy()
    assert np.array_equal(_bits(s[..., :2]), _bits(ref[2][..., :2])) and np.array_equal(s[..., 2:], ref[2][..., 2:])
    # entry 0 of p_grid is the candidate's first-step load, and the candidates differ
    first = sums[:, 0, 0].cpu().numpy()
    assert np.all(np.abs(curve[:, 0, 0].cpu().numpy() - first) <= 1e-12 * np.abs(first))
    assert not np.array_equal(_bits(curve[0]), _bits(curve[1]))
    # replica g's rows are the live batch's after commit(g)
    g = 2
    agg.commit(g)
    agg.collect_data()
    live = agg.plan(keys, ROWS4)
    torch.cuda.synchronize()
    for x, y in zip((curve, count, stats), live):
        assert tuple(y.shape)[0] == 1 and np.array_equal(_bits(x[g]), _bits(y[0]))
    with pytest.raises(ValueError):
        agg.sweep_plan(keys)                                      # the hold is spent


# ------------------------------------------------------------------ no host round trip
def test_plan_observations_do_not_synchronise(gpu, community):
    from dragg_amd.rl import DeviceVectorEnv, SetpointAgent, SweepAgent
    from dragg_amd.vector import VectorAggregator
    homes, (oat, ghi, tou) = community
    va = VectorAggregator(homes, oat, ghi, tou, 4, list(SEEDS), list(STARTS), 2)
    env = DeviceVectorEnv(va, _cfg(), plan_keys=("p_grid", "p_load"), plan_rows=("solve_counter",))
    pi, sw = SetpointAgent(_cfg()), SweepAgent(_cfg(), n_candidates=3)
    obs = env.reset()
    cands = sw.act_device(obs)
    seeds = torch.tensor([21, 22, 23, 24], device=gpu)
    starts = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=gpu)
    obs, _ = env.step(pi.act_device(obs))                    # (the first calls: code objects, workspaces)
    obs, _ = env.step_swept(cands)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        obs = env.reset(env.done(), seeds=seeds, start_indices=starts)
        pi.reset_device(env.done())
        obs, done = env.step(pi.act_device(obs))
        obs, done = env.step_swept(sw.act_device(obs))
        va.plan(("cost",))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert va.clocks_host() == [2] * 4 and bool(done.all())
    assert tuple(obs["plan"].shape) == (4, 2, va.H) and int(obs["plan_count"][:, 0, 0].min()) == len(homes)
