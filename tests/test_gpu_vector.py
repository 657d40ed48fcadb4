"""Vectorised episodes on the GPU (dragg_mpc_step_episodes, dragg_amd.vector.VectorAggregator): E
episodes of one community stepped as one grouped batch, each with its own season-noise seed, start index,
clock and reward-price row.

The reference of every test is existing code: a fresh single `DeviceAggregator` run with the episode's
seed, start index and price trajectory, stepped serially.  Every episode must equal it BIT FOR BIT (the
int64 views of the hash history, vals, fc, plus status, int_path and the collect_data sums).

Community: 16 homes of all four types (every fourth of 64), H = 24, April weather -- at H = 24 every
July draw is "summer" and a seed test would prove nothing; in April the season flag (max(oat + 1.1^k z_k)
<= 30) depends on the keyed draw.  The single runs are computed once per (seed, start, price) and shared."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_step import _noise_host
from tests.test_gpu_sweep import _prices

pytestmark = pytest.mark.gpu

MONTH = 4
SEEDS = (5, 6, 2 ** 40 + 7)          # (the high word feeds Philox's second key)
STARTS = (0, 7, 12)                  # (one is odd)
T = 4


def _bits(x):
    return x.contiguous().view(torch.int64)


@pytest.fixture(scope="module")
def community():
    from dragg_amd.community import synthetic_homes, synthetic_weather
    # (every fourth home: synthetic_homes lists the homes by type, so the first 16 of 64 hold two types only)
    homes = synthetic_homes(64, seed=5, days=2, dt=4, horizon_hours=6)[::4]
    assert len(homes) == 16 and {h["type"] for h in homes} == {"base", "pv_only", "battery_only", "pv_battery"}
    return homes, synthetic_weather(2, 4, 24, seed=5, month=MONTH)


_SINGLES = {}


def _single(homes, weather, seed, start, price, steps, int_mode="round", key=None):
    """A fresh single run (existing code), stepped serially: per step the hash history row, vals, fc,
    status, int_path and the sums, as clones.  Cached: the tests share the runs and never write them."""
    k = (key, len(homes), seed, start, None if price is None else tuple(np.asarray(price).tolist()), steps, int_mode)
    if k in _SINGLES:
        return _SINGLES[k]
    from dragg_amd.aggregator import DeviceAggregator
    oat, ghi, tou = weather
    agg = DeviceAggregator(homes, oat, ghi, tou, start, steps, reward_price=price, seed=seed, int_mode=int_mode)
    out = {"hist": [], "vals": [], "fc": [], "status": [], "path": [], "sums": []}
    for t in range(steps):
        agg.run_iteration()
        out["sums"].append(agg.collect_data().clone())
        b = agg.batch
        out["hist"].append(_bits(agg.hist[t]).clone())
        out["vals"].append(_bits(b.vals).clone())
        out["fc"].append(_bits(b.fc_store).clone())
        out["status"].append(b.status.clone())
        out["path"].append(b.int_path.clone())
    _SINGLES[k] = out
    return out


def _vector(homes, weather, seeds, starts, steps=T, int_mode="round"):
    from dragg_amd.vector import VectorAggregator
    oat, ghi, tou = weather
    return VectorAggregator(homes, oat, ghi, tou, len(seeds), list(seeds), list(starts), steps, int_mode=int_mode)


def _check_episode(va, e, ref, t, sums=None, what=""):
    """Episode e's columns after a step equal step t of the single run `ref`, bit for bit."""
    b, Nb = va.batch, va.Nb
    sl = slice(e * Nb, (e + 1) * Nb)
    assert torch.equal(_bits(b.vals[:, sl]), ref["vals"][t]), (what, e, t, "vals")
    assert torch.equal(_bits(b.fc_store[sl]), ref["fc"][t]), (what, e, t, "fc")
    assert torch.equal(b.status[sl], ref["status"][t]), (what, e, t, "status")
    assert torch.equal(b.int_path[sl], ref["path"][t]), (what, e, t, "int_path")
    if sums is not None:
        assert torch.equal(_bits(sums[e]), _bits(ref["sums"][t])), (what, e, t, "sums")


def _check_history(va, e, ref, lo, n, what=""):
    """Episode e's history rows equal steps [lo, lo + n) of the single run."""
    h = va.episode_history(e)
    assert h.shape[0] == n, (what, e, h.shape)
    st, pa, sm = va.episode_status(e), va.episode_paths(e), va.episode_sums(e)
    for i in range(n):
        assert torch.equal(_bits(h[i]), ref["hist"][lo + i]), (what, e, i, "hist")
        assert torch.equal(st[i], ref["status"][lo + i]) and torch.equal(pa[i], ref["path"][lo + i]), (what, e, i)
        assert torch.equal(_bits(sm[i]), _bits(ref["sums"][lo + i])), (what, e, i, "sums")


def _singles3(community, steps=T):
    homes, weather = community
    return [_single(homes, weather, SEEDS[e], STARTS[e], _prices()[e], steps) for e in range(3)]


def test_chosen_month_and_seeds_make_the_draw_matter(gpu, community):
    """On the CPU first (the host restatement of the keyed draw and the oracle's season test): two of the
    chosen seeds give different season flags at the same start; then, from the single runs' outputs: the
    seed changes the results, and at least half of the home-steps are optimal."""
    from dragg_amd import _lib as L
    from oracle.mpc import season_is_winter
    homes, weather = community
    oat = weather[0]
    flags = {s: np.array([[season_is_winter(oat[t:t + 25], _noise_host(s, h, t, 24)) for h in range(16)]
                          for t in range(T)]) for s in SEEDS[:2]}
    assert (flags[5] != flags[6]).any() and 0 < flags[5].mean() < 1
    a = _single(homes, weather, 5, 0, _prices()[0], T)
    b = _single(homes, weather, 6, 0, _prices()[0], T)
    assert any(not torch.equal(x, y) for x, y in zip(a["hist"], b["hist"]))
    st = torch.stack([s for r in _singles3(community) for s in r["status"]])
    print("optimal home-steps of the single runs:", int((st == L.ST_OPTIMAL).sum()), "of", st.numel())
    assert int((st == L.ST_OPTIMAL).sum()) * 2 >= st.numel()


def test_episodes_equal_single_runs(gpu, community):
    from dragg_amd import _lib as L
    homes, weather = community
    refs = _singles3(community)
    va = _vector(homes, weather, SEEDS, STARTS)
    P = torch.as_tensor(_prices(), dtype=torch.float64)
    for t in range(T):
        sums = va.step(P)
        for e in range(3):
            _check_episode(va, e, refs[e], t, sums)
    for e in range(3):
        _check_history(va, e, refs[e], 0, T)
    assert va.clocks_host() == [T] * 3 and bool(va.done().all())
    assert not torch.equal(_bits(va.episode_history(0)), _bits(va.episode_history(1)))
    # the prices put the hot path and the later launches side by side: an RL-priced episode's optimal
    # homes all finish in a later launch
    c = va.approx_counts()
    assert [len(c[k]) for k in ("approx_solves", "step_dp_solves", "later_launch_solves")] == [3, 3, 3]
    p = va.path_hist.view(T, 3, va.Nb)
    assert c["later_launch_solves"] == [int(((p[:, e] & L.PATH_SECOND) != 0).sum()) for e in range(3)]
    assert c["later_launch_solves"][1] > c["later_launch_solves"][0]
    # a further step finds every episode done: nothing moves
    before = _bits(va.batch.vals).clone()
    va.step(P)
    assert torch.equal(_bits(va.batch.vals), before) and va.clocks_host() == [T] * 3


def test_staggered_clocks(gpu, community):
    homes, weather = community
    refs = _singles3(community)
    fresh = _single(homes, weather, 9, STARTS[1], _prices()[1], 2)
    assert any(not torch.equal(x, y) for x, y in zip(fresh["hist"], refs[1]["hist"][:2]))     # the seed matters
    va = _vector(homes, weather, SEEDS, STARTS)
    P = torch.as_tensor(_prices(), dtype=torch.float64)
    for t in range(2):
        va.step(P)
    va.reset([False, True, False], seeds=[0, 9, 0])
    assert va.clocks_host() == [2, 0, 2]
    sl = slice(va.Nb, 2 * va.Nb)
    assert bool(torch.isnan(va.batch.vals[:, sl]).all()) and bool(torch.isnan(va.batch.fc_store[sl]).all())
    for k in range(2):
        # episode 1 sits at t = 0 and reads params while its neighbours read their hash arrays
        sums = va.step(P)
        _check_episode(va, 1, fresh, k, sums, "second life")
        _check_episode(va, 0, refs[0], 2 + k, sums)
        _check_episode(va, 2, refs[2], 2 + k, sums)
    assert va.clocks_host() == [4, 2, 4]
    _check_history(va, 1, fresh, 0, 2, "second life")
    _check_history(va, 0, refs[0], 0, T)
    _check_history(va, 2, refs[2], 0, T)


def test_idle_group_keeps_its_bits(gpu, community):
    homes, weather = community
    refs = _singles3(community)
    va = _vector(homes, weather, SEEDS, STARTS)
    P = torch.as_tensor(_prices(), dtype=torch.float64)
    va.step(P)
    b, Nb = va.batch, va.Nb
    sl = slice(Nb, 2 * Nb)
    va.park([1])                                     # the RL-priced episode
    before = [x.clone() for x in (_bits(b.vals[:, sl]), _bits(b.fc_store[sl]), b.status[sl], b.int_path[sl],
                                  b.iters[sl], _bits(b.obj[sl]), _bits(b.relax_obj[sl]))]
    sums = va.step(P)                                # (its history row is NaN-prefilled: va._row)
    after = (_bits(b.vals[:, sl]), _bits(b.fc_store[sl]), b.status[sl], b.int_path[sl], b.iters[sl],
             _bits(b.obj[sl]), _bits(b.relax_obj[sl]))
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert bool(torch.isnan(va._row[:, sl]).all()) and not bool(torch.isnan(va._row[:, :Nb]).all())
    _check_episode(va, 0, refs[0], 1, sums)
    _check_episode(va, 2, refs[2], 1, sums)
    assert va.clocks_host() == [2, 1, 2]
    va.resume([1])
    for k in range(2):                               # one step late, bit-identical
        sums = va.step(P)
        _check_episode(va, 1, refs[1], 1 + k, sums, "resumed")
        _check_episode(va, 0, refs[0], 2 + k, sums)
    assert va.clocks_host() == [4, 3, 4]
    _check_history(va, 1, refs[1], 0, 3, "resumed")
    _check_history(va, 2, refs[2], 0, T)


def test_one_episode_equals_a_plain_step_run(gpu, community):
    homes, weather = community
    ref = _single(homes, weather, SEEDS[1], STARTS[1], _prices()[1], 2)
    va = _vector(homes, weather, SEEDS[1:2], STARTS[1:2], steps=2)
    assert va.batch.dims.n_groups == 0 and va.batch.N == 16
    for t in range(2):
        sums = va.step(_prices()[1:2])
        _check_episode(va, 0, ref, t, sums)
    _check_history(va, 0, ref, 0, 2)


def test_odd_row_length(gpu, community):
    homes, weather = community
    va = _vector(homes[:13], weather, SEEDS, STARTS, steps=2)
    refs = [_single(homes[:13], weather, SEEDS[e], STARTS[e], _prices()[e], 2) for e in range(3)]
    for t in range(2):
        sums = va.step(_prices())
        for e in range(3):
            _check_episode(va, e, refs[e], t, sums)


def test_five_episodes_relax(gpu, community):
    homes, weather = community
    seeds, starts = (5, 6, 7, 8, 2 ** 40 + 7), (0, 7, 12, 3, 1)
    pr = np.concatenate([_prices(), _prices()[1:2] - 0.1, _prices()[:1] + 0.05])
    va = _vector(homes, weather, seeds, starts, steps=2, int_mode="relax")
    refs = [_single(homes, weather, seeds[e], starts[e], pr[e], 2, int_mode="relax") for e in range(5)]
    for t in range(2):
        sums = va.step(pr)
        for e in range(5):
            _check_episode(va, e, refs[e], t, sums)


@pytest.mark.parametrize("off,stride", [(0, 1), (3, 4)])
def test_season_noise_episodes(gpu, community, off, stride):
    from dragg_amd.mpc import MPCBatch
    homes, weather = community
    g = MPCBatch(homes[:13], *weather, 0, [0.0], groups=3, home_offset=off, home_stride=stride)
    dev = g.device
    clocks = (7, 0, 3)
    seeds = torch.tensor(SEEDS, dtype=torch.int64, device=dev)
    z = g.season_noise_episodes(seeds, torch.tensor(clocks, dtype=torch.int32, device=dev))
    for e in range(3):
        p = MPCBatch(homes[:13], *weather, 0, [0.0], seed=SEEDS[e], home_offset=off, home_stride=stride)
        assert torch.equal(_bits(z[:, e * 13:(e + 1) * 13]), _bits(p.season_noise(clocks[e]))), e
    # an idle group's columns are left as they are; no clocks: the shared timestep
    z2 = g.season_noise_episodes(seeds, torch.tensor((7, -1, 3), dtype=torch.int32, device=dev))
    assert bool(torch.isnan(z2[:, 13:26]).all()) and torch.equal(_bits(z2[:, :13]), _bits(z[:, :13]))
    z3 = g.season_noise_episodes(seeds, None, t=3)
    assert torch.equal(_bits(z3[:, 26:]), _bits(z[:, 26:]))


def test_arguments(gpu, community):
    from dragg_amd import _lib as L
    from dragg_amd.mpc import MPCBatch
    from dragg_amd.vector import VectorAggregator
    homes, weather = community
    oat, ghi, tou = weather
    lib = L.load()
    pr = _prices()
    a = MPCBatch(homes, oat, ghi, tou, 3, pr, seed=5, groups=3)
    b = MPCBatch(homes, oat, ghi, tou, 3, pr, seed=5, groups=3)
    stream = L.stream_ptr(None, a.device)
    prob, hsh, out = a._problem(), a._hash(), a._out()
    ep = L.Episodes()
    assert lib.dragg_mpc_step_episodes(a.dims, prob, None, hsh, out, 0, None, stream) == -1        # DRAGG_E_ARG
    d = L.Dims.from_buffer_copy(a.dims)
    d.n_groups = 5                                   # 48 homes
    assert lib.dragg_mpc_step_episodes(d, prob, ep, hsh, out, 0, None, stream) == -1
    assert lib.dragg_mpc_season_noise_episodes(a.dims, None, 0, 1, 0, None, stream) == -1
    assert lib.dragg_mpc_season_noise_episodes(d, ep, 0, 1, 0, None, stream) == -1
    assert lib.dragg_mpc_step_episodes(a.dims, prob, ep, hsh, out, -1, None, stream) == -1         # shared t < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(a.vals).all())           # nothing ran
    # an empty shard is a no-op
    d0 = L.Dims.from_buffer_copy(a.dims)
    d0.n_homes = 0
    assert lib.dragg_mpc_step_episodes(d0, prob, ep, hsh, out, 0, None, stream) == 0
    # NULL member arrays: the shared values, i.e. dragg_mpc_step on the grouped batch, bit for bit
    for t in range(2):
        a.step_episodes(None, None, None, t=t)
        b.step(t)
        assert torch.equal(_bits(a.vals), _bits(b.vals)) and torch.equal(_bits(a.fc_store), _bits(b.fc_store))
        assert torch.equal(a.status, b.status) and torch.equal(a.int_path, b.int_path)
        assert torch.equal(_bits(a.obj), _bits(b.obj))
    assert not bool(torch.isnan(a.vals[0]).any())
    # a group whose window leaves the environment lists is idle, not read out of bounds
    n_env = len(oat)
    far = torch.tensor([3, n_env - 10, 3], dtype=torch.int32, device=a.device)
    before = _bits(a.vals).clone()
    a.step_episodes(None, far, None, t=2)
    b.step(2)
    assert torch.equal(_bits(a.vals[:, 16:32]), before[:, 16:32])
    assert torch.equal(_bits(a.vals[:, :16]), _bits(b.vals[:, :16]))
    # the host refuses what it can see
    with pytest.raises(ValueError):
        a.step_episodes(torch.zeros(3, dtype=torch.int32, device=a.device), None, None)
    with pytest.raises(ValueError):
        a.step_episodes(None, None, torch.zeros(2, dtype=torch.int32, device=a.device))
    kw = dict(num_timesteps=T)
    with pytest.raises(ValueError):
        VectorAggregator(homes, oat, ghi, tou, 3, [1, 2], [0, 0, 0], **kw)
    with pytest.raises(ValueError):
        VectorAggregator(homes, oat, ghi, tou, 3, [1, 2, 3], [0, 0], **kw)
    with pytest.raises(ValueError):
        VectorAggregator(homes, oat, ghi, tou, 3, [1, 2, 3], [0, n_env - T - 24, 0], **kw)
    with pytest.raises(ValueError):
        VectorAggregator(homes, oat, ghi, tou, 3, [1, 2, 3], [0, 0, 0], world=2, **kw)
    va = VectorAggregator(homes, oat, ghi, tou, 3, [1, 2, 3], [0, n_env - T - 25, 0], **kw)
    with pytest.raises(ValueError):
        va.reset([True, False, False], start_indices=[n_env, 0, 0])
    with pytest.raises(ValueError):
        va.reset(seeds=[1, 2])
    va.reset([False, True, True], start_indices=[n_env, 0, 0])      # (an unmasked entry is not taken)
    assert va.starts.cpu().tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        va.step([0.0, 0.0])


def test_sub_steps_4(gpu):
    """S = 4: every chain goes to the exact step-function DP, whose list entries must carry the replica
    home indices (the second episode's homes are 16..31)."""
    from dragg_amd import _lib as L
    from dragg_amd.community import synthetic_homes, synthetic_weather
    homes = synthetic_homes(64, seed=5, days=2, dt=4, horizon_hours=6, sub_steps=4)[::4]
    weather = synthetic_weather(2, 4, 24, seed=5, month=MONTH)
    seeds, starts = (5, 6), (0, 7)
    refs = [_single(homes, weather, seeds[e], starts[e], [0.0], 2, key="S4") for e in range(2)]
    va = _vector(homes, weather, seeds, starts, steps=2)
    assert va.batch.S == 4
    for t in range(2):
        sums = va.step([0.0, 0.0])
        for e in range(2):
            _check_episode(va, e, refs[e], t, sums)
    b = va.batch
    steps = ((b.int_path & L.PATH_STEPS) != 0).nonzero().reshape(-1).cpu().tolist()
    assert any(h >= 16 for h in steps) and any(h < 16 for h in steps)
    lst, n = b.work_list("steps_list")
    assert 0 < n <= b.N
    assert sorted(set(int(x) & L.LIST_HOME_MASK for x in lst)) == steps
