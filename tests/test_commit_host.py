"""Playing a swept candidate, host side (CPU): the hold of `DeviceAggregator.sweep(hold=True)`, what voids it
and what `commit` files; `VectorAggregator.sweep` / `select` / `commit`; `rl.Candidate`, `Aggregator.rl_commit`
and the `rl_step` fallback of `run_rl_agg`; `SweepAgent(commit=...)`; the two new symbols of ABI v10.

The solver is a stand-in with state in the style of tests/test_vector_host.py's: a home's step depends on
everything it owns (previous state, seed, start index, clock, price), so a twin that solves the step the
ordinary way is a real reference for the adopted one."""
import json
import logging
import os
import re

import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from dragg_amd.aggregator import DeviceAggregator
from dragg_amd.rl import Candidate, SweepAgent, agent_policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")
CPU = torch.device("cpu")
ENV = [0.0] * 64


class HoldBatch:
    """Stand-in grouped batch with MPCBatch's surface: `step` / `step_episodes`, `replicate_from` (copy-major
    copies of a base that may itself be grouped), `adopt_from`, `select_groups`, the sums."""
    H = 4

    def __init__(self, homes, *a, home_offset=0, home_stride=1, device=None, groups=1, seed=0, **kw):
        self.groups, self.Nb = groups, len(homes)
        self.N, self.off, self.stride, self.seed = groups * len(homes), home_offset, home_stride, seed
        nan = float("nan")
        self.vals = torch.full((L.NVAL, self.N), nan, dtype=torch.float64)
        self.fc = torch.full((L.NFC, self.H, self.N), nan, dtype=torch.float64)
        self.status = torch.zeros(self.N, dtype=torch.int32)
        self.iters = torch.zeros(self.N, dtype=torch.int32)
        self.int_path = torch.zeros(self.N, dtype=torch.int32)
        self.obj = torch.zeros(self.N, dtype=torch.float64)
        self.rp = torch.zeros((groups, 1), dtype=torch.float64)
        self.hist_row = None
        self.solves = 0

    def set_reward_price(self, rp):
        self.rp = rp.clone().reshape(self.groups, -1)

    def step_episodes(self, seeds, starts, clocks, noise=None, hist=None, stream=None):
        self.solves += 1
        for g in range(self.groups):
            c = int(clocks[g])
            if c < 0:
                continue
            for i in range(self.Nb):
                r, k = g * self.Nb + i, self.off + i * self.stride
                prev = 0.0 if c == 0 else float(self.vals[0, r])
                p = float(self.rp[g, 0])
                v = prev + (k + 1) * (1 + p) * (c + 1) + 0.001 * int(seeds[g]) + int(starts[g])
                self.vals[0, r], self.vals[1, r], self.vals[L.K["cost_opt"], r] = v, 2 * v, v * p
                self.fc[0, 0, r] = v
                self.status[r] = L.ST_OPTIMAL if (k + c) % 3 else L.ST_MAX_ITER
                self.iters[r] = c + k
                self.obj[r] = -v
                self.int_path[r] = L.PATH_SECOND if p < 0 else 0
                if hist is not None:
                    hist[:, r] = self.vals[:, r]

    def step(self, t, noise=None, hist=None):
        G = self.groups
        self.step_episodes([self.seed] * G, [0] * G, [t] * G, hist=hist)

    def aggregate_groups(self, stream=None):
        v = self.vals.view(L.NVAL, self.groups, self.Nb)
        return torch.stack([v[0].sum(1), v[1].sum(1), v[L.K["cost_opt"]].sum(1)], dim=1)

    def aggregate(self):
        assert self.groups == 1
        return self.aggregate_groups()[0]

    def replicate_from(self, base, stream=None):
        C = self.N // base.N
        assert base.N * C == self.N
        self.vals.copy_(base.vals.repeat(1, C))
        self.fc.copy_(base.fc.repeat(1, 1, C))

    def adopt_from(self, src, choice, hist=None, stream=None):
        assert choice.dtype == torch.int32 and tuple(choice.shape) == (self.groups,)
        C, Nb = src.N // self.N, self.Nb
        for e, c in enumerate(choice.tolist()):
            if not 0 <= c < C:
                continue
            d, s = slice(e * Nb, (e + 1) * Nb), slice(c * self.N + e * Nb, c * self.N + (e + 1) * Nb)
            for k in ("vals", "fc", "status", "iters", "int_path", "obj"):
                getattr(self, k)[..., d] = getattr(src, k)[..., s]
            if hist is not None and src.hist_row is not None:
                hist[:, d] = src.hist_row[:, s]

    def select_groups(self, sums, target, prices, stream=None):
        E = self.groups
        sums, target, prices = (torch.as_tensor(np.asarray(x), dtype=torch.float64) for x in (sums, target, prices))
        C = sums.shape[0] // E
        out = []
        for e in range(E):
            ok = [c for c in range(C) if not torch.isnan(sums[c * E + e, 0])]
            out.append(min(ok, key=lambda c: (abs(float(sums[c * E + e, 0] - target[e])),
                                              abs(float(prices.reshape(C * E, -1)[c * E + e, 0])), c)) if ok else -1)
        return torch.tensor(out, dtype=torch.int32)


HOMES = [{"name": f"h{i}"} for i in range(5)]
PRICES = [[0.5], [-0.25], [0.125]]


def _agg(steps=2, **kw):
    agg = DeviceAggregator(HOMES, None, None, None, 0, 8, device=CPU, batch_cls=HoldBatch, seed=3, **kw)
    for _ in range(steps):
        agg.run_iteration()
        agg.collect_data()
    return agg


def _same(a, b):
    nn = lambda x: x.nan_to_num(-7.5)  # noqa: E731
    return (a.timestep == b.timestep and all(torch.equal(nn(getattr(a.batch, k)), nn(getattr(b.batch, k)))
                                             for k in ("vals", "fc", "obj", "rp"))
            and all(torch.equal(getattr(a.batch, k), getattr(b.batch, k)) for k in ("status", "iters", "int_path"))
            and torch.equal(nn(a.hist), nn(b.hist)) and torch.equal(a.agg_hist, b.agg_hist)
            and torch.equal(a.status_hist, b.status_hist) and torch.equal(a.path_hist, b.path_hist))


# ------------------------------------------------------------------ DeviceAggregator: hold, commit
@pytest.mark.parametrize("steps", [1, 2, 3])
def test_commit_equals_the_solved_step(steps):
    agg, twin = _agg(), _agg()
    plain = agg.sweep(PRICES, steps).clone()
    solves = agg.batch.solves
    sw = agg.sweep(PRICES, steps, hold=True)
    assert torch.equal(sw, plain) and agg.holds() and agg.holds(2) and not agg.holds(3) and not agg.holds(-1)
    # at steps == 1 the replica batch itself is the holder, else a clone taken before the replicas move on
    assert (agg._hold["src"] is agg._sweep_batches[3]) == (steps == 1)
    agg.commit(1)
    got = agg.collect_data().clone()
    assert agg.batch.solves == solves and not agg.holds()          # no solve of the live batch
    twin.set_reward_price(PRICES[1])
    twin.run_iteration()
    want = twin.collect_data().clone()
    assert torch.equal(got, want) and torch.equal(got, sw[1, 0]) and _same(agg, twin)
    assert int((agg.path_hist[2] == L.PATH_SECOND).sum()) == len(HOMES)
    assert agg.approx_counts() == twin.approx_counts() and agg.approx_counts()["later_launch_solves"] == len(HOMES)
    agg.run_iteration()
    twin.run_iteration()
    assert torch.equal(agg.collect_data(), twin.collect_data()) and _same(agg, twin)


def test_hold_is_voided_when_the_live_state_moves(tmp_path):
    agg = _agg()
    with pytest.raises(ValueError, match="no sweep is held"):
        agg.commit(0)
    agg.sweep(PRICES, 1)
    assert not agg.holds()
    with pytest.raises(ValueError, match="no sweep is held"):
        agg.commit(0)                                   # a sweep without hold=True holds nothing
    agg.sweep(PRICES, 1, hold=True)
    for g in (3, -1):
        with pytest.raises(ValueError, match="candidate"):
            agg.commit(g)
    assert agg.holds(0)                                 # (a refused g leaves the hold)
    before = agg.snapshot()
    moves = [lambda: agg.run_iteration(), lambda: agg.restore(agg.snapshot()), lambda: agg.forecast(1),
             lambda: agg.load_state(agg.save_state(str(tmp_path / "s.pt"))), lambda: agg.commit(0)]
    for move in moves:
        agg.sweep(PRICES, 1, hold=True)
        assert agg.holds(0)
        move()
        assert not agg.holds()
        with pytest.raises(ValueError):
            agg.commit(0)
    assert agg.timestep == before[0] + 2                # (run_iteration and the commit)
    # a later sweep without hold drops an earlier hold (it overwrites the replicas)
    agg.sweep(PRICES, 1, hold=True)
    agg.sweep(PRICES, 1)
    assert not agg.holds()
    # set_reward_price does not move the state
    agg.sweep(PRICES, 1, hold=True)
    agg.set_reward_price([0.75])
    assert agg.holds(2)
    agg.commit(2)
    assert agg.batch.rp.reshape(-1).tolist() == PRICES[2]
    # a sweep of no steps holds nothing
    agg.sweep(PRICES, 0, hold=True)
    assert not agg.holds()


def test_commit_is_refused_in_lag_mode():
    agg = _agg(steps=0)
    agg.overlap = True                                  # (the stand-in has no lag mode of its own)
    agg._hold = {"t": 0, "G": 1, "P": torch.zeros((1, 1)), "gen": agg._gen, "src": agg.batch}
    assert not agg.holds()
    with pytest.raises(ValueError, match="lag mode"):
        agg.commit(0)


# ------------------------------------------------------------------ VectorAggregator: sweep, select, commit
def _va(E=3, T=5):
    from dragg_amd.vector import VectorAggregator
    return VectorAggregator(HOMES[:3], ENV, ENV, ENV, E, [5, 6, 7], [0, 7, 12], T, device=CPU, batch_cls=HoldBatch)


def test_vector_sweep_select_commit_equals_step():
    va, twin = _va(), _va()
    first = [0.0, 0.5, -0.25]
    for v in (va, twin):
        v.park([0])
        v.step(first)
        v.step(first)
        v.resume([0])
        v.park([2])
    assert va.clocks_host() == [0, 2, 2]
    cands = np.array([[0.5, -0.5], [0.25, 0.0], [0.1, 0.2]])
    keep = va.batch.vals.clone()
    solves = va.batch.solves
    sums = va.sweep(cands)
    assert tuple(sums.shape) == (3, 2, 3) and va.batch.solves == solves
    assert torch.equal(va.batch.vals.nan_to_num(-1), keep.nan_to_num(-1))
    rb = va._sweep_batches[2]
    assert rb.groups == 6 and rb.rp[:, 0].tolist() == [0.5, 0.25, 0.1, -0.5, 0.0, 0.2]      # copy-major
    choice = va.select(sums, [0.0, 1e9, 5.0], cands)
    s = sums.numpy()
    want = [min(range(2), key=lambda c: (abs(s[e, c, 0] - sp), abs(cands[e, c]), c))
            for e, sp in enumerate([0.0, 1e9, 5.0])]
    assert choice.tolist() == want == [1, 0, 0]
    got = va.commit(choice)
    assert va.batch.solves == solves and va.adopted.tolist() == [True, True, False]
    ref = twin.step([cands[e, want[e]] for e in range(3)])
    assert torch.equal(got.nan_to_num(-1), ref.nan_to_num(-1)) and va.clocks_host() == twin.clocks_host() == [1, 3, 2]
    for e in range(2):
        assert torch.equal(sums[e, want[e]], got[e])
    nn = lambda x: x.nan_to_num(-7.5)  # noqa: E731
    for k in ("vals", "fc", "obj"):
        assert torch.equal(nn(getattr(va.batch, k)), nn(getattr(twin.batch, k))), k
    for k in ("status", "iters", "int_path"):
        assert torch.equal(getattr(va.batch, k), getattr(twin.batch, k)), k
    assert torch.equal(nn(va.hist), nn(twin.hist)) and torch.equal(va.agg_hist, twin.agg_hist)
    assert torch.equal(va.status_hist, twin.status_hist) and torch.equal(va.path_hist, twin.path_hist)
    assert va.batch.rp[:2, 0].tolist() == [-0.5, 0.25]
    # spent; voided by a step or a reset; -1 and C adopt nothing; an episode resumed after the sweep stays out
    with pytest.raises(ValueError):
        va.commit(choice)
    for move in (lambda: va.step(first), lambda: va.reset([1])):
        va.sweep(cands)
        move()
        with pytest.raises(ValueError):
            va.commit(choice)
    va.sweep(cands)
    va.resume([2])
    clocks = va.clocks_host()
    va.commit(torch.tensor([-1, 2, 0], dtype=torch.int32))
    assert va.adopted.tolist() == [False, False, False] and va.clocks_host() == clocks
    with pytest.raises(ValueError):
        va.sweep(np.zeros((2, 2)))
    va.sweep(cands)
    with pytest.raises(ValueError):
        va.commit(torch.zeros(3))                       # not an int tensor
    va.commit(torch.tensor([0, 1, 1]))                  # (any int dtype)
    assert va.adopted.tolist() == [True, True, True]


def test_vector_env_step_swept():
    from dragg_amd.rl import VectorEnv
    cfg = {"agg": {"rl": {"prev_timesteps": 3}}, "rl": {"utility": {"action_space": [-4, 4], "action_scale": 100}}}
    env, twin = (VectorEnv(_va(), cfg, max_poss_load=40.0) for _ in range(2))
    obs = env.reset()
    twin.reset()
    ag = SweepAgent(cfg, n_candidates=3)
    cands = ag.act_vector(obs)
    assert cands.shape == (3, 3) and cands[1].tolist() == pytest.approx([-0.04, 0.0, 0.04])
    env.park([1])
    twin.park([1])
    obs, done = env.step_swept(cands)
    assert env.choice[1] == -1 and all(0 <= c < 3 for c in env.choice[[0, 2]])
    obs2, _ = twin.step([cands[e, max(env.choice[e], 0)] for e in range(3)])
    assert obs["timestep"].tolist() == [1, 0, 1] and not done.any()
    for k in obs:
        assert np.array_equal(obs[k], obs2[k]), k


# ------------------------------------------------------------------ SweepAgent, Candidate
CFG = {"rl": {"utility": {"action_space": [-4, 4], "action_scale": 100}}}


class _SweepEnv:
    def __init__(self, load, setpoint):
        self.load, self.agg_setpoint, self.config, self.calls = load, setpoint, CFG, []

    def rl_sweep(self, prices, steps=None, **kw):
        self.calls.append(kw)
        out = np.zeros((len(prices), 1, 3))
        out[:, 0, 0] = [self.load(p) for p in prices]
        return out


def test_sweep_agent_returns_floats_unless_commit():
    env = _SweepEnv(lambda p: 100.0 - 1000.0 * p, setpoint=83.0)          # loads 140, 120, 100, 80, 60
    a = SweepAgent(CFG, n_candidates=5).act(env)
    assert type(a) is float and a == pytest.approx(0.02) and env.calls == [{}]     # (rl_sweep called as before)
    c = SweepAgent(CFG, n_candidates=5, commit=True).act(env)
    assert isinstance(c, Candidate) and c.index == 3 and c.price == a and env.calls[-1] == {"hold": True}
    assert tuple(c) == (3, a)

    class A:
        config = {"rl": {**CFG["rl"], "parameters": {"policy": "sweep", "candidates": 3}}}
    assert agent_policy(A).__self__.commit is False
    A.config = {"rl": {**CFG["rl"], "parameters": {"policy": "sweep", "commit": True}}}
    assert agent_policy(A).__self__.commit is True


# ------------------------------------------------------------------ the runner
def _runner(tmp_path, name):
    from dragg_amd.runner import Aggregator
    from tests import fixtures as F
    from tests.test_runner import _synthetic_data
    data = tmp_path / f"data_{name}"
    data.mkdir()
    _synthetic_data(str(data))
    params = dict(n=5, batt=1, pv=1, pvb=1, start="2015-01-01 00", end="2015-01-01 02", dt=4, horizon=1,
                  action_horizon=1, seed=3)
    with open(data / "config.toml", "w") as f:
        f.write(F.config_text(params))
    a = Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / f"outputs_{name}"), device=CPU, batch_cls=HoldBatch)
    a.checkpoint_interval, a.run_dir = 10 ** 9, str(tmp_path / f"run_{name}")
    return a


def test_run_rl_agg_plays_candidates(tmp_path, caplog):
    cands = [0.03, -0.02, 0.01]

    def policy(kind):
        def act(a):
            t = a.timestep
            if kind == "plain":
                a.rl_sweep(cands)
                return cands[t % 3]
            a.rl_sweep(cands, hold=True)
            if kind == "voided" and t % 2:
                a.dev.restore(a.dev.snapshot())         # the live state "moves": the hold is dropped
            return Candidate(t % 3, cands[t % 3])
        return act

    out, solves = {}, {}
    for kind in ("plain", "commit", "voided"):
        a = _runner(tmp_path, kind)
        with caplog.at_level(logging.WARNING, logger="dragg_amd.runner"):
            caplog.clear()
            path = a.run_rl_agg(policy(kind))
            warned = [r for r in caplog.records if "no longer held" in r.getMessage()]
        assert len(warned) == (1 if kind == "voided" else 0)              # logged once
        with open(path) as f:
            out[kind] = json.load(f)
        solves[kind] = a.dev.batch.solves
        T = a.num_timesteps
        assert T == 8 and a.timestep == a.dev.timestep == T
        assert a.all_rps.tolist() == [cands[t % 3] for t in range(T)]
    assert solves == {"plain": 8, "commit": 0, "voided": 4}
    for kind in ("commit", "voided"):
        for k in out["plain"]:
            if k == "Summary":
                assert {s: v for s, v in out[kind][k].items() if s != "solve_time"} == \
                    {s: v for s, v in out["plain"][k].items() if s != "solve_time"}
            else:
                assert out[kind][k] == out["plain"][k], (kind, k)


def test_rl_commit_refuses_without_changing_anything(tmp_path):
    a = _runner(tmp_path, "x")
    a.case = "rl_agg"
    a.get_homes()
    a.setup_rl_agg_run()
    a.rl_step(0.01)
    before, rps = a.reward_price.copy(), a.all_rps.copy()
    with pytest.raises(ValueError):
        a.rl_commit(0)                                  # nothing held
    sw = a.rl_sweep([0.3, -0.1], steps=2, hold=True)
    with pytest.raises(ValueError):
        a.rl_commit(2)
    assert np.array_equal(a.reward_price, before) and np.array_equal(a.all_rps, rps) and a.timestep == 1
    agg = a.rl_commit(1)
    assert agg == sw[1, 0].tolist() and a.timestep == a.dev.timestep == 2
    assert a.reward_price.tolist() == [-0.1] * 4 and a.all_rps[1] == -0.1
    assert a.dev.batch.rp.reshape(-1).tolist() == [-0.1] * 4
    assert a.agg_load == sw[1, 0, 0] and a.baseline_agg_load_list[-1] == a.agg_load


# ------------------------------------------------------------------ ABI v10, additive
def test_new_symbols_are_declared_and_exported_under_v10():
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    for n in ("dragg_mpc_adopt", "dragg_mpc_select_groups"):
        assert n in names and n in L.EXPORTS, n
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and L.ABI_VERSION == 10
    assert set(names) == set(L.EXPORTS)
