"""Lookahead sweeps, host side (CPU): the ABI surface of dragg_mpc_select_paths, its numpy restatement
(`vector.select_paths_reference`) against the one-step rule and against the setpoints the environment files when
the loads are really played, `VectorAggregator.sweep(steps=K)` / `select_paths` / `commit` and the two vector
environments' `step_swept(lookahead=K)` on a stand-in batch, and `SweepAgent(lookahead, discount)`."""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from dragg_amd.rl import SweepAgent, agent_policy
from tests.test_commit_host import CFG, CPU, ENV, HOMES, HoldBatch, _SweepEnv
from tests.test_env_host import _bits, _cfg, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")


class AheadBatch(HoldBatch):
    """The stand-in grouped batch with the calls a lookahead sweep adds, served by the restatements."""

    def aggregate_groups(self, stream=None, out=None):
        agg = super().aggregate_groups()
        if out is None:
            return agg
        out.copy_(agg)
        return out

    def select_paths(self, sums, ran, tracked, target, weights, prices, num_timesteps, fresh_load, score=None,
                     stream=None):
        from dragg_amd.vector import select_paths_reference
        keep = [x.clone() for x in (sums, ran, tracked, target, weights, prices)]
        choice, sc = select_paths_reference(sums.numpy(), ran.numpy(), tracked.numpy(), target.numpy(), weights.numpy(),
                                            prices.numpy(), num_timesteps, 2.0 * fresh_load)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(keep, (sums, ran, tracked, target, weights, prices)))
        if score is not None:
            score.copy_(torch.as_tensor(sc))
        return torch.as_tensor(choice)

    def env_file(self, st, ran, sums, hist=None, stream=None):
        from dragg_amd.vector import env_file_reference
        env_file_reference(st.host(), ran.numpy(), sums.numpy(), self.status.numpy(), self.int_path.numpy(),
                           None if hist is None else hist.numpy())

    def env_reset(self, st, mask, stream=None):
        from dragg_amd.vector import env_reset_reference
        env_reset_reference(st.host(), mask.numpy(), self.vals.numpy(), self.fc.permute(2, 0, 1).numpy())


def _va(E, T, seeds=None, starts=None):
    from dragg_amd.vector import VectorAggregator
    return VectorAggregator(HOMES[:3], ENV, ENV, ENV, E, seeds or list(range(5, 5 + E)), starts or [0, 7, 12, 3][:E], T,
                            device=CPU, batch_cls=AheadBatch)


# ------------------------------------------------------------------ ABI surface
def test_abi_surface_of_the_path_selection(tmp_path):
    from dragg_amd import build
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    assert "dragg_mpc_select_paths" in names and "dragg_mpc_select_paths" in L.EXPORTS
    assert "typedef struct dragg_mpc_paths" in h
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and L.ABI_VERSION == 10
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "dragg_mpc_select_paths") and lib.dragg_mpc_abi_version() == 10
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(dragg_mpc_paths));']
    for f, _ in L.Paths._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(dragg_mpc_paths, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.Paths) == 96
    assert [f for f, _ in L.Paths._fields_] == ["steps", "num_timesteps", "prev_timesteps", "fresh_load", "sums", "ran",
                                                "tracked", "target", "weights", "prices", "n_rp", "choice", "score"]
    for f, _ in L.Paths._fields_:
        assert int(got[f]) == getattr(L.Paths, f).offset, f
    L.load()                                              # (the argtypes bind against the built library)
    assert L.load().dragg_mpc_select_paths.argtypes[2]._type_ is L.Paths


# ------------------------------------------------------------------ K = 1 is the existing rule
def test_one_step_with_unit_weight_is_the_existing_select_rule():
    from dragg_amd.vector import select_paths_reference
    rng = np.random.default_rng(14)
    E, C, T, P = 9, 6, 5, 4
    rule = HoldBatch(HOMES[:1], groups=E)
    for trial in range(30):
        sums = rng.uniform(0.0, 40.0, (C * E, 3))
        target = rng.uniform(5.0, 30.0, E)
        prices = rng.choice([-0.5, -0.25, 0.0, 0.25, 0.5], (C * E, 2))
        # injected ties (equal distance either side of the target, equal |price| too) and NaNs (episode 3: all)
        target[1] = 16.0
        sums[np.arange(C) * E + 1, 0] = 30.0 + np.arange(C)
        sums[0 * E + 1, 0], sums[1 * E + 1, 0], sums[2 * E + 1, 0] = 14.0, 18.0, 18.0
        prices[0 * E + 1, 0], prices[1 * E + 1, 0], prices[2 * E + 1, 0] = 0.5, -0.25, 0.25
        sums[rng.integers(0, C) * E + 2, 0] = np.nan
        sums[np.arange(C) * E + 3, 0] = np.nan
        sums[np.arange(C) * E + 4, 0] = target[4]                          # all tie: the price, then the index, decides
        want = rule.select_groups(sums, target, prices).tolist()
        choice, score = select_paths_reference(sums[None], rng.integers(0, T, E), rng.uniform(0, 40, (E, P)), target,
                                               [1.0], prices, T, 37.0)
        assert choice.tolist() == want, trial
        assert want[3] == -1 and want[1] == 1
        d = np.abs(sums[:, 0] - np.tile(target, C))
        assert _bits(score).tolist() == _bits(d).tolist()                  # (0.0 + 1.0 * d is d; NaN where no load)


# ------------------------------------------------------------------ the setpoints are the environment's
def _fresh_env(E, T, P, max_poss):
    fresh = np.full((E, P), 0.5 * max_poss)
    obs = np.zeros((len(L.OBS_KEYS), E))
    obs[3] = [np.average(fresh[e]) for e in range(E)]
    return {"num_timesteps": T, "prev_timesteps": P, "max_poss_load": max_poss, "start_load": 9.0,
            "clock": np.zeros(E, dtype=np.int32), "tracked": fresh, "max_load": np.full(E, -np.inf),
            "min_load": np.full(E, np.inf), "obs": obs, "status_hist": None, "path_hist": None, "hist": None,
            "agg_hist": None}


@pytest.mark.parametrize("P", [1, 7, 8, 9, 12, 128])
def test_reference_setpoints_equal_the_filed_ones(P):
    """Episodes at clock 0, 1, 5 and T - 2: the s_j the restatement scores against are, bit for bit, the setpoints
    `env_file_reference` (`VectorEnv`'s bookkeeping: tests/test_env_host.py) files when the candidate's loads are
    played, and the score is the sum the contract writes."""
    from dragg_amd.vector import env_file_reference, select_paths_reference
    rng = np.random.default_rng(200 + P)
    E, C, K, T, mp = 4, 3, 5, 12, 37.3
    env = _fresh_env(E, T, P, mp)
    for t in range(T - 2):                                   # episode e is brought to clock [0, 1, 5, T - 2][e]
        ran = np.array([t if t < stop else -1 for stop in (0, 1, 5, T - 2)], dtype=np.int32)
        env_file_reference(env, ran, rng.uniform(0.0, 40.0, (E, 3)))
    assert env["clock"].tolist() == [0, 1, 5, T - 2]
    sums = rng.uniform(0.0, 40.0, (K, C * E, 3))
    w = rng.uniform(0.1, 1.0, K)
    before = copy.deepcopy(env)
    sps = {}
    choice, score = select_paths_reference(sums, env["clock"], env["tracked"], env["obs"][3], w,
                                           rng.uniform(-1, 1, (C * E, 1)), T, mp, setpoints=sps)
    assert all(np.array_equal(before[k], env[k]) for k in ("tracked", "obs", "clock", "max_load"))
    for e in range(E):
        k = min(K, T - int(env["clock"][e]))
        assert k == (2 if e == 3 else K)
        for c in range(C):
            played = copy.deepcopy(env)
            filed = [float(played["obs"][3][e])]
            for j in range(k - 1):
                ran = np.full(E, -1, dtype=np.int32)
                ran[e] = played["clock"][e]
                step = np.zeros((E, 3))
                step[e] = sums[j, c * E + e]
                env_file_reference(played, ran, step)
                filed.append(float(played["obs"][3][e]))
            assert _bits(np.array(sps[(e, c)])).tolist() == _bits(np.array(filed)).tolist(), (e, c)
            acc = np.float64(0.0)
            for j in range(k):
                acc = acc + w[j] * np.abs(sums[j, c * E + e, 0] - np.float64(filed[j]))
            assert _bits(score[c * E + e:c * E + e + 1]).tolist() == _bits(np.array([acc])).tolist(), (e, c)
        assert choice[e] == min(range(C), key=lambda c: (score[c * E + e], c))


# ------------------------------------------------------------------ looking ahead changes the decision
def test_lookahead_changes_the_decision():
    """Candidate 0 hits the setpoint now and rebounds; candidate 1 is a little off now and stays close."""
    from dragg_amd.vector import select_paths_reference
    T, P, mp = 10, 4, 40.0
    tracked, target = np.full((1, P), 20.0), [20.0]
    sums = np.zeros((3, 2, 3))
    sums[:, 0, 0] = [20.0, 31.0, 33.0]
    sums[:, 1, 0] = [21.0, 20.5, 20.5]
    prices = [[0.3], [0.1]]
    one, _ = select_paths_reference(sums[:1], [4], tracked, target, [1.0], prices, T, mp)
    three, score = select_paths_reference(sums, [4], tracked, target, [1.0, 1.0, 1.0], prices, T, mp)
    assert one.tolist() == [0] and three.tolist() == [1] and score[1] < score[0]
    # an episode with one step left sees one step, whatever K is; a finished or idle one chooses nothing
    last, _ = select_paths_reference(sums, [T - 1], tracked, target, [1.0, 1.0, 1.0], prices, T, mp)
    none, sc = select_paths_reference(sums, [T], tracked, target, [1.0, 1.0, 1.0], prices, T, mp)
    idle, _ = select_paths_reference(sums, [-1], tracked, target, [1.0, 1.0, 1.0], prices, T, mp)
    assert last.tolist() == [0] and none.tolist() == idle.tolist() == [-1] and np.isnan(sc).all()
    # a NaN load past the steps an episode has left is not read, one before invalidates its candidate
    sums[2, 1, 0] = np.nan
    assert select_paths_reference(sums, [T - 2], tracked, target, [1.0, 1.0, 1.0], prices, T, mp)[0].tolist() == [1]
    assert select_paths_reference(sums, [4], tracked, target, [1.0, 1.0, 1.0], prices, T, mp)[0].tolist() == [0]


# ------------------------------------------------------------------ the aggregator's rollout on a stand-in
def test_vector_sweep_of_k_steps_and_commit_from_the_held_first_step():
    E, T, C, K = 4, 6, 3, 3
    va, twin = _va(E, T), _va(E, T)
    first = [0.0, 0.5, -0.25, 0.1]
    for v in (va, twin):
        v.park([1, 3])
        for _ in range(4):
            v.step(first)
        v.resume([1])
    assert va.clocks_host() == [4, 0, 4, 0]
    cands = np.array([[0.5, -0.5, 0.1], [0.25, 0.0, -0.1], [0.1, 0.2, 0.3], [0.0, 0.1, 0.2]])
    keep = {k: getattr(va.batch, k).clone() for k in ("vals", "fc", "status", "iters", "obj")}
    solves = va.batch.solves
    one = va.sweep(cands).clone()
    paths = va.sweep(cands, steps=K)
    assert tuple(paths.shape) == (E, C, K, 3) and va.batch.solves == solves
    assert all(torch.equal(_bits(getattr(va.batch, k)), _bits(v)) for k, v in keep.items())
    assert va.sweep_steps.tolist() == [2, 3, 2, 0] and va.sweep_steps.dtype == torch.int32
    assert torch.equal(_bits(paths[:, :, 0]), _bits(one))
    for e in range(E):
        k = int(va.sweep_steps[e])
        for c in range(C):
            t = _va(E, T)                                        # a twin brought to the same state, then stepped on
            t.park([1, 3])
            for _ in range(4):
                t.step(first)
            t.resume([1])
            for j in range(k):
                got = t.step(cands[:, c])
                assert _bits(paths[e, c, j]).tolist() == _bits(got[e]).tolist(), (e, c, j)
            for j in range(max(k, 1), K):
                assert _bits(paths[e, c, j]).tolist() == _bits(paths[e, c, max(k, 1) - 1]).tolist(), (e, c, j)
    held = va._hold["src"]
    assert held is not va._sweep_batches[C] and held is va._held[C]
    ptrs = [getattr(held, k).data_ptr() for k in ("vals", "fc", "status", "iters", "int_path", "obj")]
    buf = va._path_sums[(C, K)].data_ptr()
    choice = torch.tensor([2, 0, 1, 1], dtype=torch.int32)
    got = va.commit(choice)
    assert va.batch.solves == solves and va.adopted.tolist() == [True, True, True, False]
    ref = twin.step([cands[e, int(choice[e])] for e in range(E)])
    assert torch.equal(_bits(got), _bits(ref)) and va.clocks_host() == twin.clocks_host() == [5, 1, 5, 0]
    for k in ("vals", "fc", "obj", "status", "iters", "int_path"):
        assert torch.equal(_bits(getattr(va.batch, k)), _bits(getattr(twin.batch, k))), k
    for k in ("hist", "agg_hist", "status_hist", "path_hist"):
        assert torch.equal(_bits(getattr(va, k)), _bits(getattr(twin, k))), k
    # a second sweep at the same C and K reuses the held buffers and the sums
    va.sweep(cands, steps=K)
    assert [getattr(va._held[C], k).data_ptr() for k in ("vals", "fc", "status", "iters", "int_path", "obj")] == ptrs
    assert va._path_sums[(C, K)].data_ptr() == buf and va.sweep_steps.tolist() == [1, 3, 1, 0]
    # hold=False keeps nothing; steps < 1 is refused
    va.sweep(cands, steps=2, hold=False)
    with pytest.raises(ValueError):
        va.commit(choice)
    with pytest.raises(ValueError, match="steps"):
        va.sweep(cands, steps=0)


# ------------------------------------------------------------------ host environment against device environment
def test_step_swept_with_lookahead_host_against_device_env_on_a_stand_in():
    """E = 4, T = 6, lookahead 3: episodes 0 and 2 two steps from their end, episode 3 parked; observations,
    choices, scores, clocks and stores equal at every step, and equal to a twin that plays the chosen prices."""
    from dragg_amd.rl import DeviceVectorEnv, VectorEnv
    E, T, K = 4, 6, 3
    cfg = _cfg(3)
    host, twin = (VectorEnv(_va(E, T), cfg, max_poss_load=40.0) for _ in range(2))
    dev = DeviceVectorEnv(_va(E, T), cfg, max_poss_load=40.0)
    for env in (host, twin, dev):
        env.reset()
        env.park([1, 3])
        for _ in range(4):
            env.step([0.0, 0.5, -0.25, 0.1])
        env.resume([1])
    _same(host, dev, "before")
    agent = SweepAgent(cfg, n_candidates=3, lookahead=K, discount=0.5)
    assert agent.weights() == [1.0, 0.5, 0.25]
    obs_h, obs_d = host.observations(), dev.observations()
    steps = 0
    while not host.done()[:3].all():
        c_h, c_d = agent.act_vector(obs_h), agent.act_device(obs_d)
        obs_h, _ = host.step_swept(c_h, lookahead=agent.lookahead, weights=agent.weights())
        obs_d, _ = dev.step_swept(c_d, lookahead=agent.lookahead, weights=agent.weights())
        assert torch.is_tensor(dev.choice) and dev.choice.dtype == torch.int32 and torch.is_tensor(dev.scores)
        assert dev.choice.tolist() == host.choice.tolist() and host.choice[3] == -1
        assert tuple(dev.scores.shape) == host.scores.shape == (E, 3)
        assert _bits(dev.scores).tolist() == _bits(host.scores).tolist()
        assert np.isnan(host.scores[3]).all() and np.isnan(host.scores[host.choice < 0]).all()
        _same(host, dev, steps)
        twin.step([c_h[e, max(host.choice[e], 0)] for e in range(E)])
        for k, v in twin.observations().items():
            assert np.array_equal(v, obs_h[k]), (steps, k)
        steps += 1
        assert steps < 10
    assert steps == 6 and host.va.clocks_host() == [T, T, T, 0]
    assert len(dev._w) == 1                                   # (the host weights were uploaded once)
    # lookahead=1 takes the one-step path: no scores are written
    host.reset()
    dev.reset()
    before = dev.scores
    host.step_swept(c_h)
    dev.step_swept(c_d)
    assert dev.scores is before
    _same(host, dev, "lookahead 1")


# ------------------------------------------------------------------ SweepAgent
class _AheadEnv(_SweepEnv):
    """The runner's surface a lookahead `SweepAgent.train` reads."""
    timestep, num_timesteps, max_poss_load = 4, 10, 40.0
    tracked_loads = [20.0] * 4

    def rl_sweep(self, prices, steps=None, **kw):
        self.calls.append(dict(kw, steps=steps))
        k = min(steps, self.num_timesteps - self.timestep)
        out = np.zeros((len(prices), k, 3))
        for j in range(k):
            out[:, j, 0] = [self.load(p, j) for p in prices]
        return out


def test_sweep_agent_defaults_are_unchanged_and_lookahead_is_read():
    env = _SweepEnv(lambda p: 100.0 - 1000.0 * p, setpoint=83.0)
    a, b = SweepAgent(CFG, n_candidates=5), SweepAgent(CFG, n_candidates=5, lookahead=1, discount=0.3)
    assert [a.act(env) for _ in range(3)] == [b.act(env) for _ in range(3)] and a.history == b.history
    assert sorted(b.history) == ["action", "candidates", "response"] and env.calls == [{}] * 6
    assert b.weights() == [1.0] and SweepAgent(CFG, lookahead=3, discount=0.5).weights() == [1.0, 0.5, 0.25]

    class A:
        config = {"rl": {**CFG["rl"], "parameters": {"policy": "sweep"}}}
    assert (agent_policy(A).__self__.lookahead, agent_policy(A).__self__.discount) == (1, 1.0)
    A.config = {"rl": {**CFG["rl"], "parameters": {"policy": "sweep", "lookahead": 4, "discount": 0.9, "commit": True}}}
    ag = agent_policy(A).__self__
    assert (ag.lookahead, ag.discount, ag.commit) == (4, 0.9, True)
    # the single-community path: the price that hits the setpoint now rebounds, the zero price stays close
    table = {-0.04: [5.0, 5.0, 5.0], 0.0: [21.0, 20.5, 20.5], 0.04: [20.0, 31.0, 33.0]}
    ahead = _AheadEnv(lambda p, j: table[round(p, 2)][j], setpoint=20.0)
    near, far = SweepAgent(CFG, n_candidates=3), SweepAgent(CFG, n_candidates=3, lookahead=3, commit=True)
    p1 = near.act(_SweepEnv(lambda p: ahead.load(p, 0), setpoint=20.0))
    c3 = far.act(ahead)
    assert ahead.calls == [{"steps": 3, "hold": True}] and len(far.history["score"][0]) == 3
    assert p1 == pytest.approx(0.04) and c3.index == 1 and c3.price == 0.0
    assert far.history["response"][0] == [ahead.load(p, 0) for p in (-0.04, 0.0, 0.04)]


def test_run_rl_agg_with_a_lookahead_sweep_agent(tmp_path):
    """The runner's own loop (stand-in solver): a lookahead agent that commits solves nothing on the live batch
    and leaves the results of the same agent playing its choices the ordinary way; the last steps of the run are
    scored over the steps that are left."""
    import json
    from tests.test_commit_host import _runner
    out, agents = {}, {}
    for kind in ("plain", "commit"):
        a = _runner(tmp_path, kind)
        agents[kind] = ag = SweepAgent(CFG, n_candidates=3, commit=kind == "commit", lookahead=3, discount=0.5)
        with open(a.run_rl_agg(ag.act)) as f:
            out[kind] = json.load(f)
        assert a.num_timesteps == a.timestep == 8 and len(ag.history["score"]) == 8
        assert a.dev.batch.solves == (0 if kind == "commit" else 8)
    assert agents["plain"].history == agents["commit"].history
    assert all(len(s) == 3 and not np.isnan(s).any() for s in agents["plain"].history["score"])
    for k in out["plain"]:
        if k == "Summary":
            assert {s: v for s, v in out["commit"][k].items() if s != "solve_time"} == \
                {s: v for s, v in out["plain"][k].items() if s != "solve_time"}
        else:
            assert out["commit"][k] == out["plain"][k], k
