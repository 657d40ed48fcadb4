"""Vectorised episodes, host side (CPU): the ABI surface of dragg_mpc_step_episodes /
dragg_mpc_season_noise_episodes, and the glue on top of them -- `vector.VectorAggregator` (clocks, reset,
park, resume, done, history bookkeeping, error naming), `rl.VectorEnv` (per-episode setpoints),
`SetpointAgent.train_vector` and `runner.Aggregator.rl_vector` -- with a stand-in batch with state in the
style of tests/test_sweep_host.py's, whose step depends on everything an episode owns (seed, start index,
clock, price row, previous state).  The runner's `gen_setpoint` is pinned on a recorded sequence of loads."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from dragg_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")

CPU = torch.device("cpu")
HOMES = [{"name": f"home-{i}"} for i in range(3)]
ENV = [0.0] * 64
BAD_SEED = 666          # the stand-in's home 1 hits ERR_MISSING at clock 2 under this seed


def _home_step(prev, seed, start, clock, price, i):
    """The stand-in's closed loop for one home: the new vals[0] from everything the episode owns."""
    prev = 0.0 if clock == 0 else prev
    return prev + (i + 1) * (1 + price) * (clock + 1) + 0.001 * seed + start


class VecBatch:
    """Stand-in grouped batch: E replicas of the homes, `step_episodes` with MPCBatch's signature."""
    H = 4

    def __init__(self, homes, *a, device=None, groups=1, **kw):
        self.groups, self.Nb = groups, len(homes)
        self.N = groups * len(homes)
        self.vals = torch.full((L.NVAL, self.N), float("nan"), dtype=torch.float64)
        self.fc = torch.full((L.NFC, self.H, self.N), float("nan"), dtype=torch.float64)
        self.status = torch.zeros(self.N, dtype=torch.int32)
        self.int_path = torch.zeros(self.N, dtype=torch.int32)
        self.rp = torch.zeros((groups, 1), dtype=torch.float64)
        self.calls = []

    def set_reward_price(self, rp):
        self.rp = rp.clone().reshape(self.groups, -1)

    def step_episodes(self, seeds, starts, clocks, noise=None, hist=None, stream=None):
        assert seeds.dtype == torch.int64 and starts.dtype == torch.int32 and clocks.dtype == torch.int32
        self.calls.append(clocks.tolist())
        for g in range(self.groups):
            c = int(clocks[g])
            if c < 0:                                   # idle: nothing of the group is written
                continue
            for i in range(self.Nb):
                r = g * self.Nb + i
                v = _home_step(float(self.vals[0, r]), int(seeds[g]), int(starts[g]), c, float(self.rp[g, 0]), i)
                self.vals[0, r] = v
                self.vals[1, r] = 2 * v
                self.vals[L.K["cost_opt"], r] = v * float(self.rp[g, 0])
                self.fc[0, 0, r] = v
                bad = int(seeds[g]) == BAD_SEED and c == 2 and i == 1
                self.status[r] = L.ST_ERR_MISSING if bad else L.ST_OPTIMAL
                self.int_path[r] = L.PATH_SECOND if i == 0 else 0
                if hist is not None:
                    hist[:, r] = self.vals[:, r]

    def aggregate_groups(self, stream=None):
        v = self.vals.view(L.NVAL, self.groups, self.Nb)
        return torch.stack([v[0].sum(1), v[1].sum(1), v[L.K["cost_opt"]].sum(1)], dim=1)


def _single_run(seed, start, prices):
    """Episode as a single run: per step the homes' vals[0] and the three sums."""
    v, out = [0.0] * len(HOMES), []
    for t, p in enumerate(prices):
        v = [_home_step(v[i], seed, start, t, p, i) for i in range(len(HOMES))]
        out.append((list(v), [sum(v), sum(2 * x for x in v), sum(x * p for x in v)]))
    return out


def _va(E, seeds, starts, T=5, **kw):
    from dragg_amd.vector import VectorAggregator
    return VectorAggregator(HOMES, ENV, ENV, ENV, E, seeds, starts, T, device=CPU, batch_cls=VecBatch, **kw)


# ------------------------------------------------------------------ ABI surface
def test_abi_surface_of_the_episode_entry_points(tmp_path):
    from dragg_amd import build
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    new = ["dragg_mpc_step_episodes", "dragg_mpc_season_noise_episodes"]
    assert all(n in names and n in L.EXPORTS for n in new)
    assert "typedef struct dragg_mpc_episodes" in h
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and L.ABI_VERSION == 10
    assert [f for f, _ in L.Dims._fields_][-1] == "n_groups" and [f for f, _ in L.Problem._fields_][-1] == "reserved"
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, n) for n in new) and lib.dragg_mpc_abi_version() == 10
    # sizeof / offsetof of the new struct, from gcc, against the ctypes mirror
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(dragg_mpc_episodes));']
    for f, _ in L.Episodes._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(dragg_mpc_episodes, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.Episodes) == 24
    assert [f for f, _ in L.Episodes._fields_] == ["seed", "start_index", "timestep"]
    for f, _ in L.Episodes._fields_:
        assert int(got[f]) == getattr(L.Episodes, f).offset, f


# ------------------------------------------------------------------ VectorAggregator
def test_episodes_equal_single_runs_with_staggered_clocks_and_parking():
    seeds, starts = [5, 6, 2 ** 63 + 7], [0, 7, 12]
    va = _va(3, seeds, starts)
    assert va.seeds.tolist() == [5, 6, 7 - 2 ** 63]          # (a uint64 seed keeps its bits)
    prices = [[0.0, 0.5, -0.25], [0.1, 0.5, -0.25], [0.2, 0.4, 0.0], [0.3, 0.5, 0.25], [0.0, 0.0, 0.0],
              [0.1, 0.2, 0.3], [0.5, 0.5, 0.5]]
    refs = [_single_run(7 - 2 ** 63 if e == 2 else seeds[e], starts[e], [p[e] for p in prices[:5]]) for e in range(3)]
    out = va.step(prices[0])
    assert tuple(out.shape) == (3, 3) and va.clocks_host() == [1, 1, 1]
    for e in range(3):
        assert out[e].tolist() == refs[e][0][1]
    # park episode 1 for a step: its columns and rows keep their values, it resumes one step late
    va.park([1])
    keep = va.batch.vals[:, 3:6].clone()
    va.step(prices[1])
    assert va.batch.calls[-1] == [1, -1, 1] and va.clocks_host() == [2, 1, 2]
    assert torch.equal(va.batch.vals[:, 3:6].nan_to_num(-1), keep.nan_to_num(-1))
    va.resume([1])
    # reset episode 2 alone with a new seed: clock 0, NaN columns, cleared rows; the others go on
    va.reset([False, False, True], seeds=[0, 0, 9])
    assert va.clocks_host() == [2, 1, 0] and va.seeds.tolist() == [5, 6, 9]
    assert bool(torch.isnan(va.batch.vals[:, 6:9]).all()) and bool(torch.isnan(va.batch.fc[:, :, 6:9]).all())
    assert not bool(torch.isnan(va.batch.vals[0, :6]).any())
    assert bool(torch.isnan(va.hist[:, :, 6:9]).all()) and int(va.status_hist[:, 6:9].abs().sum()) == 0
    assert va.episode_history(2).shape[0] == 0
    second = _single_run(9, 12, [p[2] for p in prices[2:]])
    ep1 = _single_run(6, 7, [prices[0][1]] + [p[1] for p in prices[2:6]])
    for k, p in enumerate(prices[2:5]):
        out = va.step(p)
        assert out[2].tolist() == second[k][1] and out[0].tolist() == refs[0][2 + k][1]
        assert out[1].tolist() == ep1[1 + k][1]
    assert va.clocks_host() == [5, 4, 3] and va.done().tolist() == [True, False, False]
    assert va.active().tolist() == [False, True, True]
    # a done episode sits idle: its clock stays, its rows stay
    out = va.step(prices[5])
    assert va.batch.calls[-1] == [-1, 4, 3] and va.clocks_host() == [5, 5, 4]
    assert out[0].tolist() == refs[0][4][1]                  # (an idle episode's sums: its last step's)
    # history bookkeeping: every episode's rows by its own clock
    for e, ref in ((0, refs[0]), (1, ep1), (2, second)):
        h, n = va.episode_history(e), va.clocks_host()[e]
        assert tuple(h.shape) == (n, L.NVAL, 3)
        assert [h[t, 0].tolist() for t in range(n)] == [ref[t][0] for t in range(n)]
        assert va.episode_sums(e).tolist() == [ref[t][1] for t in range(n)]
        assert tuple(va.episode_status(e).shape) == (n, 3) and tuple(va.episode_paths(e).shape) == (n, 3)
    assert va.approx_counts() == {"approx_solves": [0, 0, 0], "step_dp_solves": [0, 0, 0],
                                  "later_launch_solves": [5, 5, 4]}
    assert va.status_counts()["optimal"] == 3 * 14
    va.check_errors()
    # reset everything: a new batch's state
    va.reset()
    assert va.clocks_host() == [0, 0, 0] and bool(torch.isnan(va.batch.vals).all()) and bool(torch.isnan(va.hist).all())
    assert float(va.agg_hist.abs().sum()) == 0.0
    assert va.step([[0.0], [0.5], [-0.25]])[0].tolist() == refs[0][0][1]      # prices [E][1] too


def test_check_errors_names_episode_timestep_and_home():
    va = _va(2, [1, BAD_SEED], [0, 0])
    for _ in range(2):
        va.step([0.0, 0.0])
    va.check_errors()
    va.step([0.0, 0.0])
    with pytest.raises(KeyError, match=r"episode 1, home home-1 at timestep 2: err_missing"):
        va.check_errors()
    va.reset([1], seeds=[0, 3])                              # the rows of the failed life are cleared
    va.check_errors()


def test_constructor_and_reset_refuse_bad_keys():
    with pytest.raises(ValueError, match="seeds"):
        _va(3, [1, 2], [0, 0, 0])
    with pytest.raises(ValueError, match="start_indices"):
        _va(3, [1, 2, 3], [0, 0])
    # start + num_timesteps + H >= n_env (64 entries, T = 5, H = 4)
    with pytest.raises(ValueError, match="start index 55"):
        _va(3, [1, 2, 3], [0, 55, 0])
    with pytest.raises(ValueError, match="start index -1"):
        _va(3, [1, 2, 3], [0, -1, 0])
    with pytest.raises(ValueError, match="one rank"):
        _va(3, [1, 2, 3], [0, 0, 0], world=2)
    va = _va(3, [1, 2, 3], [0, 54, 0])
    with pytest.raises(ValueError):
        va.reset([0], start_indices=[55, 0, 0])
    with pytest.raises(ValueError):
        va.reset(seeds=[1, 2, 3, 4])
    with pytest.raises(ValueError):
        va.reset(start_indices=[0, 0])
    va.reset([1, 2], start_indices=[55, 1, 2])              # (an unmasked entry is not taken)
    assert va.starts.tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        va.step([0.0, 0.0])
    with pytest.raises(ValueError):
        va.park([True, False])


# ------------------------------------------------------------------ setpoints, VectorEnv, policies
CFG = {"agg": {"rl": {"prev_timesteps": 3}}, "rl": {"utility": {"action_space": [-1.0, 1.0], "action_scale": 100.0}}}
# a recorded sequence of loads, and what runner.Aggregator.gen_setpoint gave for it before the rule moved to
# rl.setpoint_update (timesteps 0, 1, 2, ...; max_poss_load 40, prev_timesteps 3): (setpoint, max_load, min_load)
LOADS = [9.0, 12.5, 7.25, 30.0, 1.5, 22.0]
RECORDED = [(20.0, 9.0, 9.0), (20.0, 12.5, 12.5), (15.75, 12.5, 7.25), (19.083333333333332, 30.0, 7.25),
            (12.916666666666666, 30.0, 1.5), (17.833333333333332, 30.0, 1.5)]


def _bare_runner(max_poss_load=40.0):
    from dragg_amd.runner import Aggregator
    a = Aggregator.__new__(Aggregator)
    a.config, a.max_poss_load, a.timestep, a.agg_load = CFG, max_poss_load, 0, 0
    return a


def test_runner_gen_setpoint_unchanged_on_a_recorded_sequence():
    from dragg_amd.rl import setpoint_update
    a = _bare_runner()
    state = None
    for t, load in enumerate(LOADS):
        a.timestep, a.agg_load = t, load
        sp = a.gen_setpoint()
        assert (float(sp), a.max_load, a.min_load) == RECORDED[t], t
        assert sp == a.avg_load and len(a.tracked_loads) == 3
        state = setpoint_update(state, t, load, 40.0, 3)
        assert (state[3], state[1], state[2]) == (sp, a.max_load, a.min_load) and state[0] == a.tracked_loads
        state = state[:3]
    # timestep % 24 == 0 restarts the extremes; timestep < 2 restarts the tracked loads
    a.timestep, a.agg_load = 24, 5.0
    a.gen_setpoint()
    assert (a.max_load, a.min_load) == (5.0, 5.0) and a.tracked_loads[-1] == 5.0
    a.timestep = 1
    a.gen_setpoint()
    assert a.tracked_loads == [20.0, 20.0, 20.0]


def test_vector_env_setpoints_equal_single_gen_setpoint_sequences():
    from dragg_amd.rl import VectorEnv
    seeds, starts = [5, 6, 7], [0, 7, 12]
    va = _va(3, seeds, starts, T=4)
    env = VectorEnv(va, CFG, max_poss_load=40.0)
    obs = env.reset()
    assert sorted(obs) == ["agg_cost", "agg_load", "agg_setpoint", "forecast_load", "timestep"]
    # the single runs: a runner per episode, in setup_rl_agg_run's / rl_step's order
    runners = []
    for e in range(3):
        a = _bare_runner()
        a.forecast_load = 3 * len(HOMES)
        a.gen_setpoint()
        a.agg_load = a.forecast_load
        a.agg_setpoint = a.gen_setpoint()
        runners.append(a)
    assert obs["agg_setpoint"].tolist() == [float(a.agg_setpoint) for a in runners]
    assert obs["agg_load"].tolist() == [9.0] * 3 and obs["timestep"].tolist() == [0, 0, 0]
    prices = [[0.0, 0.5, -0.25], [0.1, 0.5, -0.25], [0.2, 0.4, 0.0], [0.3, 0.5, 0.25], [0.3, 0.5, 0.25]]
    env.park([False, False, True])
    obs, done = env.step(prices[0])                          # episode 2 sits this one out
    assert obs["timestep"].tolist() == [1, 1, 0] and obs["agg_load"][2] == 9.0 and not done.any()
    env.resume([2])
    # the prices each episode lives through (episode 2 one step late), its single run and its runner
    lived = [[p[e] for p in (prices[1:] if e == 2 else prices[:4])] for e in range(3)]
    refs = [_single_run(seeds[e], starts[e], lived[e]) for e in range(3)]
    for k in range(5):
        if k > 0:
            obs, done = env.step(prices[k])
        for e, a in enumerate(runners):
            if a.timestep < min(k + (0 if e == 2 else 1), 4):    # the single run's rl_step: collect, new setpoint
                a.agg_load, a.forecast_load, a.agg_cost = refs[e][a.timestep][1]
                a.timestep += 1
                a.agg_setpoint = a.gen_setpoint()
            assert obs["timestep"][e] == a.timestep, (k, e)
            if a.timestep:
                assert (obs["agg_load"][e], obs["forecast_load"][e], obs["agg_cost"][e]) == \
                    (a.agg_load, a.forecast_load, a.agg_cost), (k, e)
            assert obs["agg_setpoint"][e] == float(a.agg_setpoint), (k, e)
        assert done.tolist() == [k >= 3, k >= 3, k >= 4]
    # a masked reset starts one episode over and leaves the others done
    obs = env.reset([1])
    assert obs["timestep"].tolist() == [4, 0, 4] and env.done().tolist() == [True, False, True]
    assert obs["agg_load"][1] == 9.0 and obs["agg_setpoint"][1] == 20.0


def test_train_vector_is_e_independent_pi_controllers():
    from dragg_amd.rl import SetpointAgent

    class Env:
        pass
    vec = SetpointAgent(CFG, kp=0.7, ki=0.2)
    singles = [SetpointAgent(CFG, kp=0.7, ki=0.2) for _ in range(3)]
    rng = np.random.default_rng(3)
    for _ in range(6):
        f, s = rng.uniform(0, 30, 3), rng.uniform(5, 20, 3)
        s[2] = 0.0                                           # (a zero setpoint divides by one)
        a = vec.train_vector({"forecast_load": f, "agg_setpoint": s})
        for e in range(3):
            env = Env()
            env.forecast_load, env.agg_setpoint = f[e], s[e]
            assert a[e] == singles[e].train(env)
        assert np.array_equal(vec.act_vector({"forecast_load": f, "agg_setpoint": s}) * 0 + a / 100.0, a / 100.0)
        for e in range(3):                                   # (act_vector trained once more: keep the singles level)
            env = Env()
            env.forecast_load, env.agg_setpoint = f[e], s[e]
            singles[e].train(env)
    vec.reset_vector([True, False, False])
    assert vec.integral_v[0] == 0.0 and vec.integral_v[1] == singles[1].integral


def test_runner_rl_vector_builds_the_environment(tmp_path):
    from dragg_amd.rl import SetpointAgent, VectorEnv
    from dragg_amd.runner import Aggregator
    from tests.test_rl import _rl_config
    from tests.test_runner import _synthetic_data
    data = tmp_path / "data"
    data.mkdir()
    _synthetic_data(str(data))
    _rl_config(data, dict(n=5, batt=1, pv=1, pvb=1, start="2015-01-01 00", end="2015-01-01 02", dt=4, horizon=1,
                          action_horizon=1, seed=3))
    a = Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / "outputs"), device=CPU, batch_cls=VecBatch)
    a.get_homes()
    env = a.rl_vector(4)
    assert isinstance(env, VectorEnv) and env.E == 4 and env.T == a.num_timesteps
    va = env.va
    assert va.seeds.tolist() == [3, 4, 5, 6] and va.starts.tolist() == [a.start_hour_index] * 4
    assert va.Nb == 5 and env.max_poss_load == a.max_poss_load
    env2 = a.rl_vector(2, seeds=[10, 20], start_indices=[0, 1])
    assert env2.va.seeds.tolist() == [10, 20] and env2.va.starts.tolist() == [0, 1]
    # a closed loop with the vector policy: runs to the end, every episode done, prices inside the action space
    agent = SetpointAgent({**a.config, "rl": CFG["rl"]})
    obs, done = env.reset(), np.zeros(4, bool)
    steps = 0
    while not done.all():
        price = agent.act_vector(obs)
        assert (np.abs(price) <= max(abs(agent.lo), abs(agent.hi)) / agent.scale + 1e-12).all()
        obs, done = env.step(price)
        steps += 1
    assert steps == a.num_timesteps and obs["timestep"].tolist() == [a.num_timesteps] * 4
    a.world = 2
    with pytest.raises(ValueError, match="one rank"):
        a.rl_vector(2)


# ------------------------------------------------------------------ the helpers both grouped-batch consumers share
def test_path_counts_equal_the_written_out_sums():
    rng = np.random.default_rng(4)
    bits = np.array([0, 1, 0x800, L.PATH_SECOND, L.PATH_STEPS, L.PATH_SECOND | L.PATH_STEPS, L.PATH_SECOND | 3,
                     L.PATH_FAIL_T], dtype=np.int32)
    a = bits[rng.integers(0, len(bits), size=(4, 3, 5))]                    # [T][G][Nb]
    assert all((a == b).any() for b in bits)
    p = torch.as_tensor(a)
    masks = (L.PATH_APPROX_MASK, L.PATH_STEPS, L.PATH_SECOND)
    assert L.PATH_COUNT_KEYS == ("approx_solves", "step_dp_solves", "later_launch_solves")
    total = L.path_counts(p)
    assert total.dtype == torch.int64 and total.tolist() == [int(((a & m) != 0).sum()) for m in masks]
    per_group = L.path_counts(p, (0, 2))                                    # VectorAggregator.approx_counts
    assert per_group.tolist() == [((a & m) != 0).sum((0, 2)).tolist() for m in masks]
    one_step = L.path_counts(p[1].reshape(3, -1), 1)                        # DeviceAggregator.sweep, per step
    assert one_step.tolist() == [((a[1] & m) != 0).sum(1).tolist() for m in masks]
    assert per_group.sum(1).tolist() == total.tolist() and 0 < total[0] < a.size


def test_episode_mask_none_bool_indices_and_wrong_length():
    E = 4
    assert L.episode_mask(None, E).tolist() == [True] * 4
    want = [False, True, False, True]
    for m in (want, np.array(want), torch.tensor(want), [1, 3], (3, 1), np.array([1, 3]), torch.tensor([3, 1]),
              np.array([[1], [3]])):
        got = L.episode_mask(m, E)
        assert got.dtype in (bool, torch.bool) and tuple(got.shape) == (E,) and got.tolist() == want, m
    assert L.episode_mask(torch.tensor(want), E).dtype == torch.bool         # (a bool tensor stays a tensor)
    assert L.episode_mask([], E).tolist() == [False] * 4
    for bad in ([True, False], np.ones(5, bool), torch.ones(3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="a mask of 4 episodes"):
            L.episode_mask(bad, E)
    with pytest.raises(IndexError):
        L.episode_mask([4], E)
    # both users: the device mask of VectorAggregator, the host mask of VectorEnv
    from dragg_amd.rl import VectorEnv
    va = _va(E, [1, 2, 3, 4], [0] * 4)
    assert va._mask([1, 3]).tolist() == want and va._mask(torch.tensor(want)).dtype == torch.bool
    env = VectorEnv.__new__(VectorEnv)
    env.E = E
    assert isinstance(env._host_mask(torch.tensor(want)), np.ndarray) and env._host_mask([3, 1]).tolist() == want
    with pytest.raises(ValueError):
        va._mask([True] * 3)


def test_device_f64_from_a_list_an_array_and_a_cpu_tensor():
    want = [[0.5, -1.25, 3.0], [2.0, 0.0, 1e-3]]
    for x in (want, np.array(want), np.array(want, dtype=np.float32), torch.tensor(want, dtype=torch.float32),
              torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.int32)):
        t = L.device_f64(x, CPU)
        assert t.dtype == torch.float64 and t.device == CPU and tuple(t.shape) == (2, 3)
        ref = np.asarray(x.numpy() if torch.is_tensor(x) else x, dtype=np.float64)
        assert np.array_equal(t.numpy(), ref)                              # (exact: every value widens exactly)
    g = torch.tensor(want, dtype=torch.float64, requires_grad=True)
    assert not L.device_f64(g, CPU).requires_grad
    assert L.device_f64(3, CPU).shape == () and L.device_f64([0.25], CPU).tolist() == [0.25]
