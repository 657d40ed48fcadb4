"""The device-resident vector environment, host side (CPU): the ABI surface of dragg_mpc_env_file /
dragg_mpc_env_reset, their numpy restatements (`vector.env_file_reference`, `vector.env_reset_reference`) against
`rl.VectorEnv`'s own bookkeeping, `rl.DeviceVectorEnv` on a stand-in batch whose `env_file` / `env_reset` are
served by the restatements, and `SetpointAgent.act_device` against `act_vector`."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from tests.test_vector_host import CPU, ENV, HOMES, VecBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")


def _cfg(P):
    return {"agg": {"rl": {"prev_timesteps": P}}, "rl": {"utility": {"action_space": [-1.0, 1.0], "action_scale": 100.0}}}


def _bits(x):
    x = torch.as_tensor(x)
    return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x


class EnvBatch(VecBatch):
    """The stand-in grouped batch with the two environment calls, served by the restatements."""

    def env_file(self, st, ran, sums, hist=None, stream=None):
        from dragg_amd.vector import env_file_reference
        env_file_reference(st.host(), ran.numpy(), sums.numpy(), self.status.numpy(), self.int_path.numpy(),
                           None if hist is None else hist.numpy())

    def env_reset(self, st, mask, stream=None):
        from dragg_amd.vector import env_reset_reference
        env_reset_reference(st.host(), mask.numpy(), self.vals.numpy(), self.fc.permute(2, 0, 1).numpy())


def _va(E, seeds, starts, T, cls):
    from dragg_amd.vector import VectorAggregator
    env = ENV * 2 if T > 40 else ENV
    return VectorAggregator(HOMES, env, env, env, E, seeds, starts, T, device=CPU, batch_cls=cls)


# ------------------------------------------------------------------ ABI surface
def test_abi_surface_of_the_environment_entry_points(tmp_path):
    from dragg_amd import build
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    new = ["dragg_mpc_env_file", "dragg_mpc_env_reset"]
    assert all(n in names and n in L.EXPORTS for n in new)
    assert "typedef struct dragg_mpc_env" in h
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and L.ABI_VERSION == 10
    assert re.search(r"#define\s+DRAGG_ENV_PREV_MAX\s+128\b", h) and L.ENV_PREV_MAX == 128
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, n) for n in new) and lib.dragg_mpc_abi_version() == 10
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(dragg_mpc_env));']
    for f, _ in L.Env._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(dragg_mpc_env, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.Env) == 112
    assert [f for f, _ in L.Env._fields_] == ["num_timesteps", "prev_timesteps", "max_poss_load", "start_load", "ran",
                                              "clock", "max_load", "min_load", "tracked", "obs", "sums",
                                              "status_hist", "path_hist", "hist", "agg_hist"]
    for f, _ in L.Env._fields_:
        assert int(got[f]) == getattr(L.Env, f).offset, f


# ------------------------------------------------------------------ the restatement against rl.setpoint_update
@pytest.mark.parametrize("P", [1, 7, 8, 9, 12, 24, 128])
def test_restatement_equals_vector_env_bookkeeping(P):
    """60 steps of random loads (timestep % 24 == 0 twice) through the restatement and through `VectorEnv`'s own
    loop body: tracked loads, max, min, setpoint and observations bit-identical at every step."""
    from dragg_amd.rl import VectorEnv
    from dragg_amd.vector import env_file_reference, env_reset_reference
    E, T = 2, 60
    va_h, va_d = _va(E, [1, 2], [0, 0], T, VecBatch), _va(E, [1, 2], [0, 0], T, EnvBatch)
    env = VectorEnv(va_h, _cfg(P), max_poss_load=37.3)
    env.reset()
    st = va_d.env_state(P, 37.3, 3 * len(HOMES))
    h = st.host()
    env_reset_reference(h, np.ones(E, bool), va_d.batch.vals.numpy(), va_d.batch.fc.permute(2, 0, 1).numpy())
    rng = np.random.default_rng(100 + P)
    for t in range(T):
        sums = rng.uniform(0.0, 40.0, (E, 3))
        for e in range(E):                                   # VectorEnv.step's loop body
            env.timestep[e] += 1
            env.agg_load[e], env.forecast_load[e], env.agg_cost[e] = sums[e]
            env._setpoint(e)
        env_file_reference(h, np.full(E, t, dtype=np.int32), sums, va_d.batch.status.numpy(),
                           va_d.batch.int_path.numpy(), None)
        for e in range(E):
            tr, mx, mn = env._sp[e]
            assert _bits(np.asarray(tr, dtype=float)).tolist() == _bits(h["tracked"][e]).tolist(), (t, e)
            assert (mx, mn) == (h["max_load"][e], h["min_load"][e]), (t, e)
        obs = env.observations()
        for i, k in enumerate(L.OBS_KEYS):
            assert _bits(np.asarray(obs[k], dtype=float)).tolist() == _bits(h["obs"][i]).tolist(), (t, k)
        assert h["clock"].tolist() == [t + 1] * E


def test_more_than_128_tracked_loads_are_refused():
    from dragg_amd.rl import DeviceVectorEnv
    va = _va(2, [1, 2], [0, 0], 4, EnvBatch)
    for bad in (129, 0):
        with pytest.raises(ValueError, match="prev_timesteps"):
            DeviceVectorEnv(va, _cfg(bad), max_poss_load=40.0)
    DeviceVectorEnv(va, _cfg(128), max_poss_load=40.0)


# ------------------------------------------------------------------ DeviceVectorEnv on a stand-in batch
def _same(host_env, dev_env, what):
    obs_h, obs_d = host_env.observations(), dev_env.observations()
    for k in L.OBS_KEYS:
        assert torch.is_tensor(obs_d[k]) and tuple(obs_d[k].shape) == (host_env.E,)
        assert _bits(np.asarray(obs_h[k], dtype=float)).tolist() == _bits(obs_d[k]).tolist(), (what, k)
    a, b = host_env.va, dev_env.va
    assert a.clocks.tolist() == b.clocks.tolist() and b.clocks.dtype == torch.int32, what
    assert host_env.done().tolist() == dev_env.done().tolist() and dev_env.done().dtype == torch.bool, what
    for k in ("hist", "status_hist", "path_hist", "agg_hist"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), (what, k)
    assert torch.equal(_bits(a.batch.vals), _bits(b.batch.vals)) and torch.equal(_bits(a.batch.fc), _bits(b.batch.fc)), what
    assert a.seeds.tolist() == b.seeds.tolist() and a.starts.tolist() == b.starts.tolist(), what


def test_device_vector_env_equals_vector_env_on_a_stand_in():
    """E = 4, T = 6: a reset of episode 1 at step 2 with a new seed, a park and resume of episode 2, episodes
    finishing at different times; observations, clocks, stores and done equal at every step."""
    from dragg_amd.rl import DeviceVectorEnv, VectorEnv
    E, T = 4, 6
    seeds, starts = [5, 6, 7, 8], [0, 7, 12, 3]
    host = VectorEnv(_va(E, seeds, starts, T, VecBatch), _cfg(3), max_poss_load=40.0)
    dev = DeviceVectorEnv(_va(E, seeds, starts, T, EnvBatch), _cfg(3), max_poss_load=40.0)
    host.reset()
    obs = dev.reset()
    assert sorted(obs) == sorted(L.OBS_KEYS) and obs["agg_load"].tolist() == [9.0] * E
    _same(host, dev, "reset")
    rng = np.random.default_rng(8)
    k = 0
    while not host.done().all():
        if k == 2:
            host.reset([1], seeds=[0, 9, 0, 0])
            dev.reset(torch.tensor([False, True, False, False]), seeds=torch.tensor([0, 9, 0, 0]))
            _same(host, dev, "masked reset")
        if k == 3:
            host.park([2])
            dev.park(torch.tensor([False, False, True, False]))
        if k == 5:
            host.resume([2])
            dev.resume([2])
        p = rng.uniform(-0.3, 0.3, E)
        _, done_h = host.step(p)
        obs_d, done_d = dev.step(torch.as_tensor(p))
        assert torch.is_tensor(done_d) and done_h.tolist() == done_d.tolist()
        _same(host, dev, k)
        k += 1
        assert k < 20
    assert k == 8 and dev.va.clocks.tolist() == [T] * E        # (episode 1 and episode 2 finish two steps late)
    # the finished episodes start over from the device mask, with device keys
    dev.reset(dev.done(), seeds=torch.tensor([11, 12, 13, 14]), start_indices=torch.tensor([1, 2, 3, 4], dtype=torch.int32))
    host.reset(host.done(), seeds=[11, 12, 13, 14], start_indices=[1, 2, 3, 4])
    _same(host, dev, "reset(done())")
    host.step([0.1] * E)
    dev.step([0.1] * E)
    _same(host, dev, "after the second start")
    # host lists are checked as before
    with pytest.raises(ValueError):
        dev.reset([0], start_indices=[60, 0, 0, 0])


def test_step_swept_on_a_stand_in_keeps_the_choice_on_the_device():
    from dragg_amd.rl import DeviceVectorEnv, SweepAgent, VectorEnv

    class SweepBatch(EnvBatch):
        def replicate_from(self, base, stream=None):
            C = self.groups // base.groups
            self.vals.copy_(base.vals.repeat(1, C))
            self.fc.copy_(base.fc.repeat(1, 1, C))

        def adopt_from(self, src, choice, hist=None, stream=None):
            for e, c in enumerate(choice.tolist()):
                if c < 0:
                    continue
                d, s = slice(e * self.Nb, (e + 1) * self.Nb), slice(c * self.N + e * self.Nb, c * self.N + (e + 1) * self.Nb)
                self.vals[:, d], self.fc[:, :, d] = src.vals[:, s], src.fc[:, :, s]
                self.status[d], self.int_path[d] = src.status[s], src.int_path[s]
                if hist is not None:
                    hist[:, d] = src.hist_row[:, s]

        def select_groups(self, sums, target, prices, stream=None):
            E = self.groups
            d = (torch.as_tensor(sums)[:, 0].view(-1, E) - torch.as_tensor(target).view(1, E)).abs()
            return d.argmin(0).to(torch.int32)
    E, T = 3, 3
    agent = SweepAgent(_cfg(3), n_candidates=3)
    host = VectorEnv(_va(E, [1, 2, 3], [0, 1, 2], T, SweepBatch), _cfg(3), max_poss_load=40.0)
    dev = DeviceVectorEnv(_va(E, [1, 2, 3], [0, 1, 2], T, SweepBatch), _cfg(3), max_poss_load=40.0)
    obs_h, obs_d = host.reset(), dev.reset()
    dev.park([1])
    host.park([1])
    for k in range(2):
        c_h, c_d = agent.act_vector(obs_h), agent.act_device(obs_d)
        assert torch.is_tensor(c_d) and c_d.tolist() == c_h.tolist()
        obs_h, _ = host.step_swept(c_h)
        obs_d, _ = dev.step_swept(c_d)
        assert torch.is_tensor(dev.choice) and dev.choice.dtype == torch.int32
        assert dev.choice.tolist() == host.choice.tolist() and dev.choice[1] == -1
        _same(host, dev, k)


# ------------------------------------------------------------------ the PI controller on tensors
def test_act_device_equals_act_vector_bit_for_bit():
    from dragg_amd.rl import SetpointAgent
    a, b = SetpointAgent(_cfg(3), kp=0.7, ki=0.2), SetpointAgent(_cfg(3), kp=0.7, ki=0.2)
    rng = np.random.default_rng(3)
    E = 5
    for k in range(40):
        f, s = rng.uniform(0, 30, E), rng.uniform(5, 20, E)
        s[2] = 0.0                                           # (a zero setpoint divides by one)
        if k % 7 == 3:
            f[1] = 1e4                                       # (drives the integral and the action into their clamps)
        if k == 20:
            mask = np.array([True, False, False, True, False])
            a.reset_vector(mask)
            b.reset_device(torch.as_tensor(mask))
        x = a.act_vector({"forecast_load": f, "agg_setpoint": s})
        y = b.act_device({"forecast_load": torch.as_tensor(f), "agg_setpoint": torch.as_tensor(s)})
        assert torch.is_tensor(y) and y.dtype == torch.float64
        assert _bits(x).tolist() == _bits(y).tolist(), k
        assert _bits(a.integral_v).tolist() == _bits(b.integral_d).tolist(), k
    assert len(b.history_device["action"]) == 40 and torch.is_tensor(b.history_device["error"][0])
    assert _bits(torch.stack(b.history_device["action"])).tolist() == _bits(np.asarray(a.history["action"])).tolist()
    c = SetpointAgent(_cfg(3))
    c.act_device({"forecast_load": torch.ones(2, dtype=torch.float64), "agg_setpoint": torch.ones(2, dtype=torch.float64)},
                 history=False)
    assert getattr(c, "history_device", None) is None
    b.reset_device()
    assert float(b.integral_d.abs().sum()) == 0.0


def test_runner_rl_vector_builds_the_device_environment(tmp_path):
    from dragg_amd.rl import DeviceVectorEnv, VectorEnv
    from dragg_amd.runner import Aggregator
    from tests.test_rl import _rl_config
    from tests.test_runner import _synthetic_data
    data = tmp_path / "data"
    data.mkdir()
    _synthetic_data(str(data))
    _rl_config(data, dict(n=5, batt=1, pv=1, pvb=1, start="2015-01-01 00", end="2015-01-01 02", dt=4, horizon=1,
                          action_horizon=1, seed=3))
    a = Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / "outputs"), device=CPU, batch_cls=EnvBatch)
    a.get_homes()
    assert type(a.rl_vector(2)) is VectorEnv
    env = a.rl_vector(4, device_env=True)
    assert isinstance(env, DeviceVectorEnv) and env.E == 4 and env.T == a.num_timesteps
    assert env.max_poss_load == a.max_poss_load and env.state.start_load == 3 * len(a.all_homes)
    ref = a.rl_vector(4)
    obs, obs_ref = env.reset(), ref.reset()
    for k in range(a.num_timesteps):
        obs, done = env.step([0.01 * k] * 4)
        obs_ref, done_ref = ref.step([0.01 * k] * 4)
        assert obs["agg_setpoint"].tolist() == obs_ref["agg_setpoint"].tolist()
    assert bool(done.all()) and done_ref.all()
