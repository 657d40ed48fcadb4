"""Price sweep, host side (CPU): G candidate reward prices solved as one grouped batch
(`DeviceAggregator.sweep`, `Aggregator.rl_sweep`, `rl.SweepAgent`) and ABI v10's symbols.

The solver is a stand-in batch with state, in the style of tests/test_rl.py's PriceBatch, that also
does what a grouped MPCBatch does (`groups`, `replicate_from`, `aggregate_groups`); what is tested is
the glue: a sweep equals the per-candidate forecasts, reads the live state without writing it, and on
two gloo ranks sums to the one-rank result under rank 0's prices."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dragg_amd.aggregator import DeviceAggregator
from dragg_amd.rl import SetpointAgent, SweepAgent, agent_policy
from tests.test_distributed import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")


class SweepBatch:
    """Stand-in solver with state: each step adds (global index+1) * (1 + price[0]) * (t+1) to the home's
    vals[0]; the sums are vals[0], its square and the price.  With groups = G it holds G replicas of the
    homes, replica g under price row g."""

    def __init__(self, homes, *a, home_offset=0, home_stride=1, device=None, groups=1, **kw):
        self.groups, self.Nb, self.H = groups, len(homes), 4
        self.N, self.off, self.stride = groups * len(homes), home_offset, home_stride
        self.vals = torch.zeros((19, self.N), dtype=torch.float64)
        self.fc = torch.zeros((15, self.H, self.N), dtype=torch.float64)
        self.status = torch.zeros(self.N, dtype=torch.int32)
        self.rp = torch.zeros((groups, 1), dtype=torch.float64)

    def set_reward_price(self, rp):
        self.rp = rp.clone().reshape(self.groups, -1)

    def step(self, t, noise=None, hist=None):
        idx = (self.off + self.stride * torch.arange(self.Nb, dtype=torch.float64) + 1).repeat(self.groups)
        self.vals[0] += idx * (1 + self.rp[:, 0].repeat_interleave(self.Nb)) * (t + 1)
        self.fc[0, 0] = self.vals[0]
        if hist is not None:
            hist.copy_(self.vals)

    def aggregate(self):
        assert self.groups == 1
        return self.aggregate_groups()[0]

    def replicate_from(self, base, stream=None):
        assert base.N * self.groups == self.N
        self.vals.copy_(base.vals.repeat(1, self.groups))
        self.fc.copy_(base.fc.repeat(1, 1, self.groups))

    def aggregate_groups(self, stream=None):
        v = self.vals[0].view(self.groups, self.Nb)
        return torch.stack([v.sum(1), (v * v).sum(1), self.rp[:, 0]], dim=1)


PRICES = [[0.5], [-0.25], [0.0]]


def _snap_equal(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def _sweep_run(rank, world, n):
    homes = [{"name": f"h{i}"} for i in range(n)]
    agg = DeviceAggregator(homes, None, None, None, 0, 6, rank=rank, world=world,
                           device=torch.device("cpu"), batch_cls=SweepBatch)
    agg.set_reward_price([0.125])
    agg.run_iteration()
    agg.collect_data()
    before = agg.snapshot()
    rp_before = agg.batch.rp.clone()
    # rank 0 decides the candidates; the others pass garbage that the broadcast overwrites
    sw = agg.sweep(PRICES if rank == 0 else [[-9.0], [-9.0], [-9.0]], 3)
    assert tuple(sw.shape) == (3, 3, 3)
    assert _snap_equal(before, agg.snapshot()) and torch.equal(agg.batch.rp, rp_before)
    assert agg.sweep(PRICES, 0).shape == (3, 0, 3)
    # the stand-in has no int_path: the counts are there, per candidate, and zero
    assert agg.sweep_counts == {k: [0, 0, 0] for k in ("approx_solves", "step_dp_solves", "later_launch_solves")}
    per = []
    for p in PRICES:
        agg.set_reward_price(p)
        per.append(agg.forecast(3))
    agg.set_reward_price([0.125])
    assert _snap_equal(before, agg.snapshot())
    return sw, torch.stack(per)


def test_sweep_equals_per_candidate_forecast_single_rank():
    sw, per = _sweep_run(0, 1, 5)
    assert torch.equal(sw, per)
    assert sw[:, 0, 2].tolist() == [0.5, -0.25, 0.0]
    assert not torch.equal(sw[0], sw[1])


def test_sweep_batch_is_cached_by_group_count():
    homes = [{"name": f"h{i}"} for i in range(4)]
    agg = DeviceAggregator(homes, None, None, None, 0, 6, device=torch.device("cpu"), batch_cls=SweepBatch)
    agg.sweep(PRICES, 1)
    rb = agg._sweep_batches[3]
    agg.sweep(PRICES, 2)
    agg.sweep(PRICES[:2], 1)
    assert agg._sweep_batches[3] is rb and sorted(agg._sweep_batches) == [2, 3]
    with pytest.raises(ValueError):
        agg.sweep([0.1, 0.2], 1)               # [G][n], not a flat list


def _sweep_worker(rank, world, port, n, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sw, per = _sweep_run(rank, world, n)
    q.put((rank, sw.tolist(), per.tolist()))
    dist.destroy_process_group()


def test_two_rank_sweep_sums_to_one_rank_under_rank0_prices():
    world, n = 2, 7
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sweep_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    sw1, _ = _sweep_run(0, 1, n)                        # the same community on one rank
    for rank, sw, per in res:
        assert sw == per                                # sweep = the per-candidate forecasts, on every rank
        sw = np.array(sw)
        np.testing.assert_allclose(sw[:, :, :2], sw1.numpy()[:, :, :2], rtol=1e-12)   # shards sum to the whole
        for g, p in enumerate(PRICES):
            assert np.all(sw[g, :, 2] == 2 * p[0])      # both ranks solved under rank 0's candidates


# ------------------------------------------------------------------ SweepAgent / agent_policy
CFG = {"rl": {"utility": {"action_space": [-4, 4], "action_scale": 100}}}


class _SweepEnv:
    """env.rl_sweep of a community whose first-step load is `load(price)`."""

    def __init__(self, load, setpoint):
        self.load, self.agg_setpoint, self.config = load, setpoint, CFG
        self.calls = []

    def rl_sweep(self, prices, steps=None):
        self.calls.append(list(prices))
        out = np.zeros((len(prices), 2, 3))
        out[:, 0, 0] = [self.load(p) for p in prices]
        out[:, 0, 1] = 1e9                               # (not the forecast column: the aggregate load)
        out[:, 1, 0] = -1e9                              # (not a later step: the first)
        return out


def test_sweep_agent_picks_candidate_nearest_setpoint():
    ag = SweepAgent(CFG, n_candidates=5)                 # actions -4, -2, 0, 2, 4 -> prices / 100
    env = _SweepEnv(lambda p: 100.0 - 1000.0 * p, setpoint=83.0)    # loads 140, 120, 100, 80, 60
    assert ag.act(env) == pytest.approx(0.02)
    assert env.calls == [pytest.approx([-0.04, -0.02, 0.0, 0.02, 0.04])]
    assert ag.history["candidates"] == [[-4.0, -2.0, 0.0, 2.0, 4.0]]
    assert ag.history["response"] == [pytest.approx([140.0, 120.0, 100.0, 80.0, 60.0])]
    assert ag.history["action"] == [2.0]
    env.agg_setpoint = 1000.0                            # far above every response: the end of the action space
    assert ag.act(env) == pytest.approx(-0.04) and -4.0 <= ag.history["action"][-1] <= 4.0
    assert len(ag.history["action"]) == 2 and len(SweepAgent(CFG).candidates()) == 8


def test_sweep_agent_breaks_ties_toward_smaller_price():
    ag = SweepAgent(CFG, n_candidates=5)
    env = _SweepEnv(lambda p: 50.0, setpoint=70.0)       # every candidate equally far
    assert ag.act(env) == 0.0
    env = _SweepEnv(lambda p: 100.0 + 1000.0 * abs(p + 0.01), setpoint=0.0)   # -0.02 and 0.0 tie at 110
    assert ag.act(env) == 0.0
    env = _SweepEnv(lambda p: 100.0 + 1000.0 * abs(p - 0.03), setpoint=0.0)   # 0.02 and 0.04 tie at 110
    assert ag.act(env) == pytest.approx(0.02)


def test_agent_policy_selects_sweep_only_when_asked():
    class A:
        config = CFG
    pol = agent_policy(A)
    assert pol.__func__ is SetpointAgent.act and isinstance(pol.__self__, SetpointAgent)
    A.config = {"rl": {**CFG["rl"], "parameters": {"kp": 2.0}}}
    pol = agent_policy(A)
    assert pol.__func__ is SetpointAgent.act and pol.__self__.kp == 2.0
    A.config = {"rl": {**CFG["rl"], "parameters": {"policy": "sweep"}}}
    pol = agent_policy(A)
    assert pol.__func__ is SweepAgent.act and pol.__self__.n == 8
    A.config = {"rl": {**CFG["rl"], "parameters": {"policy": "sweep", "candidates": 3}}}
    assert agent_policy(A).__self__.n == 3


# ------------------------------------------------------------------ the runner's rl_sweep (stand-in)
def test_rl_sweep_validates_prices_and_keeps_reward_price(tmp_path):
    from dragg_amd.runner import Aggregator
    from tests.test_rl import _rl_config
    from tests.test_runner import _synthetic_data
    data = tmp_path / "data"
    data.mkdir()
    _synthetic_data(str(data))
    params = dict(n=5, batt=1, pv=1, pvb=1, start="2015-01-01 00", end="2015-01-01 02", dt=4, horizon=1,
                  action_horizon=1, seed=3)
    _rl_config(data, params)
    a = Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / "outputs"), device=torch.device("cpu"),
                   batch_cls=SweepBatch)
    a.case = "rl_agg"
    a.get_homes()
    a.setup_rl_agg_run()
    a.rl_step(0.01)
    n = len(a.reward_price)
    assert n == 4
    before, snap = a.reward_price.copy(), a.dev.snapshot()
    out = a.rl_sweep([0.3, [-0.1] * n, [0.0]], steps=2)
    assert isinstance(out, np.ndarray) and out.shape == (3, 2, 3)
    assert out[:, 0, 2].tolist() == [0.3, -0.1, 0.0]
    for g, p in enumerate([0.3, -0.1, 0.0]):             # what rl_forecast returns for each candidate
        assert np.array_equal(out[g], a.rl_forecast(p, steps=2))
    assert np.array_equal(a.reward_price, before) and _snap_equal(a.dev.snapshot(), snap)
    assert torch.equal(a.dev.batch.rp.reshape(-1), torch.as_tensor(before))
    with pytest.raises(ValueError, match="action horizon"):
        a.rl_sweep([0.3, [0.1] * (n + 1)])
    with pytest.raises(ValueError):
        a.rl_sweep([])
    assert np.array_equal(a.reward_price, before)
    # steps default to rl.forecast_horizon and are clipped to the run's end
    left = a.num_timesteps - a.dev.timestep
    assert a.rl_sweep([0.1], steps=10 ** 6).shape == (1, left, 3)
    assert a.rl_sweep([0.1]).shape == (1, min(int(a.config["agg"]["rl"]["forecast_horizon"]), left), 3)


# ------------------------------------------------------------------ ABI v10
def test_abi_v10_symbols_and_version():
    from dragg_amd import _lib, build
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    assert "dragg_mpc_replicate" in names and "dragg_mpc_aggregate_groups" in names
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and _lib.ABI_VERSION == 10
    assert "dragg_mpc_replicate" in _lib.EXPORTS and "dragg_mpc_aggregate_groups" in _lib.EXPORTS
    assert [f for f, _ in _lib.Dims._fields_][-1] == "n_groups"
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "dragg_mpc_replicate") and hasattr(lib, "dragg_mpc_aggregate_groups")
    assert lib.dragg_mpc_abi_version() == 10
