"""An EV fleet beside the homes: DeviceAggregator(ev=...) and the runner's `[home.ev]` section.

The homes never see the vehicles: with a fleet their history, statuses and final hash are those of the run
without one, bit for bit, and agg_hist is the homes-only row plus the fleet's row -- in serial steps and in lag
mode (the S = 4 community of test_gpu_substeps.py's lag test, where every home lags).
"""
import os

import numpy as np
import pytest

from tests import fixtures as F

pytestmark = pytest.mark.gpu

N, STEPS = 64, 6


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.int64)


def _fleet(homes, tou, **kw):
    from dragg_amd.ev import EVFleet
    return EVFleet(homes, tou, 0, [0.0], day_offset=26, **kw)       # (06:30: the first departures inside the run)


@pytest.fixture(scope="module")
def world(gpu):
    """The community with vehicles at half of its homes, the run without a fleet and the serial run with one."""
    import torch
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.community import ev_sections
    from tests.test_gpu_substeps import DT, _community
    homes, oat, ghi, tou = _community(4, 1, n=N)
    for i, sec in ev_sections(N, 0.5, DT, 9).items():
        homes[i]["ev"] = sec
    env = (homes, oat, ghi, tou)
    bare = DeviceAggregator(homes, oat, ghi, tou, 0, STEPS, reward_price=[0.0], seed=12)
    bare.run_baseline()
    full = DeviceAggregator(homes, oat, ghi, tou, 0, STEPS, reward_price=[0.0], seed=12, ev=_fleet(homes, tou))
    for _ in range(STEPS):
        full.run_iteration()
        full.collect_data()
    torch.cuda.synchronize()
    return dict(env=env, bare=bare, full=full)


def test_homes_do_not_see_the_fleet(world):
    """History, status and final hash of the homes: bit-identical with and without a fleet; agg_hist = the
    homes-only rows + the fleet's rows, bit for bit; the fleet's rows are those of the fleet stepped alone."""
    import torch
    bare, full = world["bare"], world["full"]
    homes, _, _, tou = world["env"]
    assert full.ev.M == N // 2
    assert np.array_equal(_bits(bare.hist), _bits(full.hist))
    assert torch.equal(bare.status_hist, full.status_hist) and torch.equal(bare.path_hist, full.path_hist)
    assert np.array_equal(_bits(bare.batch.vals), _bits(full.batch.vals))
    assert np.array_equal(_bits(bare.batch.fc_store), _bits(full.batch.fc_store))
    assert np.array_equal(_bits(full.agg_hist), _bits(bare.agg_hist + full.ev_agg_hist))
    assert (full.ev_agg_hist[:, 0] != 0).any()
    alone = _fleet(homes, tou)
    for t in range(STEPS):
        alone.step(t)
        assert torch.equal(alone.aggregate(), full.ev_agg_hist[t]), t
        assert np.array_equal(_bits(alone.vals), _bits(full.ev_hist[t])), t


def test_lag_mode_adds_the_fleet_rows_once(world):
    """overlap=True (every home of this community lags): run_baseline's agg_hist, the homes' history and the
    fleet's are the serial run's, bit for bit."""
    import torch
    from dragg_amd.aggregator import DeviceAggregator
    homes, oat, ghi, tou = world["env"]
    full = world["full"]
    lag = DeviceAggregator(homes, oat, ghi, tou, 0, STEPS, reward_price=[0.0], seed=12, overlap=True,
                           ev=_fleet(homes, tou))
    assert lag.overlap
    out = lag.run_baseline()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(full.agg_hist))
    lag.drain()                                    # (a second drain adds nothing)
    assert np.array_equal(_bits(lag.agg_hist), _bits(full.agg_hist))
    assert np.array_equal(_bits(lag.hist), _bits(full.hist))
    assert np.array_equal(_bits(lag.ev_hist), _bits(full.ev_hist))


def test_forecast_and_resume(world, tmp_path):
    """forecast(3) at t = 2 equals the next three committed steps and restores homes and fleet; save_state /
    resume at t = 3 continues bit-identically to the uninterrupted run."""
    import torch
    from dragg_amd.aggregator import DeviceAggregator
    homes, oat, ghi, tou = world["env"]
    full = world["full"]

    def agg():
        return DeviceAggregator(homes, oat, ghi, tou, 0, STEPS, reward_price=[0.0], seed=12, ev=_fleet(homes, tou))
    a = agg()
    for _ in range(2):
        a.run_iteration()
        a.collect_data()
    before = [x.clone() for x in (a.batch.vals, a.batch.fc_store, a.ev.vals, a.ev.fc_store, a.ev.status)]
    fc = a.forecast(3)
    assert np.array_equal(_bits(fc), _bits(full.agg_hist[2:5]))
    for x, y in zip(before, (a.batch.vals, a.batch.fc_store, a.ev.vals, a.ev.fc_store, a.ev.status)):
        assert np.array_equal(_bits(x.to(torch.float64)), _bits(y.to(torch.float64)))
    a.run_iteration()
    a.collect_data()
    path = a.save_state(str(tmp_path / "state.pt"))
    b = agg()
    assert b.resume(path) == 3
    for _ in range(3, STEPS):
        b.run_iteration()
        b.collect_data()
    torch.cuda.synchronize()
    for k in ("hist", "agg_hist", "status_hist", "ev_hist", "ev_status_hist", "ev_agg_hist"):
        assert np.array_equal(_bits(getattr(b, k).to(torch.float64)), _bits(getattr(full, k).to(torch.float64))), k
    assert np.array_equal(_bits(b.ev.vals), _bits(full.ev.vals)) and np.array_equal(_bits(b.batch.vals), _bits(full.batch.vals))
    # a checkpoint with vehicles is refused by a run without them
    c = DeviceAggregator(homes, oat, ghi, tou, 0, STEPS, reward_price=[0.0], seed=12)
    with pytest.raises(ValueError, match="vehicles"):
        c.load_state(path)


def test_sweep_and_commit_refuse_a_fleet(world):
    full = world["full"]
    with pytest.raises(NotImplementedError, match="EV fleet"):
        full.sweep([[0.0], [0.01]], 1)
    with pytest.raises(NotImplementedError, match="EV fleet"):
        full.commit(0)


def test_runner_writes_ev_json(gpu, tmp_path, monkeypatch):
    """A synthetic-weather config with `[home.ev]`: ev.json is written, its aggregate is agg_hist's loads, and
    results.json is byte-identical to the same config's run without the section (the clock frozen for both)."""
    import datetime as dt_mod
    import json
    from dragg_amd import runner
    from tests.test_gpu_commit import _synthetic_data

    class Frozen(dt_mod.datetime):
        @classmethod
        def now(cls, tz=None):
            return cls(2015, 1, 1)
    monkeypatch.setattr(runner, "datetime", Frozen)
    params = dict(n=12, batt=3, pv=3, pvb=2, start="2015-01-01 00", end="2015-01-01 03", dt=2, horizon=6,
                  action_horizon=6, seed=21)
    out = {}
    for name, extra in (("ev", "\n[home.ev]\nshare = 0.5\ndepart_hour = [0.5, 1.5]\n"), ("bare", "")):
        data = tmp_path / f"data_{name}"
        data.mkdir()
        _synthetic_data(str(data))
        with open(data / "config.toml", "w") as f:
            f.write(F.config_text(params) + extra)
        a = runner.Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / f"outputs_{name}"))
        path = a.run()
        with open(path, "rb") as f:
            out[name] = f.read()
        evp = os.path.join(os.path.dirname(path), "ev.json")
        if name == "bare":
            assert a.dev.ev is None and not os.path.exists(evp)
            continue
        assert a.dev.ev is not None and a.dev.ev.M == 6 and a.dev.ev.day_offset == 0
        with open(evp) as f:
            ev = json.load(f)
        assert sorted(ev["vehicles"]) == sorted(a.dev.ev.names)
        loads = a.dev.agg_hist[:, 0].cpu().numpy()
        assert ev["Summary"]["p_grid_aggregate"] == loads.tolist()
        v = next(iter(ev["vehicles"].values()))
        assert sorted(v) == sorted(["p_ev_ch", "p_ev_disch", "e_ev_opt", "cost_ev", "status"])
        assert len(v["p_ev_ch"]) == a.num_timesteps
        ch = np.array([x["p_ev_ch"] for x in ev["vehicles"].values()])
        dis = np.array([x["p_ev_disch"] for x in ev["vehicles"].values()])
        assert np.abs(ch + dis).sum() > 0
        assert np.allclose((ch + dis).sum(0), a.dev.ev_agg_hist[:, 0].cpu().numpy(), rtol=1e-12, atol=1e-12)
    assert out["ev"] == out["bare"]
