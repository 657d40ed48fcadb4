"""Drop-in for `dragg.aggregator.Aggregator` on its run_rbo_mpc path, solved on MI355X.

Reference: aggregator.py:28-970 (+ `dragg/main.py`: `Aggregator().run()`).  The same
environment variables, config.toml, NSRDB weather csv and water-draw profiles go in; the
same outputs come out (outputs/all_homes-<N>-config.json and
outputs/<run dir>/baseline/results.json, checkpointed at the configured cadence).  In between,
nothing of the reference's per-step machinery is left: no process pool, no pickled MPCCalc,
no redis round trips.  The community's state stays on the GPU (`DeviceAggregator`), one
kernel launch per timestep solves every home of this rank's shard, and the hash history is
brought to the host only when an output file is written.

    python -m dragg_amd.runner            # like `python -m dragg.main`, DATA_DIR / CONFIG_FILE honoured

Multi-GPU: start one process per GPU (torchrun) with torch.distributed initialised
(backend "nccl" = RCCL); homes are sharded by stride (shard_index), the three per-step sums are
all-reduced, rank 0 gathers the history and writes the files.

Scope: run_rbo_mpc (the baseline case) and the RL-aggregator hooks (SURVEY.md §8 F4:
`setup_rl_agg_run`, `redis_set_current_values`, `gen_setpoint`, `test_response`, plus
`rl_step` / `rl_forecast` / `run_rl_agg`, the reward-price loop the reference leaves to an
external driver).  SPP prices (`agg.spp_enabled`, an ERCOT xlsx absent from the reference)
raise.
"""
import json
import logging
import os
import time
import warnings
from contextlib import contextmanager
from datetime import datetime

import numpy as np

from . import inputs as I
from . import results as R


class Aggregator:
    def __init__(self, data_dir=None, config_file=None, outputs_dir="outputs", int_mode="round", device=None,
                 group=None, first_name=None, batch_cls=None):
        # wall seconds per phase of the run (tools/e2e.py): {phase: seconds}, accumulated
        self.timings = {}
        with self._phase("config_and_weather"):
            self._init(data_dir, config_file, outputs_dir, int_mode, device, group, first_name, batch_cls)

    @contextmanager
    def _phase(self, name):
        t0 = time.perf_counter()
        try:
            yield
        finally:
            self.timings[name] = self.timings.get(name, 0.0) + time.perf_counter() - t0

    def _init(self, data_dir, config_file, outputs_dir, int_mode, device, group, first_name, batch_cls):
        env = os.environ
        self.data_dir = os.path.expanduser(env.get("DATA_DIR", "data")) if data_dir is None else data_dir
        self.outputs_dir = outputs_dir
        self.config_file = config_file or os.path.join(self.data_dir, env.get("CONFIG_FILE", "config.toml"))
        self.ts_data_file = os.path.join(self.data_dir, env.get("SOLAR_TEMPERATURE_DATA_FILE", "nsrdb.csv"))
        self.config = I.read_config(self.config_file)
        self.check_type = self.config["simulation"]["check_type"]
        self.dt = int(self.config["agg"]["subhourly_steps"])
        self.dt_interval = 60 // self.dt
        self.ts_data = I.load_weather(self.ts_data_file, self.dt)
        self.start_dt, self.end_dt, self.hours = I.run_window(self.config)
        self.num_timesteps = int(np.ceil(self.hours * self.dt))
        if self.config["agg"]["spp_enabled"]:
            raise I.ConfigError("SPP prices (agg.spp_enabled) are not supported by this build")
        self.tou_data = I.tou_prices(self.start_dt, self.hours, self.config["agg"])
        self.all_data, self.mask = I.join_series(self.ts_data, self.tou_data, self.start_dt, self.end_dt)
        self.all_rps = np.zeros(self.num_timesteps)
        self.all_sps = np.zeros(self.num_timesteps)
        self.case = "baseline"
        self.int_mode, self.device, self.group = int_mode, device, group
        self.first_name = first_name
        self.batch_cls = batch_cls          # injectable only for the CPU tests of the multi-rank glue
        self.rank, self.world = 0, 1
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        except ImportError:
            pass
        self.agg_load = 0                   # aggregator.py:55-57
        self.baseline_agg_load_list = []
        self.max_agg_load_list = []
        self.dev = None
        if self.rank == 0:
            os.makedirs(self.outputs_dir, exist_ok=True)

    # aggregator.py:913-925 (flush_redis: the checks, the start index and initial values)
    def flush(self):
        I.check_series(self.all_data, self.start_dt, self.end_dt, self.config["home"]["hems"]["prediction_horizon"])
        self.start_hour_index = I.start_hour_index(self.all_data, self.start_dt)
        self.timestep = 0
        self.reward_price = np.zeros(self.config["agg"]["rl"]["action_horizon"] * self.dt)

    # aggregator.py:263-271
    def get_homes(self):
        n = self.config["community"]["total_number_homes"]
        path = os.path.join(self.outputs_dir, f"all_homes-{n}-config.json")
        with self._phase("create_homes"):
            if not self.config["community"]["overwrite_existing"] and os.path.isfile(path):
                with open(path) as f:
                    self.all_homes = json.load(f)
            else:
                draws = os.path.join(self.data_dir, self.config["home"]["wh"]["waterdraw_file"])
                self.all_homes = I.create_homes(self.config, self.num_timesteps, self.dt, draws, self.first_name)
            I.check_home_counts(self.all_homes, self.config)
        if self.rank == 0:
            with self._phase("write_home_configs"):
                R.write_home_configs(self.outputs_dir, self.all_homes, n)
        self.max_poss_load = sum(I.max_load(h) for h in self.all_homes)

    def _checked_community(self):
        """What either device aggregator is built from: the checked homes (aggregator.py:762-765), OAT, GHI, tou."""
        checked = [h for h in self.all_homes if self.check_type == "all" or h["type"] == self.check_type]
        col = lambda c: self.all_data[c].to_numpy(dtype=float)  # noqa: E731
        return checked, col("OAT"), col("GHI"), col("tou")

    def _device_community(self):
        """The checked homes (aggregator.py:762-765 / 879-882) as this rank's device shard."""
        from .aggregator import DeviceAggregator
        self.checked, oat, ghi, tou = self._checked_community()
        self._hist_rows = 0                 # steps of the history already on rank 0 (_history)
        fleet = self._fleet(tou)
        self.dev = DeviceAggregator(self.checked, oat, ghi, tou, self.start_hour_index,
                                    self.num_timesteps, reward_price=self.reward_price, int_mode=self.int_mode,
                                    seed=int(self.config["simulation"]["random_seed"]), rank=self.rank,
                                    world=self.world, group=self.group, device=self.device,
                                    # run_rbo_mpc: a home in its step-function DP does not hold up the
                                    # others (lag mode, DeviceAggregator); results are bit-identical
                                    overlap=getattr(self, "case", None) == "baseline",
                                    **({"ev": fleet} if fleet is not None else {}),
                                    **({"batch_cls": self.batch_cls} if self.batch_cls else {}))
        return self.dev

    def _fleet(self, tou):
        """The optional `[home.ev]` config section (`share`, and any range of community.EV_RANGES): that share of
        the checked homes gets a vehicle (community.ev_sections: a generator of its own, keyed by the run's seed)
        and this rank's shard of them becomes an EVFleet beside the homes.  The home dicts themselves are not
        touched: results.json and the all-homes file are what they are without the section.  None without it."""
        cfg = self.config["home"].get("ev")
        if not cfg or float(cfg.get("share", 0.0)) <= 0.0:
            return None
        from .community import ev_sections
        from .ev import build_fleet
        secs = ev_sections(len(self.checked), cfg["share"], self.dt, int(self.config["simulation"]["random_seed"]), cfg)
        homes = [dict(h, ev=secs[i]) if i in secs else h for i, h in enumerate(self.checked)]
        day_offset = (self.start_dt.hour * self.dt + self.start_dt.minute // self.dt_interval) % (24 * self.dt)
        return build_fleet(homes, tou=tou, start_index=self.start_hour_index, reward_price=self.reward_price,
                           day_offset=day_offset, rank=self.rank, world=self.world,
                           **({"device": self.device} if self.device is not None else {}))

    def write_ev_outputs(self):
        """`ev.json` next to results.json: per vehicle its four series and its statuses, and the community's
        p_grid_aggregate with the vehicles (agg_hist's loads).  With more than one rank each rank writes its own
        vehicles (`ev-rank<r>-of-<w>.json`)."""
        dev = self.dev
        if dev is None or getattr(dev, "ev", None) is None:
            return None
        from . import _lib as L
        dev.drain()
        T = dev.timestep
        hist = dev.ev_hist[:T].cpu().numpy()
        status = dev.ev_status_hist[:T].cpu().numpy()
        out = {"vehicles": {}}
        for j, name in enumerate(dev.ev.names):
            rec = {k: hist[:, L.EVK[k], j].tolist() for k in L.EV_KEYS}
            rec["status"] = status[:, j].tolist()
            out["vehicles"][name] = rec
        out["Summary"] = {"p_grid_aggregate": dev.agg_hist[:T, 0].cpu().numpy().tolist()}
        d = os.path.join(self.run_dir, self.case)
        os.makedirs(d, exist_ok=True)
        name = "ev.json" if self.world == 1 else f"ev-rank{self.rank}-of-{self.world}.json"
        path = os.path.join(d, name)
        with open(path, "w") as f:
            json.dump(out, f)
        return path

    def state_path(self):
        """This rank's device-state checkpoint, next to results.json (<run dir>/<case>/)."""
        d = os.path.join(self.run_dir, self.case)
        os.makedirs(d, exist_ok=True)
        return os.path.join(d, f"state-rank{self.rank}-of-{self.world}.pt")

    # aggregator.py:757-778
    def run_baseline(self, noise_fn=None, resume=False, stop_after=None):
        """`noise_fn(t)`, optional: the season draw [H][homes checked] of step t (replaces the
        keyed on-device stream, e.g. to replay a recorded run).  Every checkpoint also saves
        each rank's device state; `resume=True` continues from it (the reference has no resume:
        aggregator.py:265-267, 768) and finishes with the results an uninterrupted run writes.
        Every rank must resume from the same timestep (a crash between two ranks' saves leaves
        them apart): they check that together and all raise otherwise.  `stop_after`: return
        after the first checkpoint at or past that many steps (an interrupted run)."""
        self.start_time = datetime.now()
        with self._phase("upload"):
            self._device_community()
            self._sync()
        t0 = 0
        if resume:                                 # every rank loads, then all agree (or all raise)
            t0 = self.dev.resume(self.state_path())
            self.timestep = t0
        loop_t0 = time.perf_counter()
        ckpt = self.timings.get("checkpoints", 0.0)
        for t in range(t0, self.num_timesteps):
            noise = noise_fn(t)[:, self.dev.index] if noise_fn is not None else None
            self.dev.run_iteration(noise)
            self.dev.collect_data(defer=True)      # no feedback: the sums are reduced at the end
            self.timestep = t + 1
            if (t + 1) % self.checkpoint_interval == 0:
                with self._phase("checkpoints"):
                    # the reference raises inside the step that fails (mpc_calc.py:280-289,
                    # 537-539); checking at each checkpoint (one host sync) keeps post-error data
                    # out of every results.json written
                    self.dev.check_errors()
                    self.write_outputs()
                    self.dev.save_state(self.state_path())
                if stop_after is not None and t + 1 >= stop_after:
                    return                         # an interrupted run
        self.dev.reduce_history()
        self.dev.check_errors()
        self.check_solve_paths()
        # the step loop: launches and device time of every step, without the checkpoint writes
        self.timings["step_loop"] = (self.timings.get("step_loop", 0.0) + time.perf_counter() - loop_t0
                                     - (self.timings.get("checkpoints", 0.0) - ckpt))

    def _sync(self):
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize()
        except ImportError:
            pass

    def check_solve_paths(self):
        """The run's solve-path counts over every rank (`self.solve_paths`: approximate solves, solves by
        the step-function DP, solves finished by a later launch); warns when a solve kept an approximate
        integer schedule -- the reference's GLPK_MI solve is exact up to its gap (mpc_calc.py:447-451),
        so such a run is not the reference's to that tolerance (int_path reasons 3 and 6)."""
        self.solve_paths = self.dev.approx_counts()
        n = self.solve_paths["approx_solves"]
        if n:
            where = self.dev.approx_solves()[:5]
            warnings.warn(f"{n} solve(s) kept an approximate integer schedule (int_path reason 3 / 6; first on "
                          f"this rank as (timestep, home, int_path): {where}); rerun with a larger "
                          "DRAGG_STEP_WORK_CAP / DRAGG_STEP_POOL_CAP or dims.flags DRAGG_FLAG_EXACT", RuntimeWarning)
        return self.solve_paths

    # ------------------------------------------------------------------ RL aggregator (§8 F4)
    # aggregator.py:677-696
    def gen_setpoint(self):
        # (the rule itself: rl.setpoint_update, shared with the per-episode setpoints of rl.VectorEnv)
        from .rl import setpoint_update
        fresh = self.timestep < 2
        state = None if fresh else (self.tracked_loads, self.max_load, self.min_load)
        self.tracked_loads, self.max_load, self.min_load, self.avg_load = setpoint_update(
            state, self.timestep, self.agg_load, self.max_poss_load,
            self.config["agg"]["rl"]["prev_timesteps"] if fresh else None)
        return self.avg_load

    def rl_vector(self, episodes, seeds=None, start_indices=None, device_env=False, plan_keys=(), plan_rows=(),
                  price_classes=None, vehicles=None):
        """A vector environment of `episodes` independent runs of the loaded community (`get_homes`), all
        stepped as one grouped batch (dragg_amd.vector.VectorAggregator, rl.VectorEnv): default seeds
        `simulation.random_seed + e`, default start indices the config's own.  device_env=True: an
        `rl.DeviceVectorEnv` (observations, done flags and choices stay on the device); `plan_keys` /
        `plan_rows`: its plan observations (device_env=True only).  `price_classes`: a reward price per class of
        homes -- "type" (class = home type: base 0, pv_only 1, battery_only 2, pv_battery 3; P = 4 even if a type is
        absent) or an int sequence, one class per loaded home in `all_homes`' order (default: the config's
        `rl.utility.price_classes`, else none); actions and candidates then take the class shapes of
        `VectorAggregator`.  `vehicles`: a config with a `[home.ev]` share > 0 must choose -- True: the vehicles
        `run()` would build (the same sections, the day clock re-based to environment index 0) are stepped beside
        every episode's homes (`VectorAggregator(vehicles=True)`) and count in the sums and in max_poss_load;
        False: they are left out on purpose; None (default) raises NotImplementedError for such a config rather
        than deciding silently.  One rank only."""
        from .rl import DeviceVectorEnv, VectorEnv
        from .vector import VectorAggregator
        if self.world > 1:
            raise ValueError("rl_vector runs on one rank: episodes are not sharded over ranks")
        ev_cfg = (self.config.get("home") or {}).get("ev") or {}
        ev_share = float(ev_cfg.get("share", 0.0))
        if ev_share > 0.0 and vehicles is None:
            raise NotImplementedError("rl_vector: this config's [home.ev] section asks for an EV fleet; choose "
                                      "vehicles=True (the vehicles are stepped beside every episode's homes) or "
                                      "vehicles=False (they are left out)")
        if not hasattr(self, "start_hour_index"):
            self.flush()
        E = int(episodes)
        seed = int(self.config["simulation"]["random_seed"])
        checked, oat, ghi, tou = self._checked_community()
        if price_classes is None:
            price_classes = ((self.config.get("rl") or {}).get("utility") or {}).get("price_classes")
        n_classes = None
        if price_classes is not None and not isinstance(price_classes, str):
            # one class per loaded home: P from the whole list, the map for the checked homes
            from ._lib import price_class_map
            pc, n_classes = price_class_map(list(price_classes), len(self.all_homes))
            price_classes = [int(c) for c, h in zip(pc, self.all_homes)
                             if self.check_type == "all" or h["type"] == self.check_type]
        ev_kw, ev_rate = {}, 0.0
        if vehicles and ev_share > 0.0:
            from .community import ev_sections
            secs = ev_sections(len(checked), ev_cfg["share"], self.dt, seed, ev_cfg)
            checked = [dict(h, ev=secs[i]) if i in secs else h for i, h in enumerate(checked)]
            # _fleet's day clock is that of environment index start_hour_index: re-based to index 0
            day0 = (self.start_dt.hour * self.dt + self.start_dt.minute // self.dt_interval) % (24 * self.dt)
            ev_kw = dict(vehicles=True, day_offset=(day0 - self.start_hour_index) % (24 * self.dt))
            ev_rate = sum(float(s["max_rate"]) for s in secs.values())
        va = VectorAggregator(checked, oat, ghi, tou, E,
                              [seed + e for e in range(E)] if seeds is None else seeds,
                              [self.start_hour_index] * E if start_indices is None else start_indices,
                              self.num_timesteps, int_mode=self.int_mode, device=self.device,
                              price_classes=price_classes, n_classes=n_classes, **ev_kw,
                              **({"batch_cls": self.batch_cls} if self.batch_cls else {}))
        kw = dict(max_poss_load=sum(I.max_load(h) for h in self.all_homes) + ev_rate, n_homes=len(self.all_homes))
        if not device_env:
            if plan_keys or plan_rows:
                raise ValueError("plan observations need device_env=True (rl.DeviceVectorEnv)")
            return VectorEnv(va, self.config, **kw)
        return DeviceVectorEnv(va, self.config, plan_keys=plan_keys, plan_rows=plan_rows, **kw)

    # aggregator.py:664-675: the reward price goes to every rank's solver (RCCL broadcast from
    # rank 0) instead of the redis 'reward_price' list
    def redis_set_current_values(self):
        if "rl" in self.case:
            self.all_sps[self.timestep] = self.agg_setpoint
            self.all_rps[self.timestep] = self.reward_price[0]
            self.dev.set_reward_price(self.reward_price)

    # aggregator.py:876-896
    def setup_rl_agg_run(self, noise_fn=None):
        """Needs the community (`get_homes`) like the reference's (it reads all_homes_obj)."""
        self.flush()
        self._device_community()
        self.noise_fn = noise_fn
        self.start_time = datetime.now()
        self.baseline_agg_load_list = [0]
        self.all_rewards = []
        self.forecast_load = 3 * len(self.all_homes)
        self.prev_forecast_load = self.forecast_load
        self.forecast_setpoint = self.gen_setpoint()
        self.agg_load = self.forecast_load  # approximate load for initial timestep
        self.agg_setpoint = self.gen_setpoint()
        self.redis_set_current_values()

    def _noise(self, t):
        fn = getattr(self, "noise_fn", None)
        return fn(t)[:, self.dev.index] if fn is not None else None

    # aggregator.py:728-755 on the RL path: the three community sums come to the host (the
    # agent needs them) and feed the setpoint
    def collect_data(self):
        agg = self.dev.collect_data().tolist()
        self.agg_load, self.forecast_load, self.agg_cost = agg
        self.baseline_agg_load_list.append(self.agg_load)
        self.agg_setpoint = self.gen_setpoint()
        return agg

    def _price_list(self, reward_price):
        rp = np.asarray(reward_price, dtype=float).reshape(-1)
        if len(rp) == 1:
            rp = np.full(len(self.reward_price), rp[0])
        if len(rp) != len(self.reward_price):
            raise ValueError(f"reward price has {len(rp)} entries, the action horizon holds "
                             f"{len(self.reward_price)} (agg.rl.action_horizon * dt)")
        return rp

    def _set_price(self, reward_price):
        self.reward_price = self._price_list(reward_price)

    def rl_step(self, reward_price):
        """One RL-aggregator timestep under `reward_price` (a scalar, or action_horizon*dt
        values): publish the price, solve every home, collect, new setpoint -- the order of
        the reference's step loop (aggregator.py:768-771)."""
        self._set_price(reward_price)
        self.redis_set_current_values()
        self.dev.run_iteration(self._noise(self.dev.timestep))
        self.timestep = self.dev.timestep
        return self.collect_data()

    def rl_forecast(self, reward_price, steps=None):
        """The community's response to a candidate price over `rl.forecast_horizon` timesteps
        (README.md:67, `rl_agg_forecast_horizon`): every home re-solved ahead on device,
        nothing committed.  -> [steps][agg_load, forecast_load, agg_cost] on the host."""
        steps = int(self.config["agg"]["rl"]["forecast_horizon"]) if steps is None else int(steps)
        steps = min(steps, self.num_timesteps - self.dev.timestep)
        prev = self.reward_price
        self._set_price(reward_price)
        self.dev.set_reward_price(self.reward_price)
        try:
            out = self.dev.forecast(steps, noise_fn=self._noise if getattr(self, "noise_fn", None) else None)
        finally:
            self.reward_price = prev
            self.dev.set_reward_price(prev)
        return out.cpu().numpy()

    def rl_sweep(self, prices, steps=None, hold=False):
        """The community's response to each of G candidate prices (scalars, or lists of
        action_horizon*dt values) over `rl.forecast_horizon` timesteps, all candidates solved together
        on device (`DeviceAggregator.sweep`): what G `rl_forecast` calls return, bit for bit, without
        their snapshots and restores.  Nothing is committed and `self.reward_price` stays.
        -> [G][steps][agg_load, forecast_load, agg_cost] on the host; the candidates' solve-path counts
        are in `self.dev.sweep_counts`.  hold=True: the candidates' solved first step is kept, and
        `rl_commit(g)` plays candidate g without solving it again."""
        steps = int(self.config["agg"]["rl"]["forecast_horizon"]) if steps is None else int(steps)
        steps = min(steps, self.num_timesteps - self.dev.timestep)
        rows = [self._price_list(p) for p in prices]
        if not rows:
            raise ValueError("rl_sweep needs at least one candidate price")
        noise_fn = self._noise if getattr(self, "noise_fn", None) else None
        if hold:
            out = self.dev.sweep(np.stack(rows), steps, noise_fn=noise_fn, hold=True)
            self._held_prices = rows
        else:
            out = self.dev.sweep(np.stack(rows), steps, noise_fn=noise_fn)
        return out.cpu().numpy()

    def rl_plan(self, keys=("p_grid",), rows=()):
        """The community's planned curves over the horizon, from the state the last step left
        (`DeviceAggregator.plan`): -> (curve [nk][H], count [nk][H], stats [nr][4]: count, sum, min, max) on the
        host, the keys and rows in ascending index order (`_lib.PLAN_KEYS`, `_lib.PLAN_ROWS`).  Entry 0 of a
        curve is the step's collected value (curve of p_grid: `agg_load`), entry j the homes' plan j stages
        ahead.  This is the OPEN-LOOP plan -- what the homes intend unless the price changes, read from arrays
        the solves already wrote, nothing solved -- not `rl_forecast`'s rollout, which re-solves the community
        step by step in closed loop under a frozen price."""
        return tuple(x[0].cpu().numpy() for x in self.dev.plan(keys, rows))

    def rl_sweep_plan(self, keys=("p_grid",), rows=()):
        """The planned curves of every candidate of the held sweep (`rl_sweep(..., hold=True)`;
        `DeviceAggregator.sweep_plan`): -> (curve [G][nk][H], count [G][nk][H], stats [G][nr][4]) on the host,
        each candidate's open-loop plan after its first step -- the price-response curve over the whole horizon
        where `rl_sweep` returns the first-step sums.  Open loop, as `rl_plan`: not what `rl_forecast` or a
        sweep of several steps computes.  ValueError when no sweep of the live state is held."""
        return tuple(x.cpu().numpy() for x in self.dev.sweep_plan(keys, rows))

    def rl_commit(self, g):
        """`rl_step` under candidate g of the held sweep (`rl_sweep(..., hold=True)`) with the solve replaced:
        the price is published, replica g's solved step adopted as this timestep (`DeviceAggregator.commit`,
        which installs the sweep's own price row: the live price ends as that row bit for bit), then
        collect and the new setpoint as in `rl_step`.  ValueError (nothing changed) when the sweep is not
        held any more or g is not one of its candidates."""
        if not self.dev.holds(g):
            raise ValueError(f"rl_commit({g}): no held sweep of the live state has that candidate")
        self._set_price(self._held_prices[int(g)])
        self.redis_set_current_values()
        self.dev.commit(int(g))
        self.timestep = self.dev.timestep
        return self.collect_data()

    def _play(self, action):
        """One timestep under a policy's return value: a `rl.Candidate` of a held sweep is committed
        (`rl_commit`), anything else -- or a candidate whose sweep is no longer held, logged once -- is
        solved under its price (`rl_step`)."""
        from .rl import Candidate
        if not isinstance(action, Candidate):
            return self.rl_step(action)
        if self.dev.holds(action.index):
            return self.rl_commit(action.index)
        if not getattr(self, "_warned_hold", False):
            self._warned_hold = True
            logging.getLogger(__name__).warning(
                "run_rl_agg: the policy returned a sweep candidate but the sweep is no longer held; "
                "solving the step under its price instead (rl_step)")
        return self.rl_step(action.price)

    # aggregator.py:898-911
    def test_response(self):
        c = self.config["agg"]["simplified"]["response_rate"]
        if self.timestep == 0:
            self.agg_load = self.agg_setpoint + 0.1 * self.agg_setpoint
        self.agg_load = self.agg_load - c * self.reward_price[0] * (self.agg_setpoint - self.agg_load)
        self.agg_cost = self.agg_load * self.reward_price[0]
        self.timestep += 1

    def run_rl_agg(self, policy, noise_fn=None):
        """The `run_rl_agg` case (README.md:55): MPC homes under an RL-designed reward price.
        `policy(aggregator) -> reward price` is called once per timestep (e.g. an
        `dragg_amd.rl.SetpointAgent.act`, or the reference's agent via `rl.policy_from_agent`);
        it may call `rl_forecast` to try a candidate price, or `rl_sweep` to try several at once; after
        `rl_sweep(..., hold=True)` it may return a `rl.Candidate` instead, which is played by adopting its
        already solved step (`rl_commit`).
        Writes `<run dir>/rl_agg/results.json` with the Summary's RP and p_grid_setpoint."""
        self.case = "rl_agg"
        self.get_homes()
        self.setup_rl_agg_run(noise_fn)
        for t in range(self.num_timesteps):
            self._play(policy(self))
            if (t + 1) % self.checkpoint_interval == 0:
                # the reference raises inside the step that fails (mpc_calc.py:280-289,
                # 537-539); checking at each checkpoint (one host sync) keeps post-error data
                # out of every results.json written
                self.dev.check_errors()
                self.write_outputs()
        self.dev.check_errors()
        self.check_solve_paths()
        self.write_ev_outputs()
        return self.write_outputs()

    def _history(self):
        """The checked homes' hash history [T][19][N] on rank 0.

        Incremental: each call brings over only the steps since the previous one (a checkpoint
        then costs its own rows, not the whole run again), as one tensor gather of the shards
        padded to a common width (NCCL on the device, gloo on the host) -- no pickling."""
        self.dev.drain()
        T = self.dev.timestep
        t0 = getattr(self, "_hist_rows", 0)
        if t0 == 0:
            self._hist_host = []
        if T > t0:
            new = self.dev.hist[t0:T]                      # [dT][19][n_local]
            if self.world == 1:
                self._hist_host.append(new.cpu().numpy())
            else:
                import torch
                import torch.distributed as dist
                n_all = len(self.checked)
                width = -(-n_all // self.world)            # the widest strided shard
                on_dev = dist.get_backend(self.group) == "nccl"
                src = new if on_dev else new.cpu()
                pad = torch.full(src.shape[:2] + (width,), float("nan"), dtype=src.dtype, device=src.device)
                pad[:, :, :src.shape[2]] = src
                parts = [torch.empty_like(pad) for _ in range(self.world)] if self.rank == 0 else None
                dist.gather(pad, parts, dst=0, group=self.group)
                if self.rank == 0:
                    out = np.empty(src.shape[:2] + (n_all,), dtype=np.float64)
                    for r, p in enumerate(parts):          # rank r holds homes r, r + world, ... (shard_index)
                        k = len(range(r, n_all, self.world))
                        out[:, :, r::self.world] = p[:, :, :k].cpu().numpy()
                    self._hist_host.append(out)
            self._hist_rows = T
        if self.rank != 0:
            return None
        if not self._hist_host:
            return np.empty((0, self.dev.hist.shape[1], len(self.checked)))
        if len(self._hist_host) > 1:
            self._hist_host = [np.concatenate(self._hist_host, axis=0)]
        return self._hist_host[0]

    # aggregator.py:783-844 (summarize_baseline + write_outputs)
    def write_outputs(self):
        with self._phase("history_gather"):
            hist = self._history()
        if self.rank != 0:
            return None
        t_diff = datetime.now() - self.start_time
        with self._phase("results_build"):
            # the RL case's list starts with setup_rl_agg_run's 0 (aggregator.py:887)
            loads = self.baseline_agg_load_list if "rl" in self.case else R.aggregate_loads(hist)
            self.max_agg_load = max(loads)
            self.max_agg_load_list.append(self.max_agg_load)
            summary = R.summary(
                self.case, self.start_dt, self.end_dt, t_diff.total_seconds(),
                self.config["home"]["hems"]["prediction_horizon"], self.config["community"]["total_number_homes"],
                loads, self.all_data.loc[self.mask, "OAT"].values.tolist(),
                self.all_data.loc[self.mask, "GHI"].values.tolist(), self.all_rps.tolist(), self.all_sps.tolist(),
                tou=self.all_data.loc[self.mask, "tou"].values.tolist())
            # the reference's collected_data dict (aggregator.py:589-615, 737-748) is built when read
            self._collected_src = (self.all_homes, self.checked, hist, summary)
            self._collected = None
        with self._phase("results_write"):
            # the same bytes as json.dump(collected_data, indent=4), straight from the history array
            if not hasattr(self, "_results_cache"):
                self._results_cache = {}
            return R.write_results_history(self.run_dir, self.case, self.all_homes, self.checked, hist, summary,
                                           cache=self._results_cache)

    @property
    def collected_data(self):
        """The reference's `collected_data` (per-home series + "Summary"), as of the last write_outputs."""
        if getattr(self, "_collected", None) is None and getattr(self, "_collected_src", None) is not None:
            homes, checked, hist, summary = self._collected_src
            c = R.new_collected(homes)
            R.append_history(c, checked, hist)
            c["Summary"] = summary
            self._collected = c
        return getattr(self, "_collected", None)

    # aggregator.py:941-970
    def run(self, noise_fn=None, resume=False, stop_after=None):
        sim = self.config["simulation"]
        self.checkpoint_interval = R.checkpoint_interval(sim["checkpoint_interval"], self.dt)
        self.version = sim["named_version"]
        hems = self.config["home"]["hems"]
        self.run_dir = R.run_dir(self.outputs_dir, self.start_dt, self.end_dt, self.check_type,
                                 self.config["community"]["total_number_homes"], hems["prediction_horizon"],
                                 self.dt_interval, hems["sub_subhourly_steps"], hems["solver"], self.version)
        if sim["run_rbo_mpc"]:
            self.case = "baseline"
            with self._phase("flush"):
                self.flush()
            self.get_homes()
            self.run_baseline(noise_fn, resume=resume, stop_after=stop_after)
            if stop_after is not None and self.timestep < self.num_timesteps:
                return None
            self.write_ev_outputs()
            return self.write_outputs()
        if sim.get("run_rl_agg"):
            if resume or stop_after is not None:
                # the RL loop's state (the agent, the setpoint history, all_rps / all_sps) is not
                # checkpointed: a resumed RL run would silently start over
                raise ValueError("resume / stop_after are supported on the run_rbo_mpc case only")
            from .rl import agent_policy
            return self.run_rl_agg(agent_policy(self), noise_fn)
        return None


def main():
    """`python -m dragg_amd.runner`; under torchrun (WORLD_SIZE > 1) one rank per GPU over RCCL."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
        try:
            Aggregator().run()
        finally:
            dist.destroy_process_group()
    else:
        Aggregator().run()


if __name__ == "__main__":
    main()
