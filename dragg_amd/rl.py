"""RL reward-price policies, host side.

The north star keeps the agent on the host: a policy is a few flops per timestep against a
community solve of 10^4-10^5 homes on the GPU.  What a policy needs from the community -- the
aggregate load, its forecast, the setpoint and candidate-price rollouts -- comes from
`dragg_amd.runner.Aggregator` (`rl_step`, `rl_forecast`, `rl_sweep`, `collect_data`), i.e. from
device-resident solves; `rl_sweep` solves G candidate prices in one grouped launch (`SweepAgent`).
`VectorEnv` (`Aggregator.rl_vector`) steps E independent episodes of the community as one batch, each
with its own seed, start index, clock and price, for policies that learn over many episodes
(`SetpointAgent.train_vector`).  `DeviceVectorEnv` (`Aggregator.rl_vector(E, device_env=True)`) is the same
environment with its state, observations, done flags and choices kept on the device, for policies that are
device code themselves (`SetpointAgent.act_device`, `SweepAgent.act_device`): no step or reset synchronises.
With `plan_keys` its observations also hold the community's planned curves over the horizon per episode (the
open-loop plan the last solves left on the device, one more launch per step).

The reference's learning agent (`dragg/agent.py`, an abstract actor-critic whose
`calc_state` / `reward` are left to a subclass and which no driver of v1 calls) is out of
scope and is NOT restated here.  It plugs in unchanged through
`policy_from_agent`: any object with the reference agent's `train(env) -> action` method
becomes a `policy(aggregator) -> reward price` for `Aggregator.run_rl_agg`, the aggregator
itself being the `env` it reads.

`SetpointAgent` is this build's own default policy (parity unpinned: the reference ships
none): a discrete PI controller on the relative forecast error against the aggregator's
setpoint (`gen_setpoint`, aggregator.py:677-696), clipped to `rl.utility.action_space`.
"""
from collections import namedtuple

import numpy as np

from ._lib import episode_mask

# What a policy may return instead of a price after `rl_sweep(..., hold=True)`: candidate `index` of that
# sweep, to be played by adopting its solved step (`Aggregator.rl_commit`), and its `price` (what
# `rl_step` takes), played the ordinary way if the sweep is no longer held.
Candidate = namedtuple("Candidate", ["index", "price"])


def setpoint_update(state, timestep, agg_load, max_poss_load, prev_timesteps):
    """`Aggregator.gen_setpoint`'s rule (aggregator.py:677-696), once, for the runner and for every
    episode of a `VectorEnv`.  `state` is (tracked_loads, max_load, min_load) of the previous call, or
    None before the first; at timestep < 2 the tracked loads start over at half the community's maximum
    possible load, later the oldest makes room for `agg_load`.  -> (tracked_loads, max_load, min_load,
    avg_load); the setpoint is avg_load.  `prev_timesteps` is read only when the loads start over."""
    if timestep < 2 or state is None:
        tracked = [0.5 * max_poss_load] * prev_timesteps
        max_load, min_load = -float("inf"), float("inf")
    else:
        tracked, max_load, min_load = state
        tracked[:-1] = tracked[1:]
        tracked[-1] = agg_load
    avg_load = np.average(tracked)
    if agg_load > max_load or timestep % 24 == 0:
        max_load = agg_load
    if agg_load < min_load or timestep % 24 == 0:
        min_load = agg_load
    return tracked, max_load, min_load, avg_load


def policy_from_agent(agent, scale=1.0):
    """Wrap a reference-style agent (`train(env) -> action`, agent.py:130-149) as the policy
    `run_rl_agg` calls once per timestep: reward price = action / scale."""
    def policy(aggregator):
        return float(agent.train(aggregator)) / scale
    return policy


class SetpointAgent:
    """Action = kp e + ki Σ e clipped to the action space, e = (forecast - setpoint) /
    setpoint: a forecast above the setpoint raises the reward price (which the homes add to
    TOU, mpc_calc.py:353).  The integral term is clamped to the action space (anti-windup).
    `config["rl"]["utility"]["action_space"]` is required (KeyError, like the reference's agent
    at agent.py:75); `action_scale` maps actions to $/kWh."""

    name = "setpoint"

    def __init__(self, config, kp=1.0, ki=0.1):
        util = config["rl"]["utility"]
        lo, hi = util["action_space"]
        self.lo, self.hi = float(lo), float(hi)
        self.scale = float(util.get("action_scale", 100.0))
        self.kp, self.ki = float(kp), float(ki)
        self.integral = 0.0
        self.history = {"error": [], "action": []}

    def error(self, env):
        sp = env.agg_setpoint if env.agg_setpoint else 1.0
        return (env.forecast_load - sp) / sp

    def train(self, env):
        e = self.error(env)
        if self.ki:
            self.integral = float(np.clip(self.integral + e, self.lo / self.ki, self.hi / self.ki))
        a = float(np.clip(self.kp * e + self.ki * self.integral, self.lo, self.hi))
        self.history["error"].append(e)
        self.history["action"].append(a)
        return a

    def act(self, env):
        """policy(aggregator) -> reward price for `Aggregator.run_rl_agg`."""
        return self.train(env) / self.scale

    def train_vector(self, env_obs):
        """`train` for the E episodes of a `VectorEnv` at once: E independent PI states (`integral_v`),
        each exactly the scalar controller on its episode's observation.  `env_obs`: the environment's
        observations (`forecast_load` and `agg_setpoint`, [E] each).  -> actions [E]."""
        f = np.asarray(env_obs["forecast_load"], dtype=float)
        s = np.asarray(env_obs["agg_setpoint"], dtype=float)
        sp = np.where(s != 0, s, 1.0)
        e = (f - sp) / sp
        if getattr(self, "integral_v", None) is None or len(self.integral_v) != len(e):
            self.integral_v = np.zeros(len(e))
        if self.ki:
            self.integral_v = np.clip(self.integral_v + e, self.lo / self.ki, self.hi / self.ki)
        a = np.clip(self.kp * e + self.ki * self.integral_v, self.lo, self.hi)
        self.history["error"].append(e.tolist())
        self.history["action"].append(a.tolist())
        return a

    def reset_vector(self, mask=None):
        """Clear the PI state of the masked episodes (default: all), e.g. when they start over."""
        if getattr(self, "integral_v", None) is not None:
            self.integral_v = np.where(np.ones(len(self.integral_v), bool) if mask is None
                                       else np.asarray(mask, dtype=bool), 0.0, self.integral_v)

    def act_vector(self, env_obs):
        """Observations -> reward prices [E] for `VectorEnv.step`."""
        return self.train_vector(env_obs) / self.scale

    def train_device(self, env_obs, history=True):
        """`train_vector` on device tensors (the observations of a `DeviceVectorEnv`), as float64 elementwise
        torch ops -- every arithmetic step an op of its own, so that nothing is contracted and the actions
        equal `train_vector`'s bit for bit.  The PI state (`integral_d`) stays on the device; history=True
        appends the errors and actions to `history_device` as device tensors.  -> actions, device [E]."""
        import torch
        f, s = env_obs["forecast_load"], env_obs["agg_setpoint"]
        sp = torch.where(s != 0, s, torch.ones_like(s))
        e = f - sp
        e = e / sp
        if getattr(self, "integral_d", None) is None or self.integral_d.shape != e.shape \
                or self.integral_d.device != e.device:
            self.integral_d = torch.zeros_like(e)
        if self.ki:
            self.integral_d = torch.clamp(self.integral_d + e, self.lo / self.ki, self.hi / self.ki)
        p = self.kp * e
        i = self.ki * self.integral_d
        a = torch.clamp(p + i, self.lo, self.hi)
        if history:
            if getattr(self, "history_device", None) is None:
                self.history_device = {"error": [], "action": []}
            self.history_device["error"].append(e)
            self.history_device["action"].append(a)
        return a

    def reset_device(self, mask=None):
        """Clear the device PI state of the masked episodes (`mask`: a device bool [E]; default: all)."""
        import torch
        if getattr(self, "integral_d", None) is not None:
            zero = torch.zeros_like(self.integral_d)
            self.integral_d = zero if mask is None else torch.where(mask, zero, self.integral_d)

    def act_device(self, env_obs, history=True):
        """Device observations -> reward prices, device [E], for `DeviceVectorEnv.step`.  (The divisor is a
        tensor: torch divides a device tensor by a Python scalar as a multiplication by its reciprocal, which
        is not `act_vector`'s division in the last bit.)"""
        import torch
        a = self.train_device(env_obs, history)
        return a / torch.full_like(a, self.scale)


def _path_weights(K, weights):
    """The K step weights of a lookahead score as host doubles (None: ones)."""
    if weights is None:
        return np.ones(K)
    w = np.asarray(weights.cpu() if hasattr(weights, "cpu") else weights, dtype=float).reshape(-1)
    if len(w) != K:
        raise ValueError(f"a lookahead of {K} steps takes {K} weights, not {len(w)}")
    return w


def _env_head(env, va, config, max_poss_load, n_homes):
    """What the two vector environments' constructors share: the aggregator, its shape and price classes, and the
    setpoint rule's constants."""
    from . import inputs as I
    env.va, env.config = va, config
    env.E, env.T = va.E, va.num_timesteps
    # price classes (the aggregator's `price_classes`): actions are then [E][P] or [E][P][n], candidates
    # [E][C][P] or [E][C][P][n]
    env.n_classes, env.class_names = getattr(va, "n_classes", 1), getattr(va, "class_names", None)
    env.prev_timesteps = config["agg"]["rl"]["prev_timesteps"]
    # (an aggregator with vehicles: each vehicle's max_rate on top of the homes' own loads)
    env.max_poss_load = (sum(I.max_load(h) for h in va.homes) + getattr(va, "vehicle_max_rate", 0.0)
                         if max_poss_load is None else max_poss_load)
    env.n_homes = va.Nb if n_homes is None else int(n_homes)


class VectorEnv:
    """E episodes of one community as a vector environment for reward-price policies, on a
    `dragg_amd.vector.VectorAggregator`.

    reset() -> observations; step(actions [E] or [E][n]: each episode's reward price in $/kWh) ->
    (observations, done [E]).  An observation holds, per episode ([E] numpy arrays): `agg_load`,
    `forecast_load`, `agg_cost` (collect_data's sums of its last step), `agg_setpoint` and `timestep`.
    The setpoint is `Aggregator.gen_setpoint`'s rule (`setpoint_update`: tracked loads,
    `agg.rl.prev_timesteps`, the community's maximum possible load), kept per episode in the order of
    `Aggregator.setup_rl_agg_run` / `rl_step`.  An episode that has run its `num_timesteps` steps is done
    and sits idle until it is reset (`reset(mask)`); parked episodes sit idle too.  The three sums come to
    the host once per step (the policies are host code)."""

    def __init__(self, vector_aggregator, config, max_poss_load=None, n_homes=None):
        _env_head(self, vector_aggregator, config, max_poss_load, n_homes)
        self.timestep = np.zeros(self.E, dtype=np.int64)
        self.parked = np.zeros(self.E, dtype=bool)
        self.agg_load = np.zeros(self.E)
        self.forecast_load = np.zeros(self.E)
        self.agg_cost = np.zeros(self.E)
        self.agg_setpoint = np.zeros(self.E)
        self._sp = [None] * self.E
        self.scores = None

    def _host_mask(self, mask):
        return np.asarray(episode_mask(mask.cpu() if hasattr(mask, "cpu") else mask, self.E))

    def _setpoint(self, e):
        st = setpoint_update(self._sp[e], int(self.timestep[e]), float(self.agg_load[e]), self.max_poss_load,
                             self.prev_timesteps)
        self._sp[e] = st[:3]
        self.agg_setpoint[e] = st[3]

    def observations(self):
        return {"agg_load": self.agg_load.copy(), "forecast_load": self.forecast_load.copy(),
                "agg_cost": self.agg_cost.copy(), "agg_setpoint": self.agg_setpoint.copy(),
                "timestep": self.timestep.copy()}

    def reset(self, mask=None, seeds=None, start_indices=None):
        """Start the masked episodes (default: all) over, as `setup_rl_agg_run` starts a run: the load
        and its forecast at 3 kW per home of the community, the setpoint from fresh tracked loads."""
        m = self._host_mask(mask)
        self.va.reset(None if mask is None else m, seeds=seeds, start_indices=start_indices)
        for e in np.flatnonzero(m):
            self.timestep[e] = 0
            self.parked[e] = False
            self.forecast_load[e] = self.agg_load[e] = 3 * self.n_homes
            self.agg_cost[e] = 0.0
            self._sp[e] = None
            self._setpoint(e)
        return self.observations()

    def park(self, mask):
        m = self._host_mask(mask)
        self.va.park(m)
        self.parked |= m

    def resume(self, mask):
        m = self._host_mask(mask)
        self.va.resume(m)
        self.parked &= ~m

    def done(self):
        return self.timestep >= self.T

    def step(self, actions):
        """Publish each episode's reward price, solve every active episode in one batch, collect, new
        setpoints (the order of `Aggregator.rl_step`).  -> (observations, done [E])."""
        on = ~self.parked & ~self.done()
        agg = self.va.step(actions).cpu().numpy()
        for e in np.flatnonzero(on):
            self.timestep[e] += 1
            self.agg_load[e], self.forecast_load[e], self.agg_cost[e] = agg[e]
            self._setpoint(e)
        return self.observations(), self.done()

    def step_swept(self, candidates, lookahead=1, weights=None):
        """`step` with the price chosen from C candidates per episode (`candidates` [E][C] or [E][C][n], $/kWh)
        instead of guessed: every candidate of every active episode is solved one step ahead in one batch
        (`VectorAggregator.sweep`), the one whose load lies closest to the episode's setpoint is chosen on
        the device (`select`: ties to the smaller |price|, then the smaller index) and its solved step
        adopted (`commit`) -- no second solve.  -> (observations, done [E]); `self.choice` holds the chosen
        indices ([E] numpy, -1: the episode took no step).

        lookahead = K > 1: every candidate is rolled K steps ahead (`sweep(steps=K)`) and scored over its load
        path, step j weighted by `weights[j]` (default: ones) against the setpoint this environment would hold
        by then had the candidate been played (`vector.select_paths_reference`, on the host here); the chosen
        candidate's FIRST step is adopted.  `self.scores` holds the scores ([E][C] numpy, NaN: none)."""
        on = ~self.parked & ~self.done()
        K = int(lookahead)
        if K > 1:
            import torch
            from .vector import select_paths_reference
            paths = self.va.sweep(candidates, steps=K).cpu().numpy()                  # [E][C][K][3]
            C = paths.shape[1]
            P = int(self.prev_timesteps)
            fresh = [0.5 * self.max_poss_load] * P
            if self.n_classes > 1:                   # (the tie rule's key over the classes, as the device path's)
                rows = self.va.tie_key(candidates, C).cpu().numpy().reshape(C, self.E, 1)
            else:
                rows = np.asarray(candidates.cpu() if hasattr(candidates, "cpu") else candidates, dtype=float) \
                    .reshape(self.E, C, -1).transpose(1, 0, 2)
            ch, score = select_paths_reference(
                paths.transpose(2, 1, 0, 3).reshape(K, C * self.E, 3), np.where(on, self.timestep, -1),
                [fresh if sp is None else sp[0] for sp in self._sp], self.agg_setpoint, _path_weights(K, weights),
                rows, self.T, self.max_poss_load)
            self.scores = score.reshape(C, self.E).T.copy()
            choice = torch.as_tensor(ch, dtype=torch.int32, device=self.va.device)
        else:
            sums = self.va.sweep(candidates)
            choice = self.va.select(sums, self.agg_setpoint, candidates)
        agg = self.va.commit(choice).cpu().numpy()
        adopted = self.va.adopted.cpu().numpy()
        self.choice = np.where(adopted, choice.cpu().numpy(), -1)
        for e in np.flatnonzero(on & adopted):
            self.timestep[e] += 1
            self.agg_load[e], self.forecast_load[e], self.agg_cost[e] = agg[e]
            self._setpoint(e)
        return self.observations(), self.done()


class DeviceVectorEnv:
    """`VectorEnv` with everything kept on the device: the same constructor arguments and methods, the same
    numbers bit for bit, but the work after a step's solve is one kernel (dragg_mpc_env_file: the history rows,
    the clocks, the setpoint rule and the observations) and a reset is one kernel over the restarted episodes'
    columns alone (dragg_mpc_env_reset).  No method synchronises with the host.

    Everything returned is a device tensor: `observations()` is a dict of [E] float64 VIEWS into one buffer
    (`timestep` too: exact in a double) -- a later step or reset overwrites them, so clone what must be kept;
    `done()` is a device bool [E]; `choice` (after `step_swept`) a device int32 [E].  `reset` and `park` take
    device masks (`env.reset(env.done())`), and `reset` takes `seeds` / `start_indices` as device tensors [E],
    used for the masked episodes without a host check: a start index outside the environment window leaves that
    episode idle.  Host lists are taken and checked as in `VectorEnv`.  `agg.rl.prev_timesteps` must lie in
    1..128.

    Plan observations (`plan_keys`, `plan_rows`: names of `_lib.PLAN_KEYS` / `_lib.PLAN_ROWS`; default none): every
    `reset`, `step` and `step_swept` then ends with one more launch (dragg_mpc_plan_groups) into buffers allocated
    once, and `observations()` gains `plan` [E][nk][H] -- per episode the community's planned curve of each key
    over the horizon, entry 0 the step's collected value, keys in ascending index order (`plan_key_names`) --,
    `plan_count` [E][nk][H] (int32: the homes behind each entry) and `plan_stats` [E][nr][4] (count, sum, min, max
    of each vals row), views like the others.  It is the open-loop plan of the episodes' last solves: a parked or
    finished episode keeps its last step's, a fresh one's is empty (count 0).  Without them the environment issues
    exactly the launches it issued before.

    Price classes (an aggregator built with `price_classes`; `n_classes`, `class_names`): actions are [E][P] or
    [E][P][n], candidates [E][C][P] or [E][C][P][n].  With plan keys or rows as well, one launch more per `reset`,
    `step` and `step_swept` (dragg_mpc_plan_classes) adds `class_plan` [E][P][nk][H], `class_plan_count` (int32)
    and `class_stats` [E][P][nr][4]: the plan observations per price class, the vector observation that answers a
    vector action.  Without classes the launches are exactly those above."""

    def __init__(self, vector_aggregator, config, max_poss_load=None, n_homes=None, plan_keys=(), plan_rows=()):
        from . import _lib as L
        _env_head(self, vector_aggregator, config, max_poss_load, n_homes)
        va = self.va
        self.state = va.env_state(self.prev_timesteps, self.max_poss_load, 3 * self.n_homes)
        self.choice = self.scores = None
        self._w = {}
        _, _, ki, ri = L.plan_select(plan_keys, plan_rows)
        self.plan_key_names, self.plan_row_names = [L.PLAN_KEYS[k] for k in ki], [L.PLAN_ROWS[r] for r in ri]
        self._plan = self._class_plan = None
        if ki or ri:
            import torch
            curve, stats = L.plan_shape(ki, ri, self.E, va.H)
            self._plan = (torch.zeros(curve, dtype=torch.float64, device=va.device),
                          torch.zeros(curve, dtype=torch.int32, device=va.device),
                          torch.zeros(stats, dtype=torch.float64, device=va.device))
            if self.n_classes > 1:
                curve, stats = ((s[0], self.n_classes) + s[1:] for s in (curve, stats))
                self._class_plan = (torch.zeros(curve, dtype=torch.float64, device=va.device),
                                    torch.zeros(curve, dtype=torch.int32, device=va.device),
                                    torch.zeros(stats, dtype=torch.float64, device=va.device))

    def _observe_plan(self):
        if self._plan is not None:
            self.va.plan(self.plan_key_names, self.plan_row_names, out=self._plan)
        if self._class_plan is not None:
            self.va.plan(self.plan_key_names, self.plan_row_names, out=self._class_plan, classes=True)

    def observations(self):
        from ._lib import OBS_KEYS
        obs = {k: self.state.obs[i] for i, k in enumerate(OBS_KEYS)}
        if self._plan is not None:
            obs["plan"], obs["plan_count"], obs["plan_stats"] = self._plan
        if self._class_plan is not None:
            obs["class_plan"], obs["class_plan_count"], obs["class_stats"] = self._class_plan
        return obs

    def reset(self, mask=None, seeds=None, start_indices=None):
        self.va.reset_env(self.state, mask, seeds=seeds, start_indices=start_indices)
        self._observe_plan()
        return self.observations()

    def park(self, mask):
        self.va.park(mask)

    def resume(self, mask):
        self.va.resume(mask)

    def done(self):
        return self.va.done()

    def step(self, actions):
        """-> (observations, done [E]), as `VectorEnv.step`."""
        self.va.step_env(self.state, actions)
        self._observe_plan()
        return self.observations(), self.done()

    def _weights(self, K, weights):
        """The K step weights as a device tensor: a device tensor as it is, a host list (None: ones) uploaded
        once and cached per (K, device)."""
        import torch
        dev = self.va.device
        if torch.is_tensor(weights) and weights.device == dev:
            return weights
        vals = None if weights is None else tuple(_path_weights(K, weights).tolist())
        hit = self._w.get((K, dev))
        if hit is None or hit[0] != vals:
            hit = self._w[(K, dev)] = (vals, torch.ones(K, dtype=torch.float64, device=dev) if vals is None
                                       else torch.tensor(vals, dtype=torch.float64).to(dev))
        return hit[1]

    def step_swept(self, candidates, lookahead=1, weights=None):
        """-> (observations, done [E]), as `VectorEnv.step_swept`; the setpoints go to `select` from the device.
        lookahead = K > 1: the K-step rollouts are scored and the choice made by one kernel
        (`VectorAggregator.select_paths`) from the tracked loads, setpoints and clocks where they live;
        `self.scores` is a device view [E][C] (overwritten by the next call), bit for bit `VectorEnv`'s."""
        import torch
        va = self.va
        K = int(lookahead)
        if K > 1:
            paths = va.sweep(candidates, steps=K)
            choice = va.select_paths(paths, self.state.tracked, self.state.obs[3], candidates,
                                     self._weights(K, weights), self.max_poss_load)
            self.scores = va.path_scores
        else:
            sums = va.sweep(candidates)
            choice = va.select(sums, self.state.obs[3], candidates)
        va.commit_env(self.state, choice)
        self.choice = torch.where(va.adopted, choice, torch.full_like(choice, -1))
        self._observe_plan()
        return self.observations(), self.done()


class SweepAgent:
    """Evaluates the price-response curve instead of guessing it: `n_candidates` actions evenly
    spaced over `rl.utility.action_space` (divided by `action_scale`: $/kWh) are all solved ahead
    in one grouped launch (`env.rl_sweep`, DeviceAggregator.sweep), and the price whose first
    forecast step's aggregate load lies closest to `env.agg_setpoint` is played; ties go to the
    smaller |price|.  `history` keeps every step's candidates, their responses (the first step's
    aggregate load per candidate) and the choice.  commit=True (`rl.parameters.commit`): the sweep is held
    and `act` returns a `Candidate`, so that `run_rl_agg` plays the chosen candidate by adopting its solved
    step instead of solving it again (`Aggregator.rl_commit`; the results are the same bit for bit).
    lookahead = K > 1 (`rl.parameters.lookahead`): every candidate is rolled K steps ahead and scored over its
    load path, step j weighted by discount**j (`rl.parameters.discount`) against the setpoint `gen_setpoint`
    would hold by then had it been played -- the rule of the vector environments' `step_swept(lookahead=K,
    weights=agent.weights())`; `history["score"]` keeps the scores.  The first step is what is played."""

    name = "sweep"

    def __init__(self, config, n_candidates=8, commit=False, lookahead=1, discount=1.0):
        self.commit = bool(commit)
        self.lookahead, self.discount = max(1, int(lookahead)), float(discount)
        self.index = None
        util = config["rl"]["utility"]
        lo, hi = util["action_space"]
        self.lo, self.hi = float(lo), float(hi)
        self.scale = float(util.get("action_scale", 100.0))
        self.n = max(1, int(n_candidates))
        self.history = {"candidates": [], "response": [], "action": []}

    def candidates(self):
        return np.clip(np.linspace(self.lo, self.hi, self.n), self.lo, self.hi)

    def weights(self):
        """The step weights of the lookahead score, discount**j for j < lookahead (what a caller hands
        `step_swept(candidates, lookahead=agent.lookahead, weights=agent.weights())`)."""
        return [self.discount ** j for j in range(self.lookahead)]

    def _train_ahead(self, env, prices):
        """`train`'s choice with lookahead > 1: the candidates rolled `lookahead` steps ahead
        (`rl_sweep(prices, steps=K)`) and scored by the vector environments' rule (`select_paths_reference`, one
        episode) on the runner's own `gen_setpoint` state.  -> (index, first-step loads), or None when the run has
        no step left (the caller's tie rule decides)."""
        from .vector import select_paths_reference
        resp = np.asarray(env.rl_sweep(prices, steps=self.lookahead, hold=self.commit), dtype=float)   # [C][k][3]
        k = resp.shape[1]
        if not k:
            return None
        choice, score = select_paths_reference(
            resp.transpose(1, 0, 2), [int(env.timestep)], [list(env.tracked_loads)], [float(env.agg_setpoint)],
            self.weights()[:k], np.asarray(prices).reshape(len(prices), 1), env.num_timesteps, env.max_poss_load)
        self.history.setdefault("score", []).append(score.tolist())
        return int(choice[0]), resp[:, 0, 0]

    def train(self, env):
        acts = self.candidates()
        prices = [float(a) / self.scale for a in acts]
        ahead = self._train_ahead(env, prices) if self.lookahead > 1 else None
        if ahead is not None and ahead[0] >= 0:
            best, load = ahead
            return self._chosen(acts, load, best)
        resp = np.asarray(env.rl_sweep(prices, hold=True) if self.commit else env.rl_sweep(prices), dtype=float)
        load = resp[:, 0, 0] if resp.shape[1] else np.zeros(len(acts))   # (no step left in the run: all tie)
        sp = float(env.agg_setpoint)
        best = min(range(len(acts)), key=lambda i: (abs(load[i] - sp), abs(acts[i])))
        return self._chosen(acts, load, best)

    def _chosen(self, acts, load, best):
        a = float(np.clip(acts[best], self.lo, self.hi))
        self.index = best
        self.history["candidates"].append(acts.tolist())
        self.history["response"].append(load.tolist())
        self.history["action"].append(a)
        return a

    def act(self, env):
        """policy(aggregator) -> reward price for `Aggregator.run_rl_agg` (commit=True: the `Candidate`)."""
        p = self.train(env) / self.scale
        return Candidate(self.index, p) if self.commit else p

    def act_vector(self, env_obs, classes=None):
        """Observations of a `VectorEnv` -> candidate prices [E][C] for `VectorEnv.step_swept` (every episode
        the same `candidates()`).  classes=P (an environment with P price classes): [E][C][P], every class
        getting the same grid value -- the class path driven by this policy, the uniform prices it would play."""
        E = len(np.asarray(env_obs["agg_setpoint"]).reshape(-1))
        c = np.tile(self.candidates() / self.scale, (E, 1))
        return c if classes is None else np.repeat(c[:, :, None], int(classes), axis=2)

    def act_device(self, env_obs, classes=None):
        """`act_vector` for a `DeviceVectorEnv`: the tiled candidates as a device tensor [E][C], or [E][C][P]
        with classes=P (built once per shape and device)."""
        import torch
        s = env_obs["agg_setpoint"]
        key = (int(s.numel()), s.device, classes)
        if getattr(self, "_tiled", None) is None or self._tiled[0] != key:
            self._tiled = (key, torch.as_tensor(self.act_vector({"agg_setpoint": np.zeros(key[0])}, classes),
                                                dtype=torch.float64).to(s.device))
        return self._tiled[1]


def agent_policy(aggregator):
    """The policy a `run_rl_agg = true` config runs with: `SetpointAgent`, its gains from the keys of
    its own, `rl.parameters.kp` (default 1.0) and `rl.parameters.ki` (default 0.1).  The reference's
    `rl.parameters.learning_rate` (README.md:58-63) is a learning agent's step size, not a controller
    gain: it is left to an agent wrapped by `policy_from_agent`.  `rl.parameters.policy = "sweep"`
    selects `SweepAgent` instead, with `rl.parameters.candidates` (default 8) candidate prices;
    `rl.parameters.commit = true` makes it play the chosen candidate by adopting its solved step;
    `rl.parameters.lookahead` (default 1: one step ahead) and `rl.parameters.discount` (default 1.0) make it
    score the candidates over that many steps."""
    p = aggregator.config.get("rl", {}).get("parameters", {}) or {}
    if p.get("policy") == "sweep":
        return SweepAgent(aggregator.config, n_candidates=int(p.get("candidates", 8)),
                          commit=bool(p.get("commit", False)), lookahead=int(p.get("lookahead", 1)),
                          discount=float(p.get("discount", 1.0))).act
    return SetpointAgent(aggregator.config, kp=float(p.get("kp", 1.0)), ki=float(p.get("ki", 0.1))).act
