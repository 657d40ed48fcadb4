"""Vectorised episodes: E independent runs of one community stepped as one batch.

An RL agent that sets the reward price of a small community (the reference's configs[0]: 20 homes) lives
through many episodes, and a step of 20 homes costs about what a step of 1,000 does: a step is never shorter
than its slowest home's dependent chain of DP stages.  `VectorAggregator` therefore holds E episodes of the
community in ONE grouped `MPCBatch(groups=E)` and steps them together with `dragg_mpc_step_episodes`
(include/dragg_mi355x.h): episode e has its own season-noise seed, its own start index into the environment
lists, its own clock and its own reward-price row, and its state persists in its columns of the hash arrays.
Every episode equals, bit for bit, a single `DeviceAggregator` run with that seed, start index and price
trajectory.

The seeds, start indices and clocks live on the device and the kernels read them there: a step, a reset, a
park or a resume never synchronises with the host.  Only the accessors that hand rows to the host
(`episode_history`, `episode_status`, `episode_paths`, `approx_counts`, `check_errors`, `clocks_host`) do.

`step_env`, `commit_env` and `reset_env` are `step`, `commit` and `reset` for a device-resident environment
(`rl.DeviceVectorEnv`): the same solve, then ONE kernel that files the rows, advances the clocks and keeps the
environment's setpoint state and observations (dragg_mpc_env_file), and one kernel that starts the masked
episodes over by writing their columns alone (dragg_mpc_env_reset).  `env_file_reference` and
`env_reset_reference` restate the two kernels on numpy arrays for the tests.

`sweep(prices, steps=K)` rolls every candidate of every episode K steps ahead as one grouped batch and
`select_paths` scores the K-step load paths against the setpoints the environment's rule would file along them
(dragg_mpc_select_paths; `select_paths_reference` restates it), so that a policy sees a price's rebound before it
plays the first step.

`plan` reduces the plans the episodes' last solves left in the hash arrays to per-episode horizon curves
(dragg_mpc_plan_groups; `plan_groups_reference` restates it, summation order included).

`VectorAggregator(..., price_classes=...)` gives every home of the community a price class: an action is then a
price per class ([E][P]), every home reads its class's row (dragg_mpc_step_classes) and `plan(classes=True)`
reduces the plans per (episode, class) (dragg_mpc_plan_classes; `plan_classes_reference` restates it).  The
class-c homes of an episode equal, bit for bit, the same homes of a single run under class c's prices alone.

`VectorAggregator(..., vehicles=True)` steps the homes' electric vehicles beside them: an E-group `EVFleet` of its
own whose groups follow the episodes' start indices, clocks, resets, price rows and price classes
(dragg_mpc_ev_step_episodes), its three sums added onto the homes' before anything is filed, swept and adopted with
the homes.  The batch and the fleet are one unit here (`members.Members`, DESIGN.md section
3.15): the live state is one, every sweep's replicas are one, a held first step is a `members.Held`, and each move
of the state -- prices, step, sums, replicate, adopt, the fleet's reset -- is one call on it, homes first.  The
homes never see the fleet: their rows are those of the same aggregator
without vehicles, and every episode's sums and fleet state are a single `DeviceAggregator(ev=...)` run's, bit for bit.

One rank only: sharding episodes over ranks is not built.
"""
import numpy as np
import torch

from . import _lib as L
from .ev import EVFleet
from .members import Held, Members
from .mpc import MPCBatch


def _seed_i64(s):
    """A uint64 seed as the int64 with the same bits (the tensors are int64)."""
    s = int(s) & (2 ** 64 - 1)
    return s - 2 ** 64 if s >= 2 ** 63 else s


class EnvState:
    """What a device-resident environment keeps per episode beside the aggregator's own arrays (the members of
    dragg_mpc_env, include/dragg_mi355x.h): the setpoint rule's tracked loads [E][P] (oldest first), max_load
    and min_load [E], and the observations [5][E] (rows: L.OBS_KEYS).  The clocks and the history stores are
    the aggregator's, looked up when a call is made (its host-driven methods rebind `clocks`)."""

    def __init__(self, va, prev_timesteps, max_poss_load, start_load):
        P = int(prev_timesteps)
        if not 1 <= P <= L.ENV_PREV_MAX:
            raise ValueError(f"prev_timesteps must lie in 1..{L.ENV_PREV_MAX} for a device-resident environment, "
                             f"not {prev_timesteps!r}")
        self.va = va
        self.num_timesteps, self.prev_timesteps = va.num_timesteps, P
        self.max_poss_load, self.start_load = float(max_poss_load), float(start_load)
        dev, E = va.device, va.E
        self.tracked = torch.zeros((E, P), dtype=torch.float64, device=dev)
        self.max_load = torch.full((E,), -float("inf"), dtype=torch.float64, device=dev)
        self.min_load = torch.full((E,), float("inf"), dtype=torch.float64, device=dev)
        self.obs = torch.zeros((len(L.OBS_KEYS), E), dtype=torch.float64, device=dev)

    clock = property(lambda self: self.va.clocks)
    status_hist = property(lambda self: self.va.status_hist)
    path_hist = property(lambda self: self.va.path_hist)
    hist = property(lambda self: self.va.hist)
    agg_hist = property(lambda self: self.va.agg_hist)

    def host(self):
        """The arrays as numpy, for the restatements below (CPU tensors: views that share their memory)."""
        out = {k: getattr(self, k) for k in ("num_timesteps", "prev_timesteps", "max_poss_load", "start_load")}
        for k in ("clock", "tracked", "max_load", "min_load", "obs", "status_hist", "path_hist", "hist", "agg_hist"):
            t = getattr(self, k)
            out[k] = None if t is None else t.cpu().numpy()
        return out


def env_file_reference(env, ran, sums, status=None, int_path=None, row=None):
    """dragg_mpc_env_file restated on numpy arrays, in place (the spec its tests share, and what a stand-in
    batch serves `env_file` with -- not a solver fallback).  `env`: `EnvState.host()`'s dict; `ran` [G], `sums`
    [G][3], `status` / `int_path` [N], `row` [NVAL][N].  Group g with 0 <= ran[g] < T: its Nb columns of the
    sources filed at row ran[g] of the stores, clock ran[g] + 1, then `VectorEnv.step`'s bookkeeping with
    `rl.setpoint_update` itself; any other group: nothing written."""
    from .rl import setpoint_update
    G = len(ran)
    for g in range(G):
        t = int(ran[g])
        if t < 0 or t >= env["num_timesteps"]:
            continue
        for store, src in ((env["status_hist"], status), (env["path_hist"], int_path), (env["hist"], row)):
            if store is not None and src is not None:
                Nb = store.shape[-1] // G
                store[t, ..., g * Nb:(g + 1) * Nb] = src[..., g * Nb:(g + 1) * Nb]
        if env["agg_hist"] is not None:
            env["agg_hist"][t, g] = sums[g]
        ts = t + 1
        env["clock"][g] = ts
        load = float(sums[g][0])
        tracked, mx, mn, avg = setpoint_update((env["tracked"][g].tolist(), float(env["max_load"][g]),
                                                float(env["min_load"][g])), ts, load, env["max_poss_load"],
                                               env["prev_timesteps"])
        env["tracked"][g] = tracked
        env["max_load"][g], env["min_load"][g] = mx, mn
        env["obs"][:, g] = (load, sums[g][1], sums[g][2], avg, ts)


def env_reset_reference(env, mask, vals, fc):
    """dragg_mpc_env_reset restated on numpy arrays, in place: for each masked group, its columns of `vals`
    ([NVAL][N]) and its homes' blocks of `fc` ([N][NFC][H]) NaN, its columns of every store cleared, clock 0,
    and the state `VectorEnv.reset` leaves (through `rl.setpoint_update` itself)."""
    from .rl import setpoint_update
    G = len(mask)
    Nb = vals.shape[-1] // G
    for g in range(G):
        if not mask[g]:
            continue
        cols = slice(g * Nb, (g + 1) * Nb)
        vals[:, cols] = np.nan
        fc[cols] = np.nan
        if env["hist"] is not None:
            env["hist"][..., cols] = np.nan
        env["status_hist"][:, cols] = 0
        if env["path_hist"] is not None:
            env["path_hist"][:, cols] = 0
        if env["agg_hist"] is not None:
            env["agg_hist"][:, g] = 0.0
        env["clock"][g] = 0
        load = env["start_load"]
        tracked, mx, mn, avg = setpoint_update(None, 0, load, env["max_poss_load"], env["prev_timesteps"])
        env["tracked"][g] = tracked
        env["max_load"][g], env["min_load"][g] = mx, mn
        env["obs"][:, g] = (load, load, 0.0, avg, 0)


def select_paths_reference(sums, ran, tracked, target, weights, prices, num_timesteps, max_poss_load, setpoints=None):
    """dragg_mpc_select_paths restated on numpy arrays (the spec its tests share, the scoring of the host
    `rl.VectorEnv` and of `SweepAgent.train`, and what a stand-in batch serves `select_paths` with -- not a
    solver fallback).  `sums` [K][C * E][3] (copy-major groups c * E + e), `ran` [E], `tracked` [E][P], `target`
    [E], `weights` [K], `prices` [C * E][n] -> (choice int32 [E], score float64 [C * E]).  Candidate c of episode
    e is scored over its k = min(K, T - ran[e]) steps against the setpoints `rl.setpoint_update` itself returns
    when the candidate's loads are played on a copy of the episode's tracked loads; `setpoints` (a dict, for the
    tests) receives the list [s_0 .. s_(k-1)] per (e, c) that was scored to its end.  Nothing given is written."""
    from .rl import setpoint_update
    sums = np.asarray(sums, dtype=np.float64)
    K, CE = sums.shape[0], sums.shape[1]
    E = len(ran)
    C, T = CE // E, int(num_timesteps)
    tracked = np.asarray(tracked, dtype=np.float64).reshape(E, -1)
    P = tracked.shape[1]
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    prices = np.asarray(prices, dtype=np.float64).reshape(CE, -1)
    choice, score = np.full(E, -1, dtype=np.int32), np.full(CE, np.nan)
    for e in range(E):
        t = int(ran[e])
        k = min(K, T - t) if 0 <= t < T else 0
        best, bd, bp = -1, 0.0, 0.0
        for c in range(C if k > 0 else 0):
            g = c * E + e
            state = (tracked[e].tolist(), -float("inf"), float("inf"))
            s, acc, sps = np.float64(target[e]), np.float64(0.0), []
            for j in range(k):
                load = sums[j, g, 0]
                if load != load:
                    acc = None
                    break
                if j > 0:
                    *state, s = setpoint_update(state, t + j, float(sums[j - 1, g, 0]), max_poss_load, P)
                sps.append(float(s))
                d = w[j] * np.abs(load - s)
                acc = acc + d
            if acc is None:
                continue
            if setpoints is not None:
                setpoints[(e, c)] = sps
            score[g] = acc
            p = np.abs(prices[g, 0])
            if best < 0 or acc < bd or (acc == bd and p < bp):
                best, bd, bp = c, acc, p
        choice[e] = best
    return choice, score


def plan_groups_reference(vals, fc, G, keys, rows=()):
    """dragg_mpc_plan_groups restated on numpy arrays with explicit loops in the contract's order (the spec its
    CPU and GPU tests share, and what a stand-in batch serves `plan_groups` with -- not a solver fallback).
    `vals` [NVAL][N], `fc` [N][NFC][H], G groups of Nb = N / G homes -> (curve [G][nk][H] float64, count
    [G][nk][H] int32, stats [G][nr][4] float64).  Per entry: 16 partial sums from +0.0, partial w adding the
    present (non-NaN) values of homes w, w + 16, ... in ascending order, then the balanced tree
    ((p0 + p1) + (p2 + p3)) + ... over the 16; min and max over the present values."""
    _, _, ki, ri = L.plan_select(keys, rows)
    vals, fc = np.asarray(vals, dtype=np.float64), np.asarray(fc, dtype=np.float64)
    N, H = vals.shape[1], fc.shape[2]
    G = max(int(G), 1)
    if N % G:
        raise ValueError(f"{N} homes are not {G} groups")
    Nb, W = N // G, L.PLAN_WAYS
    curve, count = np.zeros((G, len(ki), H)), np.zeros((G, len(ki), H), dtype=np.int32)
    stats = np.zeros((G, len(ri), len(L.PLAN_STATS)))

    def reduce(values):
        """values: the Nb homes' doubles of one entry, NaN = absent -> (count, sum, min, max)."""
        p = [np.float64(0.0)] * W
        n, mn, mx = 0, np.float64(np.inf), np.float64(-np.inf)
        for w in range(W):
            for i in range(w, len(values), W):
                x = np.float64(values[i])
                if x == x:
                    p[w] = p[w] + x
                    n += 1
                    mn, mx = (x if x < mn else mn), (x if x > mx else mx)
        while len(p) > 1:
            p = [p[2 * m] + p[2 * m + 1] for m in range(len(p) // 2)]
        return n, p[0], mn, mx

    for g in range(G):
        cols = range(g * Nb, (g + 1) * Nb)
        shift = []
        for n in cols:
            cnt = vals[L.K["solve_counter"], n]
            shift.append(int(cnt) if 0 <= cnt < H else H)         # (NaN: H)
        for a, k in enumerate(ki):
            for j in range(H):
                if j == 0:
                    v = [vals[k, n] for n in cols]
                else:
                    v = [fc[n, k, c + j] if c + j < H else np.nan for n, c in zip(cols, shift)]
                count[g, a, j], curve[g, a, j] = reduce(v)[:2]
        for a, r in enumerate(ri):
            stats[g, a] = reduce([vals[r, n] for n in cols])
    return curve, count, stats


def plan_classes_reference(vals, fc, G, classes, P, keys, rows=()):
    """dragg_mpc_plan_classes restated (the spec its CPU and GPU tests share): `plan_groups_reference` once per
    class on NaN-masked copies -- for class c every vals row (the solve counter included) and every fc entry of
    the homes whose class is not c made absent.  `classes`: the community's map [Nb] by base home, shared by the
    G groups; P classes -> (curve [G][P][nk][H] float64, count [G][P][nk][H] int32, stats [G][P][nr][4])."""
    vals, fc = np.asarray(vals, dtype=np.float64), np.asarray(fc, dtype=np.float64)
    G = max(int(G), 1)
    cm, P = L.price_class_map(classes, vals.shape[1] // G, P)
    out = []
    for c in range(P):
        other = np.tile(cm != c, G)
        v, f = vals.copy(), fc.copy()
        v[:, other] = np.nan
        f[other] = np.nan
        out.append(plan_groups_reference(v, f, G, keys, rows))
    return tuple(np.stack([o[k] for o in out], axis=1) for k in range(3))


def resolve_price_classes(price_classes, homes, n_classes=None):
    """A community's price classes -> (map int32 [len(homes)], P, class names), or (None, 1, None) for None.
    "type": class = home type in `_lib.TYPE_CODE`'s order (base 0, pv_only 1, battery_only 2, pv_battery 3), P = 4
    even if a type is absent; else an int sequence, one per home (`_lib.price_class_map`'s checks)."""
    if price_classes is None:
        return None, 1, None
    if isinstance(price_classes, str):
        if price_classes != "type":
            raise ValueError(f"price_classes is \"type\" or an int sequence, not {price_classes!r}")
        cm, P = L.price_class_map([L.TYPE_CODE[h["type"]] for h in homes], len(homes), len(L.TYPE_CLASS_NAMES))
        return cm, P, list(L.TYPE_CLASS_NAMES)
    cm, P = L.price_class_map(price_classes, len(homes), n_classes)
    return cm, P, [str(c) for c in range(P)]


class VectorAggregator:
    def __init__(self, homes, oat, ghi, tou, episodes, seeds, start_indices, num_timesteps, int_mode="round",
                 keep_history=True, device=None, batch_cls=MPCBatch, rank=0, world=1, price_classes=None,
                 n_classes=None, ev=None, vehicles=False, day_offset=0, fleet_cls=EVFleet, **batch_kw):
        """price_classes ("type", or an int sequence [Nb] with `n_classes` = P; default None: one price for the
        community): the community's price classes (`resolve_price_classes`, `MPCBatch.set_price_classes`), shared by
        every episode and every sweep replica.  With P > 1 an action is a price per class: `step` takes [E][P] or
        [E][P][n], `sweep` [E][C][P] or [E][C][P][n] -- a 2-D `step` tensor and a 3-D `sweep` tensor then mean class
        scalars, never price lists.  `n_classes`, `class_names` and `price_class_host` describe the map.

        vehicles=True: the homes' "ev" sections become an E-group fleet (`fleet_cls`, default `EVFleet`) stepped
        after the homes at the same start indices and clocks, under the same price rows (a vehicle reads its owner
        home's class's row); `day_offset`: the step of day of environment index 0.  Every sum then counts homes
        plus vehicles; `ev_sums` ([E][3]) holds the vehicles' own rows of the last step, `ev_agg_hist` ([T][E][3],
        with keep_history) their rows filed at each episode's own clock.  ValueError if no home has a vehicle.
        `ev=` (a pre-built single fleet) is not taken: an E-group fleet with its own clocks is built here."""
        if ev is not None:
            raise NotImplementedError("the vector environments do not take a pre-built EV fleet: it follows one "
                                      "shared clock and price (DeviceAggregator(ev=...)); vehicles=True builds the "
                                      "episodes' own fleet from the homes' \"ev\" sections")
        if world > 1:
            raise ValueError("VectorAggregator runs on one rank: episodes are not sharded over ranks")
        E = int(episodes)
        if E < 1:
            raise ValueError(f"episodes must be >= 1, not {episodes!r}")
        self.E, self.Nb, self.homes = E, len(homes), homes
        self.num_timesteps = T = int(num_timesteps)
        dev = device or torch.device("cuda", torch.cuda.current_device())
        self.device = dev = torch.device(dev)
        # batch_cls is injectable only so that the host logic can be exercised on the CPU with a stand-in
        # (tests/test_vector_host.py); the solver itself is MPCBatch (HIP, no fallback)
        self.batch = batch_cls(homes, oat, ghi, tou, 0, (0.0,), int_mode=int_mode, device=dev, groups=E, **batch_kw)
        self.price_class_host, self.n_classes, self.class_names = resolve_price_classes(price_classes, homes, n_classes)
        if self.n_classes > 1:
            self.batch.set_price_classes(self.price_class_host, self.n_classes)
        self.H = int(self.batch.H)
        self.n_env = int(min(len(oat), len(ghi), len(tou)))
        self.seeds = torch.zeros(E, dtype=torch.int64, device=dev)
        self.starts = torch.zeros(E, dtype=torch.int32, device=dev)
        self.clocks = torch.zeros(E, dtype=torch.int32, device=dev)       # steps each episode has taken
        self.parked = torch.zeros(E, dtype=torch.bool, device=dev)
        self._set_keys(None, seeds, start_indices, required=True)
        N = E * self.Nb
        # per-episode rows, indexed by the episode's own clock: [T][...][E][Nb]
        self.hist = (torch.full((T, L.NVAL, N), float("nan"), dtype=torch.float64, device=dev)
                     if keep_history else None)
        self._row = torch.full((L.NVAL, N), float("nan"), dtype=torch.float64, device=dev) if keep_history else None
        self.status_hist = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.path_hist = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.agg_hist = torch.zeros((T, E, 3), dtype=torch.float64, device=dev)
        # the homes and (vehicles=True) their fleet as one unit (members.py): every move of the state goes through it
        self.members = Members(self.batch, homes=homes,
                               batch_args=(batch_cls, dict(int_mode=int_mode, device=dev, **batch_kw)),
                               fleet_args=(fleet_cls, dict(day_offset=int(day_offset), device=dev)),
                               classes=(self.price_class_host, self.n_classes) if self.n_classes > 1 else None)
        # K-step sweeps: (C, K) -> the sums [K][C * E][3], C -> the held first step, C -> the scores [C * E]
        self._path_sums, self._held, self._path_score = {}, {}, {}
        self.sweep_steps = self.path_scores = None
        # a held sweep (sweep -> commit) and the moves of the live state that void it (step, reset, commit)
        self._hold = None
        self._gen = 0
        self.adopted = torch.zeros(E, dtype=torch.bool, device=dev)      # the episodes the last commit advanced
        # the vehicles: fleet_cls is injectable for the same reason batch_cls is (tests/test_ev_vector_host.py)
        self.ev_sums = self.ev_agg_hist = None
        self.vehicle_max_rate = 0.0
        if vehicles:
            if not any(h.get("ev") is not None for h in homes):
                raise ValueError("vehicles=True: no home of the community has an \"ev\" section")
            self.members.fleet = self.members.new_fleet(tou[:self.n_env], E)
            self.ev_sums = self.fleet.sums
            self.vehicle_max_rate = float(sum(float(h["ev"]["max_rate"]) for h in homes if h.get("ev") is not None))
            if keep_history:
                self.ev_agg_hist = torch.zeros((T, E, 3), dtype=torch.float64, device=dev)

    fleet = property(lambda self: self.members.fleet)       # (None: homes only)
    # C -> the C * E-group replica batch of sweep() (a view of the unit's replicas: drop one there)
    _sweep_batches = property(lambda self: {k: r.batch for k, r in self.members.replicas.items()})

    # ------------------------------------------------------------------ masks and keys
    def _mask(self, mask):
        """None (every episode), a bool sequence / tensor [E], or episode indices -> device bool [E]."""
        return torch.as_tensor(L.episode_mask(mask, self.E), device=self.device)

    def check_start(self, start):
        """The last step of an episode from `start` must read inside the environment lists
        (dragg_mpc_step's own check: start + t + H < n_env for every t < num_timesteps)."""
        start = int(start)
        if start < 0 or start + self.num_timesteps + self.H >= self.n_env:
            raise ValueError(f"start index {start}: start + num_timesteps ({self.num_timesteps}) + H ({self.H}) "
                             f"must stay below the {self.n_env} environment entries")
        return start

    def _set_keys(self, m, seeds, start_indices, required=False):
        """New seeds / start indices ([E] host values) for the masked episodes (m None: all)."""
        for name, vals in (("seeds", seeds), ("start_indices", start_indices)):
            if vals is None:
                if required:
                    raise ValueError(f"{name}: one per episode ({self.E})")
                continue
            vals = list(vals.tolist() if hasattr(vals, "tolist") else vals)
            if len(vals) != self.E:
                raise ValueError(f"{name} has {len(vals)} entries for {self.E} episodes")
            sel = range(self.E) if m is None else [e for e, on in enumerate(m.cpu().tolist()) if on]
            if name == "seeds":
                new = torch.tensor([_seed_i64(v) for v in vals], dtype=torch.int64, device=self.device)
                self.seeds = new if m is None else torch.where(m, new, self.seeds)
            else:
                for e in sel:
                    self.check_start(vals[e])
                new = torch.tensor([int(v) for v in vals], dtype=torch.int32, device=self.device)
                self.starts = new if m is None else torch.where(m, new, self.starts)

    def _homes_mask(self, m):
        return m.repeat_interleave(self.Nb)

    # ------------------------------------------------------------------ episode control
    def reset(self, mask=None, seeds=None, start_indices=None):
        """Start the masked episodes (default: all) over: clock 0, hash columns NaN (the state of a new
        batch: the step at t = 0 takes its initial conditions from the parameters), history rows cleared,
        active.  `seeds` / `start_indices` ([E]): new keys, taken for the masked episodes only."""
        m = self._mask(mask)
        self._gen += 1
        self._set_keys(None if mask is None else m, seeds, start_indices)
        hm = self._homes_mask(m)
        b = self.batch
        self._reset_fleet(m)
        nan = torch.full((), float("nan"), dtype=torch.float64, device=self.device)
        self.clocks = torch.where(m, torch.zeros_like(self.clocks), self.clocks)
        self.parked = self.parked & ~m
        b.vals.copy_(torch.where(hm, nan, b.vals))
        b.fc.copy_(torch.where(hm, nan, b.fc))
        if self.hist is not None:
            self.hist.copy_(torch.where(hm, nan, self.hist))
        zero = torch.zeros((), dtype=torch.int32, device=self.device)
        self.status_hist.copy_(torch.where(hm, zero, self.status_hist))
        self.path_hist.copy_(torch.where(hm, zero, self.path_hist))
        self._clear_sums(self.agg_hist, m)

    def _clear_sums(self, store, m):
        """store[:, e] = 0 for the masked episodes; store [T][E][3]."""
        store.copy_(torch.where(m[None, :, None], torch.zeros((), dtype=torch.float64, device=self.device), store))

    def _reset_fleet(self, m):
        """The fleet's part of a reset: the masked groups started over, the vehicles' filed rows cleared."""
        self.members.reset_fleet(m.contiguous())
        if self.ev_agg_hist is not None:
            self._clear_sums(self.ev_agg_hist, m)

    def park(self, mask):
        """The masked episodes sit out the coming steps (idle groups: nothing of them is read or written)."""
        self.parked = self.parked | self._mask(mask)

    def resume(self, mask):
        self.parked = self.parked & ~self._mask(mask)

    def active(self):
        """Device bool [E]: the episodes the next step advances."""
        return ~self.parked & (self.clocks >= 0) & (self.clocks < self.num_timesteps)

    def done(self):
        """Device bool [E]: the episodes that have run their num_timesteps steps."""
        return self.clocks >= self.num_timesteps

    def _scatter(self, store, row, idx, on):
        """store[idx[e], ..., e, :] = row[..., e, :] for the episodes that are `on` (fixed shapes: no host
        synchronisation); store [T][...][E * Nb], row [...][E * Nb]."""
        T = store.shape[0]
        s = store.view(T, -1, self.E, self.Nb)
        r = row.reshape(1, -1, self.E, self.Nb)
        index = idx.view(1, 1, self.E, 1).expand_as(r)
        s.scatter_(0, index, torch.where(on.view(1, 1, self.E, 1), r, s.gather(0, index)))

    def _scatter_sums(self, store, row, idx, on):
        """store[idx[e], e] = row[e] for the episodes that are `on`; store [T][E][3], row [E][3]."""
        ai = idx.view(1, self.E, 1).expand(1, self.E, 3)
        store.scatter_(0, ai, torch.where(on.view(1, self.E, 1), row.view(1, self.E, 3), store.gather(0, ai)))

    def _ran(self, on):
        """The clocks the episodes `on` run at, -1 for the others (a tensor of its own)."""
        return torch.where(on, self.clocks, torch.full_like(self.clocks, -1))

    def _price_rows(self, prices, what, candidates=False):
        """An action as price rows: `prices` led by [E] (`step`) or [E][C] (`sweep`), then [P] where the community has
        price classes, then [n] -- or nothing: scalars, so that a 2-D `step` tensor and a 3-D `sweep` tensor mean
        class scalars when P > 1 -> the float64 device tensor with the [n] axis."""
        P, nc = L.device_f64(prices, self.device), self.n_classes
        dims = 2 + bool(candidates) + (nc > 1)
        if P.dim() == dims - 1:
            P = P.unsqueeze(-1)
        if P.dim() != dims or P.shape[0] != self.E or (candidates and P.shape[1] < 1) or (nc > 1 and P.shape[-2] != nc):
            lead = f"[{self.E}]" + ("[C]" if candidates else "") + (f"[{nc}]" if nc > 1 else "")
            raise ValueError(f"{what} takes prices {lead} or {lead}[n], not {list(P.shape)}")
        return P

    def step(self, prices, noise=None):
        """One step of every active episode under `prices` ([E], or [E][n] with n == 1 or n >= H: row e is
        episode e's reward-price list); the others stay idle.  -> device tensor [E][3], collect_data's
        [agg_load, forecast_load, agg_cost] per episode (an idle episode's row: its state's, i.e. its last
        step's sums, NaN before its first).  The active clocks advance on the device."""
        return self._file(self._advance(prices, noise))

    def _advance(self, prices, noise=None):
        """The solve of `step`: the prices published, every active episode stepped at its own clock (kept in
        `self._keep`, -1 for the others) -> the device bool [E] of the episodes that ran.  Nothing filed yet."""
        P = self._price_rows(prices, "step")
        self._gen += 1
        self.members.set_reward_price(P.contiguous())
        on = self.active()
        eff = self._ran(on)
        if self._row is not None:
            # (a home that hits ERR_MISSING writes no history: its row entries stay NaN, as in a single run's
            # fresh history row)
            self._row.fill_(float("nan"))
        # (the fleet after the homes, on the same stream, with the same keys and rows)
        self.members.step_episodes(self.seeds, self.starts, eff, noise=noise, hist=self._row)
        self._keep = eff
        return on

    def _sums(self, on, idx):
        """The live state's sums [E][3]: the homes', plus the vehicles' where there is a fleet (whose own rows are
        then filed for the episodes `on` at the rows `idx`)."""
        agg = self.members.sums()
        if self.ev_agg_hist is not None:
            self._scatter_sums(self.ev_agg_hist, self.fleet.sums, idx, on)
        return agg

    def _file(self, on):
        """After a step of the episodes `on` (solved, or adopted): their sums, the step's rows filed at each
        episode's own clock, the clocks advanced.  -> [E][3]"""
        b = self.batch
        idx = self.clocks.clamp(0, self.num_timesteps - 1).to(torch.int64)
        agg = self._sums(on, idx)
        if self.hist is not None:
            self._scatter(self.hist, self._row, idx, on)
        self._scatter(self.status_hist, b.status, idx, on)
        if hasattr(b, "int_path"):
            self._scatter(self.path_hist, b.int_path, idx, on)
        self._scatter_sums(self.agg_hist, agg, idx, on)
        self.clocks = self.clocks + on.to(torch.int32)
        return agg

    # ------------------------------------------------------------------ sweep, select, commit
    # C candidate prices per episode, one step ahead or K: a batch of C * E groups holds C copies of the live
    # E-group batch, copy-major (group c * E + e = episode e under its candidate c), filled by
    # dragg_mpc_replicate and stepped (K times) with the episodes' keys and clocks tiled C times.  `commit` then
    # adopts, per episode, the chosen copy's solved first step (dragg_mpc_adopt) instead of solving it again;
    # the choice can be made on the device (`select`, `select_paths`), so none of this synchronises with the host.
    def sweep(self, prices, steps=1, hold=True):
        """Every active episode's next step under each of its C candidate prices (`prices` [E][C], or
        [E][C][n] with n == 1 or n >= H), nothing committed -> device tensor [E][C][3], row (e, c)
        bit-identical to what `step` returns for episode e under prices[e][c] (an idle episode's rows: its
        state's sums).  The live batch is only read.  hold=True (default) keeps the solved replicas for
        `commit`.

        steps = K > 1: every candidate is rolled K steps ahead under its price row -> [E][C][K][3].  Step 0 is
        the step above; step j steps the same C * E replicas on with the same seeds and starts at the clocks
        + j.  A replica whose episode has no step j left (clock + j >= num_timesteps, or idle at step 0) is idle
        from then on: `self.sweep_steps` (device int32 [E]) holds the steps k_e each episode's replicas took,
        row (e, c, j), j < k_e, is bit-identical to the sums after j + 1 `step`s under prices[e][c], and the
        rows j >= k_e repeat row k_e - 1.  hold=True then keeps a copy of the replicas' FIRST step for `commit`
        (the replicas themselves move on), in buffers allocated once per C.  Extra device memory for K > 1:
        that copy -- the replica batch's hash arrays and per-home outputs over again, C * E * Nb * (NVAL + NFC *
        H + 5) doubles' worth, about C times the live batch -- and K * C * E * 3 doubles of sums per (C, K).  No
        host synchronisation for any K."""
        K = int(steps)
        if K < 1:
            raise ValueError(f"sweep takes steps >= 1, not {steps!r}")
        P, nc = self._price_rows(prices, "sweep", candidates=True), self.n_classes
        C = int(P.shape[1])
        Pc = P.transpose(0, 1).contiguous()                      # copy-major: [C][E][n] ([C][E][P][n] with classes)
        self._hold = None
        r = self.members.replica(C * self.E, key=C)
        r.set_reward_price(Pc.view(C * self.E, nc, -1) if nc > 1 else Pc.view(C * self.E, -1))
        r.replicate_from(self.members)
        on = self.active()
        eff = self._ran(on)
        rb = r.batch
        if hold and self._row is not None:
            if getattr(rb, "hist_row", None) is None:
                rb.hist_row = torch.empty((L.NVAL, rb.N), dtype=torch.float64, device=self.device)
            rb.hist_row.fill_(float("nan"))
        keys = (self.seeds.repeat(C), self.starts.repeat(C), eff.repeat(C))
        r.step_episodes(*keys, hist=rb.hist_row if hold and self._row is not None else None)
        # (a hold's "unit" is what `commit` adopts from -- the replicas, or the held copy of their first step --
        # and "src" its homes' half)
        hold = {"C": C, "P": Pc, "gen": self._gen, "on": on, "unit": r, "src": rb, "keys": keys} if hold else None
        if K > 1:
            return self._roll(r, C, K, eff, keys, hold)
        self._hold = hold
        return r.sums().view(C, self.E, 3).permute(1, 0, 2).contiguous()

    def _roll(self, r, C, K, eff, keys, hold):
        """The rest of a K-step sweep after the replicas' step 0: its sums, the held copy of it (`hold`: the hold
        that will keep it, or None), then steps 1 .. K - 1 of the replicas, each step's sums written in place into
        block j of the [K][C * E][3] buffer kept per (C, K).  The clock rows are fixed-shape ops: no host
        synchronisation."""
        E, T = self.E, self.num_timesteps
        buf = self._path_sums.get((C, K))
        if buf is None:
            buf = self._path_sums[(C, K)] = torch.zeros((K, C * E, 3), dtype=torch.float64, device=self.device)
        r.sums(out=buf[0])
        if hold is not None:
            held = self._held.get(C)
            if held is None:
                held = self._held[C] = Held(r)
            hold["unit"] = hold["src"] = held.fill(r, getattr(r.batch, "hist_row", None))
        idle = torch.full_like(eff, -1)
        for j in range(1, K):
            clk = torch.where((eff >= 0) & (eff + j < T), eff + j, idle).repeat(C)
            r.step_episodes(keys[0], keys[1], clk)
            r.sums(out=buf[j])
        self.sweep_steps = torch.where(eff >= 0, (T - eff).clamp(max=K), torch.zeros_like(eff))
        self._hold = hold
        out = buf.view(K, C, E, 3).permute(2, 1, 0, 3).contiguous()
        self._paths = (out, buf)
        return out

    def select_paths(self, paths, tracked, setpoints, prices, weights, max_poss_load):
        """`select` over K-step rollouts (dragg_mpc_select_paths): per episode the candidate whose loads
        (`paths` [E][C][K][3], `sweep(steps=K)`'s) lie closest, weighted by `weights` [K], to the setpoints the
        environment's rule would file if the candidate were played -- from the tracked loads `tracked` [E][P],
        the setpoints now `setpoints` [E] and the community's `max_poss_load`; only the steps an episode has
        left count.  Ties to the smaller |price| (`prices` [E][C] or [E][C][n]: its first entry), then the
        smaller index; -1 where no candidate has its loads or the episode is idle.  -> device int32 [E]; the
        scores are kept in `self.path_scores` ([E][C], NaN: no score).  Device tensors are read where they are:
        no synchronisation."""
        dev, E = self.device, self.E
        S = L.device_f64(paths, dev)
        if S.dim() != 4 or S.shape[0] != E or S.shape[3] != 3:
            raise ValueError(f"select_paths takes paths [{E}][C][K][3], not {list(S.shape)}")
        C, K = int(S.shape[1]), int(S.shape[2])
        last = getattr(self, "_paths", None)
        sums = last[1] if last is not None and last[0] is paths else S.permute(2, 1, 0, 3).reshape(K, C * E, 3).contiguous()
        P = self._tie_rows(prices, C).contiguous()
        w = L.device_f64(weights, dev).reshape(-1).contiguous()
        if w.numel() != K:
            raise ValueError(f"select_paths takes {K} weights, not {w.numel()}")
        score = self._path_score.get(C)
        if score is None:
            score = self._path_score[C] = torch.full((C * E,), float("nan"), dtype=torch.float64, device=dev)
        on = self.active()
        ran = self._ran(on)
        choice = self.batch.select_paths(sums, ran, L.device_f64(tracked, dev).reshape(E, -1).contiguous(),
                                         L.device_f64(setpoints, dev).reshape(-1).contiguous(), w, P,
                                         self.num_timesteps, 0.5 * float(max_poss_load), score=score)
        self.path_scores = score.view(C, E).t()
        return choice

    def select(self, sums, setpoints, prices):
        """Per episode the candidate whose load (`sums` [E][C][3], `sweep`'s) lies closest to its setpoint
        (`setpoints` [E]); ties to the smaller |price| (`prices` [E][C] or [E][C][n]: its first entry), then the
        smaller index; -1 where no candidate has a load -> device int32 [E] (dragg_mpc_select_groups)."""
        S = L.device_f64(sums, self.device)
        P = L.device_f64(prices, self.device)
        if S.dim() != 3 or S.shape[0] != self.E or S.shape[2] != 3:
            raise ValueError(f"select takes sums [{self.E}][C][3], not {list(S.shape)}")
        C = int(S.shape[1])
        return self.batch.select_groups(S.permute(1, 0, 2).reshape(C * self.E, 3), setpoints, self._tie_rows(P, C))

    def tie_key(self, prices, C):
        """The tie rule's key of every candidate, copy-major [C * E][1]: the sum over the classes, ascending, of
        |first entry of the class's price row|, added left to right by elementwise ops (no host synchronisation).
        One class: |first entry| -- what the select kernels themselves take of a price row."""
        Q = L.device_f64(prices, self.device).reshape(self.E, C, self.n_classes, -1)[..., 0]
        key = Q[..., 0].abs()
        for c in range(1, self.n_classes):
            key = key + Q[..., c].abs()
        return key.t().reshape(C * self.E, 1)

    def _tie_rows(self, prices, C):
        """The price rows the select kernels read for their tie rule, copy-major [C * E][n]: without classes the
        candidates' own rows, with classes `tie_key` (the kernels take |row[0]|, and the key is not negative)."""
        if self.n_classes > 1:
            return self.tie_key(prices, C)
        return L.device_f64(prices, self.device).reshape(self.E, C, -1).permute(1, 0, 2).reshape(C * self.E, -1)

    def commit(self, choice):
        """Play, per episode, candidate choice[e] of the held sweep (`choice`: a device int tensor [E]): its
        solved step becomes the episode's step, as `step` under the chosen price rows would have left it, bit
        for bit.  An entry outside [0, C) -- and every episode that was idle in the sweep or is idle now --
        adopts nothing and stays where it is.  The chosen rows become the live batch's reward price (an
        episode that adopted nothing: its candidate 0's row, which nothing reads).  -> [E][3], the episodes'
        sums as `step` returns them; `self.adopted` (device bool [E]) holds the episodes that advanced."""
        return self._file(self._adopt(choice))

    def _adopt(self, choice):
        """The adoption of `commit` -> the device bool [E] of the episodes that adopted a step (also
        `self.adopted`).  Nothing filed yet."""
        h = self._hold
        if h is None or h["gen"] != self._gen:
            raise ValueError("commit: no sweep of the live state is held (sweep first; a step or a reset voids it)")
        C = h["C"]
        if not torch.is_tensor(choice) or tuple(choice.shape) != (self.E,) or choice.dtype.is_floating_point:
            raise ValueError(f"commit takes a device int tensor [{self.E}]")
        self._hold = None
        ch = choice.to(device=self.device, dtype=torch.int32)
        on = h["on"] & self.active() & (ch >= 0) & (ch < C)
        ch = torch.where(on, ch, torch.full_like(ch, -1)).contiguous()
        self._gen += 1
        rows = h["P"][ch.clamp(0, C - 1).to(torch.int64), torch.arange(self.E, device=self.device)]
        self.members.set_reward_price(rows.contiguous())
        if self._row is not None:
            self._row.fill_(float("nan"))
        self.members.adopt_from(h["unit"], ch, hist=self._row)
        self.adopted = on
        return on

    # ------------------------------------------------------------------ the device-resident environment's paths
    # `step`, `commit` and `reset` again, ending in one kernel each (MPCBatch.env_file / env_reset) instead of
    # `_file`'s gathers and scatters and `reset`'s whole-store rewrites; the kernel also keeps the environment
    # state of an `rl.DeviceVectorEnv` (`EnvState`).  The clocks are written in place.
    def env_state(self, prev_timesteps, max_poss_load, start_load):
        return EnvState(self, prev_timesteps, max_poss_load, start_load)

    def _env_file(self, st, on, ran=None):
        """File the step of the episodes `on`; `ran`: the clocks they ran at, -1 for the others (a tensor of
        its own: the kernel reads it in every block and writes the clocks)."""
        if ran is None:
            ran = self._ran(on)
        agg = self._sums(on, ran.clamp(0, self.num_timesteps - 1).to(torch.int64))
        self.batch.env_file(st, ran, agg, hist=self._row)
        return agg

    def step_env(self, st, prices, noise=None):
        """`step`, filed by dragg_mpc_env_file: the same solve, sums, rows and clocks, plus the environment
        state `st` (`env_state`) and its observations.  -> [E][3]"""
        on = self._advance(prices, noise)
        return self._env_file(st, on, self._keep)

    def commit_env(self, st, choice):
        """`commit`, filed by dragg_mpc_env_file (the episodes that ran: those that adopted a step)."""
        return self._env_file(st, self._adopt(choice))

    def reset_env(self, st, mask=None, seeds=None, start_indices=None):
        """`reset` as one kernel over the masked episodes' columns alone (dragg_mpc_env_reset), the
        environment state `st` started over with them.  `mask` may be a device bool tensor [E] (e.g.
        `done()`), `seeds` / `start_indices` device tensors [E]: they are taken for the masked episodes with no
        host check and no host round trip -- an episode whose start index leaves the environment lists sits
        idle (dragg_mpc_step_episodes).  Host lists are checked as in `reset`."""
        m = self._mask(mask)
        self._gen += 1
        host = {}
        for name, vals, dtype in (("seeds", seeds, torch.int64), ("start_indices", start_indices, torch.int32)):
            if torch.is_tensor(vals) and vals.device == self.device:
                if tuple(vals.shape) != (self.E,) or vals.dtype.is_floating_point:
                    raise ValueError(f"{name}: a device int tensor [{self.E}]")
                attr = "seeds" if name == "seeds" else "starts"
                setattr(self, attr, torch.where(m, vals.to(dtype), getattr(self, attr)))
            else:
                host[name] = vals
        self._set_keys(None if mask is None else m, host.get("seeds"), host.get("start_indices"))
        self.parked = self.parked & ~m
        self.batch.env_reset(st, m.contiguous())
        self._reset_fleet(m)

    # ------------------------------------------------------------------ plan observations
    def plan(self, keys, rows=(), out=None, classes=False):
        """Every episode's planned curves, from the state its last step left (`MPCBatch.plan_groups`): device
        tensors (curve [E][nk][H], count [E][nk][H], stats [E][nr][4]).  A pure function of the hash arrays: a
        parked or finished episode's rows are those of its last step, a fresh one's empty (count 0).  No
        synchronisation.  classes=True: per (episode, price class) -- curve and count [E][P][nk][H], stats
        [E][P][nr][4] (`MPCBatch.plan_groups(classes=True)`, dragg_mpc_plan_classes)."""
        if classes:
            return self.batch.plan_groups(keys, rows, out=out, classes=True)
        return self.batch.plan_groups(keys, rows, out=out)

    # ------------------------------------------------------------------ rows for the host
    def clocks_host(self):
        return [int(c) for c in self.clocks.cpu().tolist()]

    def _rows(self, store, e, t=None):
        t = self.clocks_host()[e] if t is None else t
        return store.view(store.shape[0], -1, self.E, self.Nb)[:min(t, self.num_timesteps), :, e, :]

    def episode_history(self, e):
        """Episode e's hash history so far: [t_e][NVAL][Nb]."""
        if self.hist is None:
            raise RuntimeError("keep_history=False: no history rows")
        return self._rows(self.hist, e)

    def episode_status(self, e):
        """[t_e][Nb] dragg_status of every step of episode e."""
        return self._rows(self.status_hist, e)[:, 0]

    def episode_paths(self, e):
        """[t_e][Nb] int_path bits of every step of episode e."""
        return self._rows(self.path_hist, e)[:, 0]

    def episode_sums(self, e):
        """[t_e][3] collect_data sums of every step of episode e."""
        return self.agg_hist[:min(self.clocks_host()[e], self.num_timesteps), e]

    def approx_counts(self):
        """Per episode, the solves so far by int_path (the masks of DeviceAggregator.approx_counts):
        {"approx_solves": [E], "step_dp_solves": [E], "later_launch_solves": [E]}."""
        p = self.path_hist.view(self.num_timesteps, self.E, self.Nb)        # (cleared rows are 0)
        return dict(zip(L.PATH_COUNT_KEYS, L.path_counts(p, (0, 2)).cpu().tolist()))

    def status_counts(self):
        """Solves so far by dragg_status over every episode: {status name: count}."""
        clk = self.clocks_host()
        st = self.status_hist.view(self.num_timesteps, self.E, self.Nb).cpu().numpy()
        n = np.zeros(len(L.STATUS_NAMES), dtype=np.int64)
        for e, t in enumerate(clk):
            n += np.bincount(st[:min(t, self.num_timesteps), e].reshape(-1), minlength=len(n))[:len(n)]
        return {k: int(v) for k, v in zip(L.STATUS_NAMES, n)}

    def check_errors(self):
        """Raise as the reference would if a home hit a crashing path (KeyError / ValueError): the first
        such over the episodes, by (timestep, episode, home), with all three named."""
        clk = self.clocks_host()
        st = self.status_hist.view(self.num_timesteps, self.E, self.Nb).cpu().numpy()
        first = None
        for code in (L.ST_ERR_MISSING, L.ST_ERR_PARSE):
            for t, e, i in np.argwhere(st == code):
                if t < clk[e] and (first is None or (t, e, i) < first[:3]):
                    first = (int(t), int(e), int(i), code)
                    break
        if first is None:
            return
        t, e, i, code = first
        exc = KeyError if code == L.ST_ERR_MISSING else ValueError
        raise exc(f"episode {e}, home {self.homes[i]['name']} at timestep {t}: {L.STATUS_NAMES[code]} "
                  "(the reference raises here, mpc_calc.py:280-289 / 537-539)")
