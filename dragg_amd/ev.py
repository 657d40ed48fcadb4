"""Electric vehicles: a fleet of stage-varying storage LPs solved beside the homes (dragg_mpc_ev_*).

The reference has no vehicle; the model is this project's.  A home dict may carry an
`"ev"` section, on any home type:

    capacity (kWh), capacity_lower, capacity_upper (fractions), max_rate (kW), ch_eff, disch_eff,
    e_ev_init (fraction), v2g (bool), depart_step, return_step (steps of day, 0 <= depart < return <= 24 dt),
    trip_kwh (per day), depart_soc (fraction)

The vehicle is one more separable block of its home: the price is an input and nothing else couples it to the
home's LP, so the fleet is a batch of its own (one wave per vehicle) whose three sums are added to the homes'.
`pack_evs` and `ev_schedule` are plain numpy (the schedule arithmetic the kernel's prologue does); `EVFleet` holds
the device state and has no CPU fallback.  The aggregators move a fleet together with its homes' batch through
`members.Members` (prices, episode steps, sums, replicas, adoption, reset); the arrays that make a fleet's state are
named once, `members.FLEET_ARRAYS`.
"""
import ctypes

import numpy as np

from . import _lib as L
from .members import FLEET_ARRAYS
from .mpc import hems_dims

EV_FIELDS = ("capacity", "capacity_lower", "capacity_upper", "max_rate", "ch_eff", "disch_eff", "e_ev_init", "v2g",
             "depart_step", "return_step", "trip_kwh", "depart_soc")


def pack_evs(homes):
    """home dicts -> (params [NEVP][M] float64, owners [M]: the index in `homes` of each vehicle's home), in the
    homes' order.  ValueError for a missing field or a schedule outside 0 <= depart < return <= 24 dt."""
    owners = [i for i, h in enumerate(homes) if h.get("ev") is not None]
    P = np.zeros((L.NEVP, len(owners)))
    for j, i in enumerate(owners):
        e = homes[i]["ev"]
        missing = [k for k in EV_FIELDS if k not in e]
        if missing:
            raise ValueError(f"home {homes[i].get('name', i)}: ev section lacks {missing}")
        dt = hems_dims(homes[i])[1]
        dep, ret = int(e["depart_step"]), int(e["return_step"])
        if dep != e["depart_step"] or ret != e["return_step"] or not 0 <= dep < ret <= 24 * dt:
            raise ValueError(f"home {homes[i].get('name', i)}: ev schedule needs integer steps with "
                             f"0 <= depart_step < return_step <= {24 * dt}, not {e['depart_step']}, {e['return_step']}")
        cap = float(e["capacity"])
        P[L.EVP["CAP"], j] = cap
        P[L.EVP["EMIN"], j] = float(e["capacity_lower"]) * cap
        P[L.EVP["EMAX"], j] = float(e["capacity_upper"]) * cap
        P[L.EVP["RATE"], j] = float(e["max_rate"])
        P[L.EVP["ETAC"], j] = float(e["ch_eff"])
        P[L.EVP["ETAD"], j] = float(e["disch_eff"])
        P[L.EVP["EINIT"], j] = float(e["e_ev_init"]) * cap
        P[L.EVP["V2G"], j] = 1.0 if e["v2g"] else 0.0
        P[L.EVP["DEPART"], j] = dep
        P[L.EVP["RETURN"], j] = ret
        P[L.EVP["TRIP"], j] = float(e["trip_kwh"])
        P[L.EVP["EREQ"], j] = float(e["depart_soc"]) * cap
    return P, np.asarray(owners, dtype=np.int64)


def ev_schedule(P, dt, day_offset, t, H):
    """The stage arrays of the step at timestep t, as the kernel's prologue builds them: a dict of [H][M] arrays
    rate_ch, rate_dis, drain, lo, hi (row k of lo / hi: the box of E_{k+1}) and `away` (bool)."""
    P = np.asarray(P, dtype=float)
    D = 24 * int(dt)
    s = (int(day_offset) + int(t) + np.arange(H + 1)) % D                  # step of day of stage k
    dep, ret = P[L.EVP["DEPART"]].astype(int), P[L.EVP["RETURN"]].astype(int)
    away = (dep[None, :] <= s[:H, None]) & (s[:H, None] < ret[None, :])
    rate_ch = np.where(away, 0.0, P[L.EVP["RATE"]][None, :])
    rate_dis = np.where(P[L.EVP["V2G"]][None, :] != 0.0, rate_ch, 0.0)
    drain = np.where(away, (P[L.EVP["TRIP"]] / (ret - dep).astype(float))[None, :], 0.0)
    lo = np.where(s[1:, None] == dep[None, :], np.maximum(P[L.EVP["EMIN"]], P[L.EVP["EREQ"]])[None, :],
                  P[L.EVP["EMIN"]][None, :])
    hi = np.broadcast_to(P[L.EVP["EMAX"]][None, :], lo.shape).copy()
    return {"rate_ch": rate_ch, "rate_dis": rate_dis, "drain": drain, "lo": lo, "hi": hi, "away": away}


def ev_episode_day_step(day_offset, start0, start, t, dt):
    """The step of day of stage 0 of an episode step (dragg_mpc_ev_step_episodes' day clock): `day_offset` is the
    step of day of environment index `start0`, the episode starts at index `start` and stands at timestep `t`
    -> (day_offset + (start - start0) + t) mod 24 dt, the non-negative remainder.  Scalars or integer arrays."""
    D = 24 * int(dt)
    d = (np.asarray(day_offset, dtype=np.int64) + (np.asarray(start, dtype=np.int64) - np.asarray(start0, dtype=np.int64))
         + np.asarray(t, dtype=np.int64))
    r = np.mod(d, D)
    return int(r) if r.ndim == 0 else r


def ev_fallback(P, dt, rate_ch, drain, E0):
    """The uncontrolled rule of a vehicle without a trajectory, in the kernel's operation order (one column per
    vehicle): -> (ch [H][M], E [H][M]); dis is zero."""
    a = P[L.EVP["ETAC"]] / int(dt)
    E = np.array(E0, dtype=float)
    ch_rows, e_rows = [], []
    for k in range(len(rate_ch)):
        room = (P[L.EVP["EMAX"]] - E) / a
        ch = np.minimum(rate_ch[k], np.maximum(0.0, room))
        E = np.minimum(np.maximum((E + a * ch) - drain[k], 0.0), P[L.EVP["CAP"]])
        ch_rows.append(ch)
        e_rows.append(E)
    return np.array(ch_rows), np.array(e_rows)


def shard_evs(homes, rank=0, world=1):
    """The vehicles of the homes a rank solves (homes rank, rank + world, ...: aggregator.shard_index, so a vehicle
    lives on its home's rank) -> (params [NEVP][M], owners [M]: the vehicles' GLOBAL home indices, the list of the
    shard's homes)."""
    idx = np.arange(rank, len(homes), world)
    mine = [homes[i] for i in idx]
    P, owners = pack_evs(mine)
    return P, idx[owners] if len(owners) else owners, mine


def has_evs(homes):
    return any(h.get("ev") is not None for h in homes)


class EVFleet:
    """The vehicles of `homes` (those with an "ev" section) as one device-resident batch.

    tou, start_index : the environment's TOU list and start index (the homes' own).
    reward_price : as MPCBatch's (length 1 or >= H; a grouped fleet: [G][n] or one list for every group).
    day_offset : the step of day of timestep 0, i.e. of environment index `start_index`.
    groups : G > 1: G consecutive replicas of the vehicles, replica g under price row g (`replicate_from`).  The
        groups may be episodes, each with its own start index and clock (`step_episodes`), and the vehicles may
        have price classes (`set_price_classes`): the vector environments' fleet.
    rank, world : keep the vehicles of homes rank, rank + world, ... only (the homes' `shard_index`).
    template_home : a home of the community, for the dims of a fleet without vehicles (its steps are no-ops).
    """

    def __init__(self, homes, tou=None, start_index=0, reward_price=(0.0,), day_offset=0, device="cuda", groups=1,
                 rank=0, world=1, template_home=None):
        import torch
        if int(groups) < 1:
            raise ValueError(f"groups must be >= 1, not {groups!r}")
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.DraggError("no GPU visible: the EV fleet has no CPU fallback")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        all_homes = homes
        P, owners, homes = shard_evs(all_homes, rank, world)
        owner_homes = [all_homes[i] for i in owners]
        if not owner_homes and template_home is None and not homes:
            raise ValueError("no homes")
        S, dt, H, disc = hems_dims(owner_homes[0] if owner_homes else (homes[0] if homes else template_home))
        for h in owner_homes:
            if hems_dims(h) != (S, dt, H, disc):
                raise ValueError("all homes of a fleet must share the hems settings")
        self.owners = owners
        self.names = [h.get("name", str(i)) for i, h in zip(owners, owner_homes)]
        self.groups, self.Mb = int(groups), len(owners)
        self.params_host = P
        if self.groups > 1:
            P = np.tile(P, (1, self.groups))
        self.M, self.H, self.S, self.dt = self.groups * self.Mb, H, S, dt
        self.day_offset = int(day_offset) % (24 * dt)
        dev = self.device
        self.params = torch.tensor(P, dtype=torch.float64, device=dev).contiguous()
        self.dims = L.Dims(n_homes=self.M, horizon=H, sub_steps=S, dt=dt, n_draw_hours=1, n_env=0, n_rp=1,
                           int_mode=L.INT_ROUND, max_iter=0, check_every=0, discount=disc, flags=0,
                           n_groups=self.groups if self.groups > 1 else 0)
        rc = self.lib.dragg_mpc_ev_lds_bytes(ctypes.byref(self.dims))
        if rc < 0:
            L.check(rc)
        self.lds_bytes = rc
        self.n_classes, self.price_class, self.price_class_host = 1, None, None
        self.set_environment(tou if tou is not None else [0.0], start_index)
        self.set_reward_price(reward_price)
        self.vals = torch.full((L.NEVV, self.M), float("nan"), dtype=torch.float64, device=dev)
        self.fc_store = torch.full((self.M, L.NEVK, H), float("nan"), dtype=torch.float64, device=dev)
        self.fc = self.fc_store.permute(1, 2, 0)           # [NEVK][H][M], as MPCBatch.fc
        self.status = torch.zeros(self.M, dtype=torch.int32, device=dev)
        self.obj = torch.full((self.M,), float("nan"), dtype=torch.float64, device=dev)
        self.sums = torch.zeros((self.groups, 3), dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ inputs
    def set_environment(self, tou, start_index):
        import torch
        self.tou = (tou.detach().to(device=self.device, dtype=torch.float64).contiguous() if torch.is_tensor(tou)
                    else torch.tensor(np.asarray(tou, dtype=float), dtype=torch.float64, device=self.device))
        self.start_index = int(start_index)
        self.dims.n_env = int(self.tou.numel())

    def set_price_classes(self, vehicle_classes, n_classes=None):
        """The vehicles' price classes: `vehicle_classes`, a host int sequence [Mb] by base vehicle (each vehicle's
        owner home's class), P = `n_classes` (None: the largest class + 1), shared by every group.  The fleet then
        holds P price rows per group and `step_episodes` solves vehicle v of group g under row (g, class of v).
        The rows start over at price 0.  `_lib.price_class_map`'s checks; P == 1 (or None): no classes."""
        import torch
        if vehicle_classes is None:
            cm, P = None, 1
        else:
            cm, P = L.price_class_map(vehicle_classes, self.Mb, n_classes)
        self.n_classes = P
        self.price_class_host = cm if P > 1 else None
        self.price_class = torch.tensor(cm, dtype=torch.int32, device=self.device).contiguous() if P > 1 else None
        self.set_reward_price(torch.zeros((self.groups, P) if P > 1 else (self.groups, 1), dtype=torch.float64))

    def set_reward_price(self, rp):
        """As MPCBatch.set_reward_price (`_lib.price_rows`): one list, or [G][n] for a grouped fleet; with P price
        classes (`set_price_classes`) [G][P][n], [G][P] (class scalars), or one [P] / [P][n] for every group."""
        rp, self.dims.n_rp = L.price_rows(rp, self.groups, self.n_classes, self.H, self.device, "a fleet")
        self.rp = rp.clone()                    # (a copy of its own: the caller's rows may be rewritten)

    # ------------------------------------------------------------------ structs and launches
    def _ev(self):
        return L.Ev(params=L.ptr(self.params), vals=L.ptr(self.vals), fc=L.ptr(self.fc_store),
                    status=L.ptr(self.status), obj=L.ptr(self.obj), day_offset=self.day_offset, n_vehicles=self.M)

    def _problem(self):
        return L.Problem(tou=L.ptr(self.tou), reward_price=L.ptr(self.rp), start_index=self.start_index)

    def step(self, t, stream=None):
        """One closed-loop step of every vehicle (dragg_mpc_ev_step) on `stream` (default: the current one)."""
        L.check(self.lib.dragg_mpc_ev_step(self.dims, self._problem(), self._ev(), int(t),
                                           L.stream_ptr(stream, self.device)))

    def step_episodes(self, starts, clocks, stream=None, t=0):
        """One step of a fleet whose groups are episodes (dragg_mpc_ev_step_episodes): group g at its own start
        index `starts[g]` and timestep `clocks[g]` (contiguous device int32 [G]; a negative clock, or a window that
        leaves the environment lists: the group is idle and no byte of it is written), under its own price row --
        its vehicles' classes' rows with price classes.  None for either: the fleet's own start_index / `t` for
        every group.  The day clock follows the start index (`ev_episode_day_step`).  No synchronisation."""
        import torch
        for name, x in (("starts", starts), ("clocks", clocks)):
            if x is not None:
                L.device_arg(x, name, self.device, torch.int32, (self.groups,))
        ep = L.Episodes(seed=None, start_index=L.ptr(starts), timestep=L.ptr(clocks))
        cls = L.Classes(n_classes=int(self.n_classes), price_class=L.ptr(self.price_class))
        L.check(self.lib.dragg_mpc_ev_step_episodes(self.dims, self._problem(), ep, cls, self._ev(), int(t),
                                                    L.stream_ptr(stream, self.device)))
        self._keep = (starts, clocks)           # (the launch is asynchronous: keep its keys alive)

    def solve_explicit(self, price, rate_ch, rate_dis, drain, lo, hi, E0, stream=None):
        """The general storage LP on explicit per-stage inputs [H][M] and E0 [M] (dragg_mpc_ev_solve_explicit):
        writes vals, fc, status, obj."""
        rows = [L.device_f64(x, self.device).contiguous() for x in (price, rate_ch, rate_dis, drain, lo, hi)]
        for x in rows:
            if tuple(x.shape) != (self.H, self.M):
                raise ValueError(f"explicit inputs are [{self.H}][{self.M}], not {list(x.shape)}")
        e0 = L.device_f64(E0, self.device).contiguous()
        if tuple(e0.shape) != (self.M,):
            raise ValueError(f"E0 is [{self.M}], not {list(e0.shape)}")
        ex = L.EvExplicit(*[L.ptr(x) for x in rows], L.ptr(e0))
        L.check(self.lib.dragg_mpc_ev_solve_explicit(self.dims, self._ev(), ex, L.stream_ptr(stream, self.device)))
        self._keep = (rows, e0)                # (the launch is asynchronous: keep its inputs alive)

    def aggregate_groups(self, out=None, stream=None):
        """[G][agg_load, forecast_load, agg_cost] of the vehicles (dragg_mpc_ev_aggregate)."""
        out = self.sums if out is None else out
        L.check(self.lib.dragg_mpc_ev_aggregate(self.dims, self._ev(), L.ptr(out), L.stream_ptr(stream, self.device)))
        return out

    def aggregate(self, out=None, stream=None):
        """The fleet's three sums: [3] for one group, [G][3] for a grouped fleet."""
        s = self.aggregate_groups(out.reshape(self.groups, 3) if out is not None else None, stream)
        return s.reshape(3) if self.groups == 1 else s

    def aggregate_onto(self, base, out=None, stream=None):
        """`base` ([G][3], the homes' sums) plus the vehicles' (dragg_mpc_ev_aggregate_onto): `aggregate_groups`'
        rows in the same summation order, then one fp64 add per entry -> `out` (default: `base` itself, in place).
        The vehicles' own rows go to `self.sums`."""
        import torch
        out = base if out is None else out
        for name, x in (("base", base), ("out", out)):
            L.device_arg(x, f"aggregate_onto: {name}", self.device, torch.float64, numel=self.groups * 3)
        L.check(self.lib.dragg_mpc_ev_aggregate_onto(self.dims, self._ev(), L.ptr(base), L.ptr(out), L.ptr(self.sums),
                                                     L.stream_ptr(stream, self.device)))
        return out

    # ------------------------------------------------------------------ state
    def adopt_from(self, src, choice, stream=None):
        """`MPCBatch.adopt_from` for a fleet (dragg_mpc_ev_adopt): `src` holds C copies of this fleet's E groups,
        copy-major; group e takes the vals columns, fc blocks, status and obj of copy `choice[e]` (contiguous
        device int32 [E]), bit for bit; an entry outside [0, C) leaves its group untouched.  `src`: an EVFleet,
        or anything with its arrays (vals, fc_store, status, obj, M, H)."""
        import torch
        copies = src.M // self.M if self.M else 1
        if copies < 1 or src.M != copies * self.M or src.H != self.H:
            raise ValueError(f"adopt_from: a fleet of {self.M} vehicles (H = {self.H}) cannot adopt from {src.M} "
                             f"vehicles (H = {src.H}): the source holds whole copies of it")
        L.device_arg(choice, "choice", self.device, torch.int32, (self.groups,))
        s = L.Ev(params=None, vals=L.ptr(src.vals), fc=L.ptr(src.fc_store), status=L.ptr(src.status),
                 obj=L.ptr(src.obj), day_offset=self.day_offset, n_vehicles=src.M)
        L.check(self.lib.dragg_mpc_ev_adopt(self.dims, copies, L.ptr(choice), s, self._ev(),
                                            L.stream_ptr(stream, self.device)))
        self._keep = (src, choice)

    def reset_groups(self, mask, stream=None):
        """Start the masked groups (`mask`: contiguous device bool [G]) over (dragg_mpc_ev_reset): their vals
        columns, fc blocks and obj NaN, their status 0 -- the state of a new fleet; the others keep every byte."""
        import torch
        L.device_arg(mask, "mask", self.device, torch.bool, (self.groups,))
        L.check(self.lib.dragg_mpc_ev_reset(self.dims, self._ev(), L.ptr(mask), L.stream_ptr(stream, self.device)))
        self._keep = (mask,)

    def snapshot(self):
        return tuple(getattr(self, k).clone() for k in FLEET_ARRAYS)

    def restore(self, snap):
        for k, src in zip(FLEET_ARRAYS, snap):
            getattr(self, k).copy_(src)

    def replicate_from(self, base):
        """A grouped fleet's state: every group a copy of `base`'s (a fleet of the same vehicles, one group).
        `base` may itself be a grouped fleet of E groups: this fleet (C * E groups) then holds C copies of it,
        copy-major -- copy c of base group e is group c * E + e (as `MPCBatch.replicate_from`)."""
        E = max(getattr(base, "groups", 1), 1)
        C = self.groups // E
        if C < 1 or C * E != self.groups or base.M != E * self.Mb or base.H != self.H:
            raise ValueError(f"replicate_from: a base fleet of {self.Mb} vehicles at H = {self.H} (in groups that "
                             f"divide {self.groups}), not {base.M} at H = {base.H} in {E} groups")
        self.vals.view(L.NEVV, C, base.M).copy_(base.vals.unsqueeze(1).expand(-1, C, -1))
        self.fc_store.view(C, base.M, L.NEVK, self.H).copy_(base.fc_store.unsqueeze(0).expand(C, -1, -1, -1))
        self.status.view(C, base.M).copy_(base.status.unsqueeze(0).expand(C, -1))
        self.obj.view(C, base.M).copy_(base.obj.unsqueeze(0).expand(C, -1))

    def schedule(self, t, start=None):
        """`ev_schedule` of this fleet's vehicles (tiled over the groups) at timestep t; `start`: of an episode
        that starts at that environment index (the day clock of `ev_episode_day_step`; default: the fleet's own)."""
        P = np.tile(self.params_host, (1, self.groups)) if self.groups > 1 else self.params_host
        day = (self.day_offset if start is None
               else ev_episode_day_step(self.day_offset, self.start_index, int(start), 0, self.dt))
        return ev_schedule(P, self.dt, day, t, self.H)


def build_fleet(homes, **kw):
    """An EVFleet of `homes`' vehicles, or None when no home of the community has an "ev" section (decided on the
    whole community, so every rank decides alike; a shard without vehicles gets an empty fleet)."""
    if not has_evs(homes):
        return None
    kw.setdefault("template_home", homes[0])
    return EVFleet(homes, **kw)
