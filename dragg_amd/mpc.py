"""Host side of the batched MPC: home packing, device-resident hash arrays, launches.

This is the MI355X-native replacement of `dragg/mpc_calc.py`'s per-home solve: all homes
of a timestep are solved by ONE kernel launch of libdragg_mi355x.so (one 64-lane
workgroup per home).  Per-home parameters, the redis "hash" of each home and the
environment lists live on the GPU as fp64 struct-of-arrays tensors (home index
innermost).  See `dragg_amd.calc.MPCCalc` for the per-home facade with the
reference's interface.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

TAP_TEMP = 15.0  # mpc_calc.py:181
SEED_DTYPES = (torch.int64, getattr(torch, "uint64", torch.int64))      # a seed's bits are the key, either way


def _f(x):
    return float(x)


def hems_dims(home):
    """(S, dt, H, discount) exactly as `setup_base_problem` derives them (mpc_calc.py:148-152)."""
    hems = home["hems"]
    S = max(1, int(hems["sub_subhourly_steps"]))
    dt = max(1, int(hems["hourly_agg_steps"]))
    H = max(1, int(hems["horizon"] * dt))
    return S, dt, H, float(hems["discount_factor"])


def pack_homes(homes, template=None):
    """home dicts (aggregator.py:423-449 schema) -> (params [NPARAM][N], types [N], draws [hours][N], dims).

    Derived constants are computed with the reference's own float expressions
    (mpc_calc.py:157-189, 239-244, 257-258, 274).  `template`: a home of the community whose
    hems settings give the dims of an empty shard (N = 0, more ranks than homes)."""
    N = len(homes)
    if N == 0 and template is None:
        raise ValueError("no homes")
    S, dt, H, disc = hems_dims(homes[0] if N else template)
    for h in homes:
        if hems_dims(h) != (S, dt, H, disc):
            raise ValueError("all homes of a batch must share the hems settings (responsive_hems)")
    P = np.zeros((L.NPARAM, N))
    types = np.zeros(N, dtype=np.int32)
    nd = max((len(h["wh"]["draw_sizes"]) for h in homes), default=1)
    draws = np.zeros((nd, N))
    for i, h in enumerate(homes):
        if h["type"] not in L.TYPE_CODE:
            raise ValueError(f"unknown home type {h['type']!r}")
        types[i] = L.TYPE_CODE[h["type"]]
        hv, wh = h["hvac"], h["wh"]
        P[L.P["R"], i] = _f(hv["r"])
        P[L.P["C"], i] = _f(hv["c"]) * 1000
        P[L.P["PC"], i] = _f(hv["p_c"]) / S
        P[L.P["PH"], i] = (_f(hv["p_h"])) / S
        P[L.P["RW"], i] = _f(wh["r"]) * 1000
        P[L.P["PW"], i] = _f(wh["p"]) / S
        P[L.P["CW"], i] = _f(wh["tank_size"]) * 4.2
        P[L.P["V"], i] = _f(wh["tank_size"])
        P[L.P["TMIN"], i] = _f(hv["temp_in_min"])
        P[L.P["TMAX"], i] = _f(hv["temp_in_max"])
        P[L.P["TWMIN"], i] = _f(wh["temp_wh_min"])
        P[L.P["TWMAX"], i] = _f(wh["temp_wh_max"])
        P[L.P["TINIT"], i] = _f(hv["temp_in_init"])
        P[L.P["TWINIT"], i] = _f(wh["temp_wh_init"])
        if "battery" in h["type"]:
            b = h["battery"]
            cap = _f(b["capacity"])
            P[L.P["BRATE"], i] = _f(b["max_rate"])
            P[L.P["EMIN"], i] = _f(b["capacity_lower"]) * cap
            P[L.P["EMAX"], i] = _f(b["capacity_upper"]) * cap
            P[L.P["ETAC"], i] = _f(b["ch_eff"])
            P[L.P["ETAD"], i] = _f(b["disch_eff"])
            P[L.P["EINIT"], i] = _f(b["e_batt_init"]) * cap
        if "pv" in h["type"]:
            P[L.P["PVAREA"], i] = _f(h["pv"]["area"])
            P[L.P["PVEFF"], i] = _f(h["pv"]["eff"])
        ds = np.asarray(h["wh"]["draw_sizes"], dtype=float)
        draws[:len(ds), i] = ds
    return P, types, draws, dict(S=S, dt=dt, H=H, discount=disc, n_draw_hours=nd)


class MPCBatch:
    """A device-resident batch of homes that share one environment.

    Parameters
    ----------
    homes : list of home dicts (the `all_homes` records of the aggregator).
    oat, ghi, tou : full-length redis lists (aggregator.py:653-662), any sequence of floats.
    start_index : `start_hour_index` (aggregator.py:630-638).
    reward_price : the redis 'reward_price' list (length 1 or >= H, mpc_calc.py:353).
    int_mode : 'round' (default: the reference MILP -- thermal integer duty cycles by DP, the
        battery LP by an exact piecewise-linear DP), 'relax' (the LP relaxation by ADMM + exact
        vertex polish) or 'round_lp' (the relaxation for status / battery, then the integer DP).
    seed : key of the on-device season-noise stream used when no noise is supplied.
    home_offset, home_stride : global community index of home i is home_offset + i*home_stride
        (the season-noise key), so a shard draws the same numbers as the whole community.
    template_home : a home of the community, for the dims of an empty shard (homes == []):
        its steps are no-ops and its sums zero.
    exact : int_mode round: every chain the Pareto-front DP cannot take (a feasible set narrower
        than one duty step -- ~0.3 homes per 10k-home step --, mixed-sign prices without a usable
        bound, RL fronts past 2,048 labels) by the exact step-function DP (slow) instead of the
        bucketed DP's schedule (DRAGG_FLAG_EXACT).  Statuses are exact either way.
    groups : G > 1 makes a grouped batch (dims.n_groups, include/dragg_mi355x.h): G consecutive
        replicas of `homes` (N = G * len(homes), self.Nb = len(homes)), replica g solved under row g
        of the reward price ([G][n]) with its base homes' season noise -- G candidate prices against
        one community in one launch.  Its state comes from a base batch (`replicate_from`), its sums
        per group from `aggregate_groups`; `step` is its only solve (no lag mode, no explicit inputs).
    """

    def __init__(self, homes, oat=None, ghi=None, tou=None, start_index=0, reward_price=(0.0,),
                 int_mode="round", seed=0, max_iter=4000, check_every=10, device="cuda", home_offset=0,
                 home_stride=1, template_home=None, exact=False, groups=1):
        if int_mode not in L.INT_MODES:
            raise ValueError(f"int_mode must be one of {sorted(L.INT_MODES)}, not {int_mode!r}")
        if int(groups) < 1:
            raise ValueError(f"groups must be >= 1, not {groups!r}")
        self.lib = L.load()
        if not torch.cuda.is_available():
            raise L.DraggError("no GPU visible: the batched MPC has no CPU fallback")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.homes = homes
        self.names = [h["name"] for h in homes]
        P, types, draws, dm = pack_homes(homes, template_home)
        self.groups, self.Nb = int(groups), len(homes)
        if self.groups > 1:                 # replica g of base home i is home g * Nb + i
            P, types, draws = np.tile(P, (1, self.groups)), np.tile(types, self.groups), np.tile(draws, (1, self.groups))
        self.N, self.H, self.S, self.dt = self.groups * len(homes), dm["H"], dm["S"], dm["dt"]
        dev = self.device
        self.params = torch.tensor(P, dtype=torch.float64, device=dev).contiguous()
        self.types = torch.tensor(types, dtype=torch.int32, device=dev)
        self.types_host = types
        self.draws = torch.tensor(draws, dtype=torch.float64, device=dev).contiguous()
        self.dims = L.Dims(n_homes=self.N, horizon=self.H, sub_steps=self.S, dt=self.dt,
                           n_draw_hours=dm["n_draw_hours"], n_env=0, n_rp=1,
                           int_mode=L.INT_MODES[int_mode],
                           max_iter=max_iter, check_every=check_every, discount=dm["discount"],
                           flags=L.FLAG_EXACT if exact else 0, n_groups=self.groups if self.groups > 1 else 0)
        self.seed = int(seed)
        self.home_offset = int(home_offset)
        self.home_stride = int(home_stride)
        self.set_environment(oat if oat is not None else [0.0], ghi if ghi is not None else [0.0],
                             tou if tou is not None else [0.0], start_index)
        self.workspace = None
        self.lag = None
        self.n_classes, self.price_class, self.price_class_host = 1, None, None    # (set_price_classes)
        self.set_reward_price(reward_price)
        self.vals = torch.full((L.NVAL, self.N), float("nan"), dtype=torch.float64, device=dev)
        # the forecast fields <key>_<j>: stored home-contiguous ([N][NFC][H], dragg_mi355x.h: one home's
        # fields are one 5.7 KB run the solver writes with coalesced stores), seen here as the
        # [NFC][H][N] view the rest of the host code indexes
        self.fc_store = torch.full((self.N, L.NFC, self.H), float("nan"), dtype=torch.float64, device=dev)
        self.fc = self.fc_store.permute(1, 2, 0)
        self.status = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.obj = torch.zeros(self.N, dtype=torch.float64, device=dev)
        self.relax_obj = torch.zeros(self.N, dtype=torch.float64, device=dev)
        self.int_path = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self.agg = torch.zeros(3, dtype=torch.float64, device=dev)
        self.hist_row = None        # a held sweep's history row ([NVAL][N], adopt_from reads it)
        self.cycles = None
        rc = self.lib.dragg_mpc_lds_bytes(ctypes.byref(self.dims))
        if rc < 0:
            L.check(rc)
        self.lds_bytes = rc
        self._ensure_workspace()

    # ------------------------------------------------------------------ environment
    def set_environment(self, oat, ghi, tou, start_index):
        # (lag mode: a side pass still in flight holds raw pointers to the current lists, and their blocks
        # belong to the main stream's allocator pool: join it before they can be freed and reused)
        if getattr(self, "lag", None) is not None:
            self.drain()
        dev = self.device
        self.oat = torch.tensor(np.asarray(oat, dtype=float), dtype=torch.float64, device=dev)
        self.ghi = torch.tensor(np.asarray(ghi, dtype=float), dtype=torch.float64, device=dev)
        self.tou = torch.tensor(np.asarray(tou, dtype=float), dtype=torch.float64, device=dev)
        self.start_index = int(start_index)
        self.dims.n_env = int(min(len(oat), len(ghi), len(tou)))

    def set_reward_price(self, rp):
        """The redis 'reward_price' list (mpc_calc.py:630-637): host values, or a device tensor
        (e.g. an RL action broadcast over RCCL), taken without a host round trip.  A grouped batch
        takes [G][n], one list per group (every row n entries), or one list for every group; with price classes
        [G][P], [G][P][n], or one [P] / [P][n] for every group (`_lib.price_rows`)."""
        rp, n = L.price_rows(rp, getattr(self, "groups", 1), getattr(self, "n_classes", 1), self.H, self.device)
        if getattr(self, "lag", None) is not None:
            self.drain()                     # (as in set_environment: the side pass reads self.rp)
        self.rp = rp
        self.dims.n_rp = n
        if self.workspace is not None or hasattr(self, "vals"):
            self._ensure_workspace()

    def set_price_classes(self, classes, n_classes=None):
        """The community's price classes (dragg_mpc_classes): `classes`, a host int sequence [Nb], gives every
        base home a class 0 .. P - 1 (`n_classes` = P; None: the largest class + 1), shared by every group.  The
        batch then holds P reward-price rows per group (`set_reward_price`: [G][P], [G][P][n], or one [P] /
        [P][n] for every group) and `step_episodes` solves home r of group g under row (g, classes[r % Nb])
        (dragg_mpc_step_classes); state has no class, so `replicate_from` / `adopt_from` are as before.  The rows
        start over at price 0.  Like a grouped batch, a batch with P > 1 has no lag mode and no explicit solves;
        `step_episodes` is its solve.  ValueError: a wrong length, a class outside 0 .. P - 1, P outside
        1 .. CLASS_MAX -- no such map reaches the device.  P == 1 (or classes None): no classes."""
        if classes is None:
            cm, P = None, 1
        else:
            cm, P = L.price_class_map(classes, self.Nb, n_classes)
        if P > 1 and getattr(self, "lag", None) is not None:
            raise ValueError("a batch in lag mode takes no price classes")
        self.n_classes = P
        self.price_class_host = cm if P > 1 else None
        self.price_class = (torch.tensor(cm, dtype=torch.int32, device=self.device).contiguous() if P > 1 else None)
        self.set_reward_price(torch.zeros((max(getattr(self, "groups", 1), 1), P) if P > 1
                                          else (max(getattr(self, "groups", 1), 1), 1), dtype=torch.float64))

    def _classes(self):
        """The dragg_mpc_classes struct of this batch's map."""
        return L.Classes(n_classes=int(self.n_classes), price_class=L.ptr(self.price_class))

    def _ensure_workspace(self):
        """Device scratch of dragg_mpc_workspace_bytes(dims) bytes (it grows when a reward-price list makes
        RL prices possible: the cell bound's rows); the lag mode's side workspace likewise."""
        ws = self.lib.dragg_mpc_workspace_bytes(ctypes.byref(self.dims))
        if ws < 0:
            L.check(int(ws))
        need = max(1, (ws + 7) // 8) if ws > 0 else 0
        have = self.workspace.numel() if self.workspace is not None else 0
        if need > have:
            self.drain()
            self.workspace = torch.empty(need, dtype=torch.int64, device=self.device)
            if self.lag is not None:
                self.lag["side_ws"] = self._side_workspace()

    def _side_workspace(self):
        """The lag mode's side workspace: only the lists and per-block scratch of the side pass
        (dragg_mpc_side_workspace_bytes; the per-home regions stay in self.workspace)."""
        sb = self.lib.dragg_mpc_side_workspace_bytes(ctypes.byref(self.dims))
        if sb < 0:
            L.check(int(sb))
        return torch.empty(max(1, (sb + 7) // 8), dtype=torch.int64, device=self.device)

    def _region(self, name, nbytes):
        """`nbytes` of the workspace from the start of region `name` (L.workspace_regions), as uint8."""
        off = L.workspace_regions(self.dims)[name]
        return self.workspace.view(torch.uint8)[off:off + nbytes]

    def work_list(self, name):
        """A device work list of the last serial step ("deferred": hot -> mid, "steps_list": -> the step-function
        DP, "mid_list": mid -> big), after a device synchronise: (its entries as int32 [min(n, N)], its length n).
        An entry's home is `entry & L.LIST_HOME_MASK`."""
        if name not in L.WORK_LISTS:
            raise ValueError(f"a work list is one of {L.WORK_LISTS}, not {name!r}")
        torch.cuda.synchronize(self.device)
        lst = self._region(name, 4 * (self.N + 1)).view(torch.int32).cpu().numpy()
        n = int(lst[self.N])
        return lst[:min(n, self.N)], n

    def solution_rows(self):
        """The workspace's stage-slot solutions [N][H][8] float64 (a view; slot 7 is the diagnostics' pad)."""
        return self._region("solutions", self.N * self.H * 64).view(torch.float64).view(self.N, self.H, 8)

    # ------------------------------------------------------------------ structs
    def _problem(self):
        return L.Problem(params=L.ptr(self.params), home_type=L.ptr(self.types), draw_hourly=L.ptr(self.draws),
                         oat=L.ptr(self.oat), ghi=L.ptr(self.ghi), tou=L.ptr(self.tou),
                         reward_price=L.ptr(self.rp), start_index=self.start_index,
                         home_offset=self.home_offset, seed=self.seed, workspace=L.ptr(self.workspace),
                         home_stride=self.home_stride)

    def _hash(self):
        return L.Hash(vals=L.ptr(self.vals), fc=L.ptr(self.fc_store))

    def _out(self, hist=None, status=None, int_path=None, timed=True):
        """The step's outputs: `status` / `int_path` rows of the caller's (default: the batch's own);
        timed=False: no phase stamps."""
        return L.Out(status=L.ptr(status if status is not None else self.status), iters=L.ptr(self.iters),
                     obj=L.ptr(self.obj), relax_obj=L.ptr(self.relax_obj), hist=L.ptr(hist),
                     cycles=L.ptr(self.cycles if timed else None),
                     int_path=L.ptr(int_path if int_path is not None else self.int_path))

    def _call(self, fn, *args, stream=None):
        """One library call: the dims, `args` (a struct goes by reference: the argtypes of L.load),
        the launch stream (default: the current one); a non-zero return code raises."""
        L.check(fn(self.dims, *args, L.stream_ptr(stream, self.device)))

    def enable_phase_timing(self, on=True):
        """Stamp per-phase shader cycles of every home into self.cycles [NPHASE][N] (diagnostic)."""
        self.cycles = (torch.zeros((L.NPHASE, self.N), dtype=torch.int64, device=self.device) if on else None)

    # ------------------------------------------------------------------ launches
    def step(self, t, noise=None, hist=None, stream=None):
        """One closed-loop timestep for every home (run_iteration, aggregator.py:711-726)."""
        if self.n_classes > 1:
            raise ValueError("a batch with price classes is stepped by step_episodes (dragg_mpc_step_classes)")
        with torch.cuda.device(self.device):
            self.drain(stream)
            if self.lag is not None:
                self.lag["next"] = None          # the clocks no longer describe the state
            if noise is not None:
                noise = noise.to(device=self.device, dtype=torch.float64)
                if self.groups > 1 and tuple(noise.shape) == (self.H, self.Nb):
                    noise = noise.repeat(1, self.groups)        # the base homes' draws, for every replica
                noise = noise.contiguous()
                assert tuple(noise.shape) == (self.H, self.N)
            self._call(self.lib.dragg_mpc_step, self._problem(), self._hash(), self._out(hist), int(t), L.ptr(noise),
                       stream=stream)
            self._keep = (noise, hist)
            return self.status

    # ------------------------------------------------------------------ lag mode
    def enable_lag(self, ring=128):
        """Lag mode (dragg_mpc_step_main / _side, include/dragg_mi355x.h): a home whose chain needs the
        step-function DP finishes that step on a side stream while the other homes go on with their
        next steps; it catches up there.  Allocates the side pass's workspace, the per-home clocks, a
        ring of `ring` per-step list pairs (the main pass of step t + ring waits for the side pass of
        step t), the side stream and the events that order the two passes."""
        if self.dims.int_mode not in (L.INT_ROUND, L.INT_FAIL):
            raise ValueError("lag mode needs int_mode 'round' (or 'fail')")
        if self.groups > 1 or self.n_classes > 1:
            raise ValueError("a grouped batch, or one with price classes, has no lag mode (dragg_mpc_step only)")
        dev = self.device
        with torch.cuda.device(dev):
            self.lag = {
                "ring": int(ring),
                "lists": torch.zeros((ring, 2, L.lag_list_ints(self.N)), dtype=torch.int32, device=dev),
                "clock": torch.zeros(max(1, self.N), dtype=torch.int32, device=dev),
                "side_ws": self._side_workspace() if self.workspace is not None else None,
                # (a high-priority side stream, measured in round 6: no change -- the 8-way shard holding
                # home 7519 0.8476-0.8482 against 0.8457-0.8489 ms/step, profiles/r06/ab/prio*)
                "stream": torch.cuda.Stream(device=dev),
                "main_done": torch.cuda.Event(),
                "side_done": [torch.cuda.Event() for _ in range(ring)],
                "recorded": [False] * ring,
                "next": None,                   # the step the clocks are ready for
                "pending": False,               # side work not yet joined into the main stream
            }

    def step_lagged(self, t, hist, status_row, stream=None, path_row=None, sums_row=None):
        """One timestep in lag mode: the main pass on `stream` (default: the current one), the side pass
        on the side stream after it.  `hist` ([NVAL][N]), `status_row` ([N] int32) and `path_row` ([N]
        int32, the int_path bits; default self.int_path) receive the step's per-home results -- a
        lagging home's later -- so they must be this step's own rows; nothing of the step may be read
        before drain().  `sums_row` ([3] f64, optional): collect_data's sums of the step, from `hist`,
        computed on the side stream after the step's side pass (dragg_mpc_aggregate_rows)."""
        lg = self.lag
        if lg is None:
            raise RuntimeError("enable_lag() first")
        assert hist is not None and status_row is not None and status_row.dtype == torch.int32
        with torch.cuda.device(self.device):
            main = stream if stream is not None else torch.cuda.current_stream(self.device)
            side = lg["stream"]
            slot = t % lg["ring"]
            lag = L.Lag(clock=L.ptr(lg["clock"]), skipped=L.ptr(lg["lists"][slot, 0]),
                        narrow=L.ptr(lg["lists"][slot, 1]), side_workspace=L.ptr(lg["side_ws"]))
            if lg["next"] != t:
                # (the first lag-mode step, or one after a serial step: every step before t is complete)
                self.drain(main)
                self._call(self.lib.dragg_mpc_lag_reset, lag, int(t), stream=main)
            if lg["recorded"][slot]:
                main.wait_event(lg["side_done"][slot])      # the side pass of step t - ring is done with the lists
            step = (self._problem(), self._hash(), self._out(hist, status_row, path_row, timed=False), int(t), lag)
            self._call(self.lib.dragg_mpc_step_main, *step, stream=main)
            lg["main_done"].record(main)
            side.wait_event(lg["main_done"])
            self._call(self.lib.dragg_mpc_step_side, *step, stream=side)
            if sums_row is not None:
                self._call(self.lib.dragg_mpc_aggregate_rows, L.ptr(hist), 1, L.ptr(sums_row), stream=side)
            lg["side_done"][slot].record(side)
            lg["recorded"][slot] = True
            lg["last"] = slot
            lg["next"] = t + 1
            lg["pending"] = True
            self._keep = (hist, status_row, path_row, sums_row)

    def drain(self, stream=None):
        """Join the side stream into `stream` (default: the current one): after this, everything the
        lag-mode steps wrote is visible in stream order."""
        lg = self.lag
        if lg is None or not lg["pending"]:
            return
        main = stream if stream is not None else torch.cuda.current_stream(self.device)
        main.wait_event(lg["side_done"][lg["last"]])
        lg["pending"] = False

    def aggregate_rows(self, rows, stream=None):
        """collect_data sums of every history row of `rows` ([T][NVAL][N]) -> [T][3] (bit-identical to
        aggregate() on each row)."""
        with torch.cuda.device(self.device):
            out = torch.empty((rows.shape[0], 3), dtype=torch.float64, device=self.device)
            self._call(self.lib.dragg_mpc_aggregate_rows, L.ptr(rows.contiguous()), int(rows.shape[0]), L.ptr(out),
                       stream=stream)
            return out

    def solve_explicit(self, t, T0, Tw0, E0, counter, winter, draw, oat, ghi, price, stream=None):
        """Independent per-home solves with explicit inputs ([N] and [H+1 or H][N] arrays)."""
        dev, N, H = self.device, self.N, self.H
        if self.n_classes > 1:
            raise ValueError("a batch with price classes takes no explicit inputs (they carry no price list)")

        def d(x, shape, dtype=torch.float64):
            return torch.as_tensor(np.asarray(x), dtype=dtype).to(dev).reshape(shape).contiguous()
        with torch.cuda.device(dev):
            self.drain(stream)
            ex_t = {
                "t": d(t, (N,), torch.int32), "T0": d(T0, (N,)), "Tw0": d(Tw0, (N,)),
                "E0": d(np.nan_to_num(np.asarray(E0, dtype=float)), (N,)),
                "counter": d(counter, (N,), torch.int32), "winter": d(winter, (N,), torch.int32),
                "draw": d(draw, (H + 1, N)), "oat": d(oat, (H + 1, N)), "ghi": d(ghi, (H + 1, N)),
                "price": d(price, (H, N)),
            }
            ex = L.Explicit(**{k: L.ptr(v) for k, v in ex_t.items()})
            self._call(self.lib.dragg_mpc_solve_explicit, self._problem(), ex, self._hash(), self._out(), stream=stream)
            self._keep = ex_t
            return self.status

    def aggregate(self, stream=None):
        """collect_data sums (aggregator.py:751-753) -> device tensor [agg_load, forecast_load, agg_cost].
        A home whose fields are absent (a crashed home: the reference raises KeyError in
        collect_data, aggregator.py:750-752) makes the sums NaN."""
        with torch.cuda.device(self.device):
            self.drain(stream)
            self._call(self.lib.dragg_mpc_aggregate, self._hash(), L.ptr(self.agg), stream=stream)
            return self.agg

    # ------------------------------------------------------------------ grouped batches
    def replicate_from(self, base, stream=None):
        """Copy `base`'s hash arrays (vals, fc: the state a step reads) into every replica of this
        grouped batch, bit for bit, in one kernel (dragg_mpc_replicate).  `base` is only read.  `base` may
        itself be a grouped batch of E groups: this batch (C * E groups) then holds C copies of it,
        copy-major -- copy c of base group e is group c * E + e."""
        copies = self.groups // max(getattr(base, "groups", 1), 1)
        if base.N * copies != self.N or copies * getattr(base, "groups", 1) != self.groups or base.H != self.H:
            raise ValueError(f"replicate_from: {self.groups} replicas of {self.Nb} homes (H = {self.H}) cannot "
                             f"take a batch of {base.N} homes (H = {base.H})")
        with torch.cuda.device(self.device):
            base.drain(stream)
            dims = L.Dims.from_buffer_copy(self.dims)
            dims.n_groups = copies if copies > 1 else 0
            L.check(self.lib.dragg_mpc_replicate(dims, base._hash(), self._hash(), L.stream_ptr(stream, self.device)))

    def adopt_from(self, src, choice, hist=None, stream=None):
        """The way back (dragg_mpc_adopt): `src` holds C copies of this batch, copy-major (what
        `replicate_from(self)` fills and a step then solves); group e of this batch takes the columns of copy
        `choice[e]` -- vals, fc, status, iters, obj, relax_obj, int_path, and `src.hist_row` ([NVAL][C * N],
        the history row the source's step wrote) into `hist` ([NVAL][N]) where both are given -- bit for
        bit.  `choice`: a contiguous device int32 [E]; an entry outside [0, C) leaves its group untouched.
        `src` is only read (an MPCBatch, or anything with its arrays: a clone of them).  No synchronisation."""
        E = max(self.groups, 1)
        copies = src.N // self.N if self.N else max(getattr(src, "groups", 1), 1) // E
        if copies < 1 or src.N != copies * self.N or src.H != self.H:
            raise ValueError(f"adopt_from: a batch of {self.N} homes (H = {self.H}) cannot adopt from "
                             f"{src.N} homes (H = {src.H}): the source holds whole copies of it")
        L.device_arg(choice, "choice", self.device, torch.int32, (E,))
        row = getattr(src, "hist_row", None)
        with torch.cuda.device(self.device):
            self.drain(stream)
            src_out = L.Out(status=L.ptr(src.status), iters=L.ptr(src.iters), obj=L.ptr(src.obj),
                            relax_obj=L.ptr(src.relax_obj), hist=L.ptr(row if hist is not None else None),
                            cycles=None, int_path=L.ptr(src.int_path))
            L.check(self.lib.dragg_mpc_adopt(self.dims, copies, L.ptr(choice),
                                             L.Hash(vals=L.ptr(src.vals), fc=L.ptr(src.fc_store)), src_out,
                                             self._hash(), self._out(hist if row is not None else None, timed=False),
                                             L.stream_ptr(stream, self.device)))
            self._keep = (src, choice, hist)

    def select_groups(self, sums, target, prices, stream=None):
        """The choice for `adopt_from`, made on the device (dragg_mpc_select_groups): `sums` [C * E][3]
        (`aggregate_groups` of the copies' batch), `target` [E], `prices` [C * E][n] (its reward-price rows)
        -> device int32 [E]: per group the copy whose load lies closest to the target, ties to the smaller
        |price|, then the smaller copy; -1 where every load is NaN.  No synchronisation."""
        E = max(self.groups, 1)
        sums = L.device_f64(sums, self.device).contiguous()
        target = L.device_f64(target, self.device).reshape(-1).contiguous()
        prices = L.device_f64(prices, self.device)
        if sums.dim() != 2 or sums.shape[1] != 3 or sums.shape[0] < E or sums.shape[0] % E or target.numel() != E:
            raise ValueError(f"select_groups takes sums [C * {E}][3] and target [{E}], not {list(sums.shape)} "
                             f"and {list(target.shape)}")
        prices = prices.reshape(sums.shape[0], -1).contiguous()
        with torch.cuda.device(self.device):
            choice = torch.empty(E, dtype=torch.int32, device=self.device)
            L.check(self.lib.dragg_mpc_select_groups(self.dims, sums.shape[0] // E, L.ptr(sums), L.ptr(target),
                                                     L.ptr(prices), int(prices.shape[1]), L.ptr(choice),
                                                     L.stream_ptr(stream, self.device)))
            self._keep = (sums, target, prices)
            return choice

    def select_paths(self, sums, ran, tracked, target, weights, prices, num_timesteps, fresh_load, score=None,
                     stream=None):
        """The choice for `adopt_from` over K-step rollouts, made on the device (dragg_mpc_select_paths): `sums`
        [K][C * E][3] (`aggregate_groups` of the copies' batch after each rollout step), `ran` int32 [E] (the
        clocks step 0 ran with; outside [0, num_timesteps): no step), `tracked` [E][P] and `target` [E] (the
        setpoint rule's tracked loads and setpoint now), `weights` [K], `prices` [C * E][n] -- contiguous device
        tensors, read as they are.  Per episode the candidate of least weighted distance between its loads and
        the setpoints the rule would file if it were played; ties to the smaller |price|, then the smaller copy;
        -1 where none is valid.  `score`: a contiguous device float64 tensor of C * E entries for the scores
        (copy-major), or None.  -> device int32 [E].  No synchronisation."""
        E = max(self.groups, 1)
        dev = self.device
        for name, x, dt in (("sums", sums, torch.float64), ("ran", ran, torch.int32), ("tracked", tracked, torch.float64),
                            ("target", target, torch.float64), ("weights", weights, torch.float64),
                            ("prices", prices, torch.float64), ("score", score, torch.float64)):
            if x is None and name == "score":
                continue
            L.device_arg(x, f"select_paths: {name}", dev, dt)
        if sums.dim() != 3 or sums.shape[2] != 3 or sums.shape[1] < E or sums.shape[1] % E or sums.shape[0] < 1:
            raise ValueError(f"select_paths takes sums [K][C * {E}][3], not {list(sums.shape)}")
        K, CE = int(sums.shape[0]), int(sums.shape[1])
        if tracked.dim() != 2 or tracked.shape[0] != E or ran.numel() != E or target.numel() != E \
                or weights.numel() != K or prices.dim() != 2 or prices.shape[0] != CE \
                or (score is not None and score.numel() != CE):
            raise ValueError(f"select_paths takes ran [{E}], tracked [{E}][P], target [{E}], weights [{K}], prices "
                             f"[{CE}][n] and score [{CE}]")
        with torch.cuda.device(dev):
            choice = torch.empty(E, dtype=torch.int32, device=dev)
            p = L.Paths(steps=K, num_timesteps=int(num_timesteps), prev_timesteps=int(tracked.shape[1]),
                        fresh_load=float(fresh_load), sums=L.ptr(sums), ran=L.ptr(ran), tracked=L.ptr(tracked),
                        target=L.ptr(target), weights=L.ptr(weights), prices=L.ptr(prices),
                        n_rp=int(prices.shape[1]), choice=L.ptr(choice), score=L.ptr(score))
            L.check(self.lib.dragg_mpc_select_paths(self.dims, CE // E, p, L.stream_ptr(stream, dev)))
            self._keep = (sums, ran, tracked, target, weights, prices, score)
            return choice

    def aggregate_groups(self, stream=None, out=None):
        """collect_data's sums of every group -> device tensor [G][3]; row g is bit-identical to
        aggregate() of a batch holding replica g's homes (dragg_mpc_aggregate_groups).  `out`: a contiguous
        device float64 tensor of G * 3 entries to write instead of the batch's own rows."""
        with torch.cuda.device(self.device):
            if out is None:
                if getattr(self, "agg_groups", None) is None:
                    self.agg_groups = torch.zeros((self.groups, 3), dtype=torch.float64, device=self.device)
                out = self.agg_groups
            else:
                L.device_arg(out, "aggregate_groups: out", self.device, torch.float64, numel=self.groups * 3)
            self._call(self.lib.dragg_mpc_aggregate_groups, self._hash(), L.ptr(out), stream=stream)
            return out

    # ------------------------------------------------------------------ plan observations
    def plan_groups(self, keys, rows=(), out=None, stream=None, src=None, classes=False):
        """The planned curves of every group (dragg_mpc_plan_groups) -> (curve [G][nk][H] float64, count
        [G][nk][H] int32, stats [G][nr][4] float64: count, sum, min, max) as device tensors.  `keys`: the forecast
        keys whose time-aligned horizon curve is summed over each group's homes, `rows`: the vals rows whose
        statistics are taken (names of L.PLAN_KEYS / L.PLAN_ROWS or indices; the outputs hold them in ascending
        index order).  Entry 0 of a curve is the collected value, entry j the homes' plan j stages ahead of the
        wall clock (a home in fallback: its stale plan, shifted by its solve counter); absent values (NaN) add
        nothing and `count` says how many homes stand behind each sum.  The summation order is fixed (16 partial
        sums over homes w, w + 16, ..., then a balanced tree: `vector.plan_groups_reference`), so a group's rows
        do not depend on the batch around it.  The hash arrays are only read.  `out`: a (curve, count, stats)
        triple to write into instead of new tensors; `src`: another holder of hash arrays of this horizon (vals,
        fc_store, N, groups -- a held sweep's replicas) in place of this batch's.  No synchronisation.
        classes=True: per (group, price class) of this batch's map (dragg_mpc_plan_classes) -> curve and count
        [G][P][nk][H], stats [G][P][nr][4]; class c's rows are the group's rows with every home of another class
        absent (`vector.plan_classes_reference`), an empty class's the empty result.  Without a map (P == 1) the
        class axis has length 1 and the rows are plan_groups' own."""
        km, rm, ki, ri = L.plan_select(keys, rows)
        b = self if src is None else src
        G = max(int(getattr(b, "groups", 1)), 1)
        if b.H != self.H:
            raise ValueError(f"plan_groups: a source of horizon {b.H}, not {self.H}")
        lead = (G, int(self.n_classes)) if classes else (G,)
        shapes = {"curve": (lead + (len(ki), self.H), torch.float64), "count": (lead + (len(ki), self.H), torch.int32),
                  "stats": (lead + (len(ri), len(L.PLAN_STATS)), torch.float64)}
        with torch.cuda.device(self.device):
            if out is None:
                out = tuple(torch.empty(s, dtype=d, device=self.device) for s, d in shapes.values())
            for t, (name, (s, d)) in zip(out, shapes.items()):
                L.device_arg(t, f"plan_groups: out's {name}", self.device, d, s)
            if src is None:
                self.drain(stream)
            dims = L.Dims.from_buffer_copy(self.dims)
            dims.n_homes, dims.n_groups = int(b.N), G if G > 1 else 0
            plan = L.Plan(fc_keys=km, val_rows=rm, curve=L.ptr(out[0]), count=L.ptr(out[1]), stats=L.ptr(out[2]))
            h = L.Hash(vals=L.ptr(b.vals), fc=L.ptr(b.fc_store))
            if classes:
                L.check(self.lib.dragg_mpc_plan_classes(dims, h, self._classes(), plan, L.stream_ptr(stream, self.device)))
            else:
                L.check(self.lib.dragg_mpc_plan_groups(dims, h, plan, L.stream_ptr(stream, self.device)))
            self._keep = (src, out)
            return tuple(out)

    # ------------------------------------------------------------------ device-resident environment
    def _env(self, st, ran=None, sums=None):
        """The dragg_mpc_env struct of an environment state (`dragg_amd.vector.EnvState`: scalars, the state
        tensors and the history stores, None where a store is not kept)."""
        return L.Env(num_timesteps=int(st.num_timesteps), prev_timesteps=int(st.prev_timesteps),
                     max_poss_load=float(st.max_poss_load), start_load=float(st.start_load), ran=L.ptr(ran),
                     clock=L.ptr(st.clock), max_load=L.ptr(st.max_load), min_load=L.ptr(st.min_load),
                     tracked=L.ptr(st.tracked), obs=L.ptr(st.obs), sums=L.ptr(sums),
                     status_hist=L.ptr(st.status_hist), path_hist=L.ptr(st.path_hist), hist=L.ptr(st.hist),
                     agg_hist=L.ptr(st.agg_hist))

    def env_file(self, st, ran, sums, hist=None, stream=None):
        """After a step that ran with the timesteps `ran` (device int32 [G]; negative: idle): file the step's
        status, int_path and history row (`hist` [NVAL][N]) at row ran[g] of the stores of `st`, the sums
        (`sums` [G][3], `aggregate_groups`') into its agg_hist, advance its clocks and update the environment
        state and observations -- one kernel (dragg_mpc_env_file).  No synchronisation."""
        with torch.cuda.device(self.device):
            out = L.Out(status=L.ptr(self.status), hist=L.ptr(hist if st.hist is not None else None),
                        int_path=L.ptr(self.int_path if st.path_hist is not None else None))
            self._call(self.lib.dragg_mpc_env_file, self._env(st, ran, sums), out, stream=stream)
            self._keep = (ran, sums, hist)

    def env_reset(self, st, mask, stream=None):
        """Start the masked groups (`mask`: device bool [G]) over: their columns of vals and fc NaN, their
        columns of every store of `st` cleared, clock 0, the environment state of a fresh episode -- one
        kernel (dragg_mpc_env_reset) that touches the masked groups' columns only.  No synchronisation."""
        with torch.cuda.device(self.device):
            self.drain(stream)
            L.check(self.lib.dragg_mpc_env_reset(self.dims, self._env(st), L.ptr(mask), self._hash(),
                                                 L.stream_ptr(stream, self.device)))
            self._keep = (mask,)

    def season_noise(self, t, stream=None):
        with torch.cuda.device(self.device):
            out = torch.empty((self.H, self.N), dtype=torch.float64, device=self.device)
            self._call(self.lib.dragg_mpc_season_noise, self.seed, self.home_offset, self.home_stride, int(t),
                       L.ptr(out), stream=stream)
            return out

    # ------------------------------------------------------------------ vectorised episodes
    def _episodes(self, seeds, starts, clocks):
        """The dragg_mpc_episodes struct of device tensors [G] (None: the member stays NULL, the shared
        value for every group) and the tensors it points to."""
        G, dev = self.groups, self.device

        keep = (None if seeds is None else L.device_arg(seeds, "seeds", dev, SEED_DTYPES, (G,)),
                None if starts is None else L.device_arg(starts, "starts", dev, torch.int32, (G,)),
                None if clocks is None else L.device_arg(clocks, "clocks", dev, torch.int32, (G,)))
        return L.Episodes(seed=L.ptr(keep[0]), start_index=L.ptr(keep[1]), timestep=L.ptr(keep[2])), keep

    def step_episodes(self, seeds, starts, clocks, noise=None, hist=None, stream=None, t=0):
        """One step of a batch of episodes (dragg_mpc_step_episodes): group g with its own season-noise
        seed `seeds[g]` (int64 / uint64 [G], the bits are the key), start index `starts[g]` and timestep
        `clocks[g]` (int32 [G]; negative: the group is idle and nothing of it is written), all device
        tensors read by the kernels -- no host synchronisation.  None for any of them: the batch's own
        seed / start_index / `t` for every group."""
        with torch.cuda.device(self.device):
            ep, keep = self._episodes(seeds, starts, clocks)
            if noise is not None:
                noise = noise.to(device=self.device, dtype=torch.float64).contiguous()
                assert tuple(noise.shape) == (self.H, self.N)
            if self.n_classes > 1:
                self._call(self.lib.dragg_mpc_step_classes, self._problem(), ep, self._classes(), self._hash(),
                           self._out(hist), int(t), L.ptr(noise), stream=stream)
            else:
                self._call(self.lib.dragg_mpc_step_episodes, self._problem(), ep, self._hash(), self._out(hist), int(t),
                           L.ptr(noise), stream=stream)
            self._keep = (noise, hist, keep)
            return self.status

    def season_noise_episodes(self, seeds, clocks, out=None, stream=None, t=0):
        """The keyed season draw [H][N] of a batch of episodes (dragg_mpc_season_noise_episodes): group g
        draws the stream of (seeds[g], base home, clocks[g]); an idle group's columns keep `out`'s values
        (NaN in a fresh tensor)."""
        with torch.cuda.device(self.device):
            ep, keep = self._episodes(seeds, None, clocks)
            if out is None:
                out = torch.full((self.H, self.N), float("nan"), dtype=torch.float64, device=self.device)
            self._call(self.lib.dragg_mpc_season_noise_episodes, ep, self.home_offset, self.home_stride, int(t),
                       L.ptr(out), stream=stream)
            self._keep = (keep, out)
            return out

    # ------------------------------------------------------------------ hash views
    def hash_dict(self, i, as_str=True):
        """The home's redis hash as `hgetall` would return it (str values, absent fields omitted)."""
        self.drain()
        vals = self.vals[:, i].cpu().numpy()
        fc = self.fc[:, :, i].cpu().numpy()
        out = {}
        for k, name in enumerate(L.FC_KEYS):
            for j in range(self.H):
                if not np.isnan(fc[k, j]):
                    out[f"{name}_{j}"] = fc[k, j]
        for k, name in enumerate(L.VAL_KEYS):
            if not np.isnan(vals[k]):
                out[name] = vals[k]
        if "solve_counter" in out:
            out["solve_counter"] = int(out["solve_counter"])
        if "correct_solve" in out:
            out["correct_solve"] = int(out["correct_solve"])
        if as_str:
            out = {k: (str(v) if isinstance(v, int) else repr(float(v))) for k, v in out.items()}
        return out
