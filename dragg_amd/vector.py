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

One rank only: sharding episodes over ranks is not built.
"""
import numpy as np
import torch

from . import _lib as L
from .mpc import MPCBatch


def _seed_i64(s):
    """A uint64 seed as the int64 with the same bits (the tensors are int64)."""
    s = int(s) & (2 ** 64 - 1)
    return s - 2 ** 64 if s >= 2 ** 63 else s


class VectorAggregator:
    def __init__(self, homes, oat, ghi, tou, episodes, seeds, start_indices, num_timesteps, int_mode="round",
                 keep_history=True, device=None, batch_cls=MPCBatch, rank=0, world=1, **batch_kw):
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
        self._batch_args = (batch_cls, dict(int_mode=int_mode, device=dev, **batch_kw))
        self._sweep_batches = {}     # C -> the C * E-group batch of sweep()
        # a held sweep (sweep -> commit) and the moves of the live state that void it (step, reset, commit)
        self._hold = None
        self._gen = 0
        self.adopted = torch.zeros(E, dtype=torch.bool, device=dev)      # the episodes the last commit advanced

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
        self.agg_hist.copy_(torch.where(m[None, :, None], torch.zeros((), dtype=torch.float64, device=self.device),
                                        self.agg_hist))

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

    def step(self, prices, noise=None):
        """One step of every active episode under `prices` ([E], or [E][n] with n == 1 or n >= H: row e is
        episode e's reward-price list); the others stay idle.  -> device tensor [E][3], collect_data's
        [agg_load, forecast_load, agg_cost] per episode (an idle episode's row: its state's, i.e. its last
        step's sums, NaN before its first).  The active clocks advance on the device."""
        P = L.device_f64(prices, self.device)
        if P.dim() == 1:
            P = P.reshape(-1, 1)
        if P.dim() != 2 or P.shape[0] != self.E:
            raise ValueError(f"step takes prices [{self.E}] or [{self.E}][n], not {list(P.shape)}")
        b = self.batch
        self._gen += 1
        b.set_reward_price(P.contiguous())
        on = self.active()
        eff = torch.where(on, self.clocks, torch.full_like(self.clocks, -1))
        if self._row is not None:
            # (a home that hits ERR_MISSING writes no history: its row entries stay NaN, as in a single run's
            # fresh history row)
            self._row.fill_(float("nan"))
        b.step_episodes(self.seeds, self.starts, eff, noise=noise, hist=self._row)
        self._keep = eff
        return self._file(on)

    def _file(self, on):
        """After a step of the episodes `on` (solved, or adopted): their sums, the step's rows filed at each
        episode's own clock, the clocks advanced.  -> [E][3]"""
        b = self.batch
        agg = b.aggregate_groups()
        idx = self.clocks.clamp(0, self.num_timesteps - 1).to(torch.int64)
        if self.hist is not None:
            self._scatter(self.hist, self._row, idx, on)
        self._scatter(self.status_hist, b.status, idx, on)
        if hasattr(b, "int_path"):
            self._scatter(self.path_hist, b.int_path, idx, on)
        a = self.agg_hist                                        # [T][E][3]
        ai = idx.view(1, self.E, 1).expand(1, self.E, 3)
        a.scatter_(0, ai, torch.where(on.view(1, self.E, 1), agg.view(1, self.E, 3), a.gather(0, ai)))
        self.clocks = self.clocks + on.to(torch.int32)
        return agg

    # ------------------------------------------------------------------ sweep, select, commit
    # C candidate prices per episode, one step ahead: a batch of C * E groups holds C copies of the live
    # E-group batch, copy-major (group c * E + e = episode e under its candidate c), filled by
    # dragg_mpc_replicate and stepped once with the episodes' keys and clocks tiled C times.  `commit` then
    # adopts, per episode, the chosen copy's solved step (dragg_mpc_adopt) instead of solving it again; the
    # choice can be made on the device (`select`), so none of this synchronises with the host.
    def _sweep_batch(self, C):
        rb = self._sweep_batches.get(C)
        if rb is None:
            cls, kw = self._batch_args
            rb = cls(self.homes, None, None, None, 0, (0.0,), groups=C * self.E, **kw)
            self._sweep_batches[C] = rb
        for k in ("oat", "ghi", "tou", "start_index"):           # the live batch's environment (the same tensors)
            if hasattr(self.batch, k):
                setattr(rb, k, getattr(self.batch, k))
        if hasattr(self.batch, "dims"):
            rb.dims.n_env = self.batch.dims.n_env
        return rb

    def sweep(self, prices, hold=True):
        """Every active episode's next step under each of its C candidate prices (`prices` [E][C], or
        [E][C][n] with n == 1 or n >= H), nothing committed -> device tensor [E][C][3], row (e, c)
        bit-identical to what `step` returns for episode e under prices[e][c] (an idle episode's rows: its
        state's sums).  One step ahead only.  The live batch is only read.  hold=True (default) keeps the
        solved replicas for `commit`."""
        P = L.device_f64(prices, self.device)
        if P.dim() == 2:
            P = P.unsqueeze(-1)
        if P.dim() != 3 or P.shape[0] != self.E or P.shape[1] < 1:
            raise ValueError(f"sweep takes prices [{self.E}][C] or [{self.E}][C][n], not {list(P.shape)}")
        C = int(P.shape[1])
        Pc = P.permute(1, 0, 2).contiguous()                     # copy-major: [C][E][n]
        self._hold = None
        rb = self._sweep_batch(C)
        rb.set_reward_price(Pc.view(C * self.E, -1))
        rb.replicate_from(self.batch)
        on = self.active()
        eff = torch.where(on, self.clocks, torch.full_like(self.clocks, -1))
        if hold and self._row is not None:
            if getattr(rb, "hist_row", None) is None:
                rb.hist_row = torch.empty((L.NVAL, rb.N), dtype=torch.float64, device=self.device)
            rb.hist_row.fill_(float("nan"))
        keys = (self.seeds.repeat(C), self.starts.repeat(C), eff.repeat(C))
        rb.step_episodes(*keys, hist=rb.hist_row if hold and self._row is not None else None)
        sums = rb.aggregate_groups().view(C, self.E, 3)
        if hold:
            self._hold = {"C": C, "P": Pc, "gen": self._gen, "on": on, "src": rb, "keys": keys}
        return sums.permute(1, 0, 2).contiguous()

    def select(self, sums, setpoints, prices):
        """Per episode the candidate whose load (`sums` [E][C][3], `sweep`'s) lies closest to its setpoint
        (`setpoints` [E]); ties to the smaller |price| (`prices` [E][C] or [E][C][n]: its first entry), then the
        smaller index; -1 where no candidate has a load -> device int32 [E] (dragg_mpc_select_groups)."""
        S = L.device_f64(sums, self.device)
        P = L.device_f64(prices, self.device)
        if S.dim() != 3 or S.shape[0] != self.E or S.shape[2] != 3:
            raise ValueError(f"select takes sums [{self.E}][C][3], not {list(S.shape)}")
        C = int(S.shape[1])
        P = P.reshape(self.E, C, -1).permute(1, 0, 2).reshape(C * self.E, -1)
        return self.batch.select_groups(S.permute(1, 0, 2).reshape(C * self.E, 3), setpoints, P)

    def commit(self, choice):
        """Play, per episode, candidate choice[e] of the held sweep (`choice`: a device int tensor [E]): its
        solved step becomes the episode's step, as `step` under the chosen price rows would have left it, bit
        for bit.  An entry outside [0, C) -- and every episode that was idle in the sweep or is idle now --
        adopts nothing and stays where it is.  The chosen rows become the live batch's reward price (an
        episode that adopted nothing: its candidate 0's row, which nothing reads).  -> [E][3], the episodes'
        sums as `step` returns them; `self.adopted` (device bool [E]) holds the episodes that advanced."""
        h = self._hold
        if h is None or h["gen"] != self._gen:
            raise ValueError("commit: no sweep of the live state is held (sweep first; a step or a reset voids it)")
        C, rb, b = h["C"], h["src"], self.batch
        if not torch.is_tensor(choice) or tuple(choice.shape) != (self.E,) or choice.dtype.is_floating_point:
            raise ValueError(f"commit takes a device int tensor [{self.E}]")
        self._hold = None
        ch = choice.to(device=self.device, dtype=torch.int32)
        on = h["on"] & self.active() & (ch >= 0) & (ch < C)
        ch = torch.where(on, ch, torch.full_like(ch, -1)).contiguous()
        self._gen += 1
        rows = h["P"][ch.clamp(0, C - 1).to(torch.int64), torch.arange(self.E, device=self.device)]
        b.set_reward_price(rows.contiguous())
        if self._row is not None:
            self._row.fill_(float("nan"))
        b.adopt_from(rb, ch, hist=self._row)
        self.adopted = on
        return self._file(on)

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
