"""The members of a community as one unit: the homes' batch and, where the community has vehicles, their fleet.

`Members` holds an `MPCBatch` and an `EVFleet` (None: homes only) of the same groups and makes, homes first, the moves
the aggregators make on both: publish price rows, step the episodes, sum, replicate into a sweep's copies and adopt
a chosen copy back.  `Held` keeps the arrays such an adoption reads -- a sweep's first step -- while the replicas move
on.  Nothing here launches anything of its own: every method is the batch's call followed by the fleet's.
"""
from types import SimpleNamespace

import torch

# the arrays `MPCBatch.adopt_from` / `EVFleet.adopt_from` read of their source: a solved step
BATCH_ARRAYS = ("vals", "fc_store", "status", "iters", "obj", "relax_obj", "int_path")
FLEET_ARRAYS = ("vals", "fc_store", "status", "obj")


class Members:
    def __init__(self, batch, fleet=None, homes=None, batch_args=None, fleet_args=None, classes=None):
        """`homes`, `batch_args` and `fleet_args` ((class, keyword arguments) each) build another batch / fleet of
        the same community (`replica`, `new_fleet`); `classes`: its price classes (map [Nb] by home, P), or None."""
        self.batch, self.fleet, self.homes = batch, fleet, homes
        self.batch_args, self.fleet_args, self.classes = batch_args, fleet_args, classes
        self.replicas = {}           # key (default: the groups) -> the replica unit of a sweep

    def new_fleet(self, tou, groups):
        """A fleet of `groups` groups of the community's vehicles over `tou` (environment index 0 first), with the
        owners' price classes."""
        cls, kw = self.fleet_args
        f = cls(self.homes, tou, start_index=0, groups=groups, **kw)
        if self.classes is not None:
            cm, P = self.classes
            f.set_price_classes([int(cm[i]) for i in f.owners], P)
        return f

    def replica(self, groups, key=None):
        """The `groups`-group copy of this unit for a sweep, built once per `key`: the same homes and class map, a
        fleet over the live fleet's TOU list where there is one, and the live batch's environment as it is now (the
        same device tensors)."""
        key = groups if key is None else key
        r = self.replicas.get(key)
        if r is None:
            cls, kw = self.batch_args
            rb = cls(self.homes, None, None, None, 0, (0.0,), groups=groups, **kw)
            if self.classes is not None:
                rb.set_price_classes(*self.classes)
            rf = self.new_fleet(self.fleet.tou, groups) if self.fleet is not None else None
            r = self.replicas[key] = Members(rb, rf)
        for k in ("oat", "ghi", "tou", "start_index"):
            if hasattr(self.batch, k):
                setattr(r.batch, k, getattr(self.batch, k))
        if hasattr(self.batch, "dims"):
            r.batch.dims.n_env = self.batch.dims.n_env
        return r

    # ------------------------------------------------------------------ the moves, homes first
    def set_reward_price(self, rows):
        self.batch.set_reward_price(rows)
        if self.fleet is not None:
            self.fleet.set_reward_price(rows)

    def step_episodes(self, seeds, starts, clocks, noise=None, hist=None):
        """One step of every group at its own start index and clock (the vehicles have no season noise)."""
        self.batch.step_episodes(seeds, starts, clocks, noise=noise, hist=hist)
        if self.fleet is not None:
            self.fleet.step_episodes(starts, clocks)

    def sums(self, out=None):
        """[G][3]: the homes' sums, plus the vehicles' (added in place; their own rows stay in `fleet.sums`)."""
        agg = self.batch.aggregate_groups() if out is None else self.batch.aggregate_groups(out=out)
        if self.fleet is not None:
            self.fleet.aggregate_onto(agg)
        return agg

    def replicate_from(self, live):
        self.batch.replicate_from(live.batch)
        if self.fleet is not None:
            self.fleet.replicate_from(live.fleet)

    def adopt_from(self, held, choice, hist=None):
        """`held`: the unit that holds the copies -- a replica `Members`, or a `Held`."""
        self.batch.adopt_from(held.batch, choice, hist=hist)
        if self.fleet is not None:
            self.fleet.adopt_from(held.fleet, choice)

    def reset_fleet(self, mask):
        """Start the fleet's masked groups over (the homes' reset is their aggregator's)."""
        if self.fleet is not None:
            self.fleet.reset_groups(mask)

    def snapshot(self):
        snap = (self.batch.vals.clone(), self.batch.fc.clone())
        return snap + (self.fleet.snapshot(),) if self.fleet is not None else snap

    def restore(self, snap):
        self.batch.vals.copy_(snap[0])
        self.batch.fc.copy_(snap[1])
        if self.fleet is not None:
            self.fleet.restore(snap[2])


class Held:
    """The first step of a sweep, kept while its replicas move on: the arrays `Members.adopt_from` reads.  The
    homes' arrays are its own attributes (it stands where a replica batch stands: `adopt_from`, `plan_groups(src=)`),
    so it is its own `batch` (a property: no stored reference to itself, and a dropped holder is freed at once);
    `fleet` holds the vehicles' (None without a fleet).  Allocated once and refilled with
    `copy_`: a holder that is kept (one per C in the vector environments) never calls the allocator again."""

    batch = property(lambda self: self)

    def __init__(self, members):
        rb = members.batch
        self.N, self.H, self.groups, self.hist_row = rb.N, rb.H, getattr(rb, "groups", 1), None
        for k in BATCH_ARRAYS:
            v = getattr(rb, k, None)
            setattr(self, k, torch.empty_like(v) if v is not None else None)
        # (fc is a view of fc_store where a batch has one: MPCBatch)
        self.fc = self.fc_store.permute(1, 2, 0) if self.fc_store is not None else torch.empty_like(rb.fc)
        self._filled = BATCH_ARRAYS if self.fc_store is not None else BATCH_ARRAYS + ("fc",)
        self.fleet = None
        if members.fleet is not None:
            f = members.fleet
            self.fleet = SimpleNamespace(M=f.M, H=f.H, groups=f.groups,
                                         **{k: torch.empty_like(getattr(f, k)) for k in FLEET_ARRAYS})

    def fill(self, members, hist_row=None):
        """Copy the unit's solved step; `hist_row`: the history row that step wrote (kept, not copied: only a
        sweep's first step writes it)."""
        for dst, src, names in ((self, members.batch, self._filled), (self.fleet, members.fleet, FLEET_ARRAYS)):
            for k in names if dst is not None else ():
                if getattr(dst, k) is not None:
                    getattr(dst, k).copy_(getattr(src, k))
        self.hist_row = hist_row
        return self
