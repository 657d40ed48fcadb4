"""The homes-and-vehicles unit, host side (CPU): `_lib.price_rows` and `_lib.device_arg` (the one parser of a reward
price's shapes and the one check of a launch's tensor arguments), `members.Held`, and `members.Members` on the
stand-in batch and fleet of tests/test_ev_vector_host.py against the direct calls on both."""
import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from dragg_amd.members import BATCH_ARRAYS, FLEET_ARRAYS, Held, Members
from tests.test_ev_vector_host import CLASSES, DAY0, HOMES, SEEDS, StandInFleet, _bits, _fleet_equal
from tests.test_classes_host import CPU, ENV, ClassBatch

G, P, H = 2, 3, 4


# ------------------------------------------------------------------ price_rows
def _rows(rp, G=G, P=P):
    flat, n = L.price_rows(rp, G, P, H, CPU)
    assert flat.dtype == torch.float64 and flat.dim() == 1 and flat.is_contiguous() and flat.numel() == G * P * n
    return flat.tolist(), n


def test_price_rows_takes_every_form():
    # one group, one class: one list, whatever its shape
    assert _rows([0.5], 1, 1) == ([0.5], 1) and _rows((0.25,), 1, 1) == ([0.25], 1)
    assert _rows(np.arange(5.0), 1, 1) == ([0.0, 1.0, 2.0, 3.0, 4.0], 5)
    assert _rows(torch.arange(4.0).reshape(1, 4), 1, 1) == ([0.0, 1.0, 2.0, 3.0], 4)
    # G groups: [n] for every group, [G][n]
    assert _rows([0.5], P=1) == ([0.5, 0.5], 1)
    assert _rows(np.arange(4.0), P=1) == ([0.0, 1.0, 2.0, 3.0] * 2, 4)
    assert _rows([[0.5], [0.25]], P=1) == ([0.5, 0.25], 1)
    gn = np.arange(2 * 5, dtype=float).reshape(G, 5)
    assert _rows(gn, P=1) == (gn.reshape(-1).tolist(), 5)
    # P classes: [G][P] (class scalars), [G][P][n], one [P] / [P][n] for every group
    gp = np.arange(G * P, dtype=float).reshape(G, P) / 8
    assert _rows(gp) == (gp.reshape(-1).tolist(), 1)
    gpn = np.arange(G * P * H, dtype=float).reshape(G, P, H) / 64
    assert _rows(gpn) == (gpn.reshape(-1).tolist(), H)
    assert _rows([0.25, 0.5, 0.75]) == ([0.25, 0.5, 0.75] * G, 1)
    pn = np.arange(P * (H + 1), dtype=float).reshape(P, H + 1)
    assert _rows(pn) == (pn.reshape(-1).tolist() * G, H + 1)
    # a 2-D [G][P] always means class scalars, also where G == P
    sq = np.arange(9.0).reshape(3, 3)
    assert _rows(sq, G=3) == (sq.reshape(-1).tolist(), 1)


def test_price_rows_refusals():
    bad = [(np.zeros((G + 1, 1)), G, 1), (np.zeros((G, 1, 1)), G, 1),                       # wrong leading dims
           (np.zeros((G, P + 1)), G, P), (np.zeros((G + 1, P)), G, P), (np.zeros((G, 2, P, 1)), G, P),
           (np.zeros((G, P, 0)), G, P), ([0.0], G, P),
           ([0.0, 0.0], 1, 1), (np.zeros((G, 2)), G, 1), (np.zeros((G, P, 2)), G, P),        # n = 2 < H
           (np.zeros((P, 2)), G, P),
           (np.zeros(P + 1), G, P), (np.zeros((P - 1, H)), G, P), (np.zeros((G, P)), G, P + 1)]   # P rows, another P
    for rp, g, p in bad:
        with pytest.raises(ValueError):
            L.price_rows(rp, g, p, H, CPU)
    with pytest.raises(ValueError, match="broadcast"):
        L.price_rows([0.0, 0.0], 1, 1, H, CPU)


def test_price_rows_returns_a_device_tensor_without_a_copy():
    for t, g, p in ((torch.zeros(H + 1, dtype=torch.float64), 1, 1), (torch.zeros((G, H), dtype=torch.float64), G, 1),
                    (torch.zeros((G, P), dtype=torch.float64), G, P), (torch.zeros((G, P, H), dtype=torch.float64), G, P)):
        flat, _ = L.price_rows(t, g, p, H, CPU)
        assert flat.data_ptr() == t.data_ptr()
    # what has to be expanded or converted is a copy
    t = torch.zeros(P, dtype=torch.float64)
    assert L.price_rows(t, G, P, H, CPU)[0].data_ptr() != t.data_ptr()
    t = torch.zeros((G, H), dtype=torch.float32)
    assert L.price_rows(t, G, 1, H, CPU)[0].data_ptr() != t.data_ptr()


# ------------------------------------------------------------------ device_arg
def test_device_arg():
    x = torch.zeros(3, dtype=torch.int32)
    assert L.device_arg(x, "x", CPU, torch.int32, (3,)) is x
    assert L.device_arg(x, "x", CPU, torch.int32) is x and L.device_arg(x, "x", CPU, torch.int32, numel=3) is x
    assert L.device_arg(x, "x", CPU, (torch.int64, torch.int32), (3,)) is x         # one of several dtypes
    y = torch.zeros((2, 3), dtype=torch.float64)
    assert L.device_arg(y, "y", CPU, torch.float64, numel=6) is y                    # any shape of 6 entries
    for bad, kw in ((x, dict(dtype=torch.int64, shape=(3,))), (x, dict(dtype=(torch.int64, torch.float64))),
                    (x, dict(dtype=torch.int32, shape=(4,))), (x, dict(dtype=torch.int32, shape=(3, 1))),
                    (x, dict(dtype=torch.int32, numel=4)),
                    (torch.zeros(6, dtype=torch.int32)[::2], dict(dtype=torch.int32, shape=(3,))),     # a strided view
                    (y.t(), dict(dtype=torch.float64, numel=6)),
                    ([0, 0, 0], dict(dtype=torch.int32, shape=(3,))), (None, dict(dtype=torch.int32)),
                    (np.zeros(3, dtype=np.int32), dict(dtype=torch.int32, shape=(3,))),
                    (x, dict(dtype=torch.int32, shape=(3,), device=torch.device("meta")))):
        kw = dict(kw)
        with pytest.raises(ValueError, match="contiguous device tensor"):
            L.device_arg(bad, "arg", kw.pop("device", CPU), **kw)


# ------------------------------------------------------------------ Members and Held on the stand-ins
E, C = 3, 2
STARTS = [0, 7, 12]


def _unit(vehicles=True):
    """A live unit of E episodes: ClassBatch homes with two price classes and, with `vehicles`, a StandInFleet."""
    batch = ClassBatch(HOMES, ENV, ENV, ENV, 0, (0.0,), device=CPU, groups=E)
    batch.set_price_classes(CLASSES, 2)
    batch.tou = torch.arange(8.0)                    # (an environment tensor for `replica` to share)
    m = Members(batch, homes=HOMES, batch_args=(ClassBatch, dict(device=CPU)),
                fleet_args=(StandInFleet, dict(day_offset=DAY0, device=CPU)), classes=(CLASSES, 2))
    if vehicles:
        m.fleet = m.new_fleet(ENV, E)
    return m


def _keys(clocks, copies=1):
    return (torch.tensor(SEEDS, dtype=torch.int64).repeat(copies), torch.tensor(STARTS, dtype=torch.int32).repeat(copies),
            torch.tensor(clocks, dtype=torch.int32).repeat(copies))


def _batch_equal(a, b):
    return all(torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k)))
               for k in ("vals", "fc", "status", "iters", "int_path", "obj"))


def test_held_is_allocated_once_and_filled_bit_for_bit():
    m = _unit()
    held = Held(m)
    names = [k for k in BATCH_ARRAYS if getattr(m.batch, k, None) is not None] + ["fc"]
    assert sorted(names) == ["fc", "int_path", "iters", "obj", "status", "vals"]     # (the stand-in has no fc_store)
    assert (held.batch.N, held.batch.H, held.batch.groups) == (m.batch.N, m.batch.H, E)
    assert (held.fleet.M, held.fleet.H, held.fleet.groups) == (m.fleet.M, m.fleet.H, E)
    ptrs = None
    for t, price in enumerate(([[0.25, 0.5]] * E, [[0.5, -0.25]] * E)):
        m.set_reward_price(torch.tensor(price, dtype=torch.float64))
        m.step_episodes(*_keys([t] * E))
        row = torch.zeros(1)
        assert held.fill(m, row) is held and held.batch.hist_row is row
        for k in names:
            a, b = getattr(held.batch, k), getattr(m.batch, k)
            assert a.data_ptr() != b.data_ptr() and torch.equal(_bits(a), _bits(b)), k
        for k in FLEET_ARRAYS:
            a, b = getattr(held.fleet, k), getattr(m.fleet, k)
            assert a.data_ptr() != b.data_ptr() and torch.equal(_bits(a), _bits(b)), k
        now = [getattr(held.batch, k).data_ptr() for k in names] + [getattr(held.fleet, k).data_ptr() for k in FLEET_ARRAYS]
        assert ptrs is None or now == ptrs
        ptrs = now
    assert held.fill(m).batch.hist_row is None
    assert all(getattr(held.batch, k) is None for k in BATCH_ARRAYS if k not in names)
    # homes only: no fleet half
    plain = _unit(vehicles=False)
    assert Held(plain).fill(plain).fleet is None


def test_replica_shares_the_environment_and_the_class_map():
    m = _unit()
    r = m.replica(C * E, key=C)
    assert m.replica(C * E, key=C) is r and list(m.replicas) == [C] and m.replica(C * E) is not r
    assert r.batch.groups == r.fleet.groups == C * E and r.batch.N == C * m.batch.N and r.fleet.M == C * m.fleet.M
    assert r.batch.tou is m.batch.tou and r.fleet.tou is m.fleet.tou
    assert r.batch.cls == m.batch.cls and r.batch.n_classes == 2
    assert r.fleet.cls == m.fleet.cls == [1, 0, 1] and r.fleet.n_classes == 2
    m.batch.tou = torch.arange(9.0)                  # a new environment reaches the replica with the next sweep
    assert m.replica(C * E, key=C).batch.tou is m.batch.tou
    plain = _unit(vehicles=False)
    assert plain.replica(C * E).fleet is None


def test_members_moves_equal_the_direct_calls():
    """set_reward_price, step_episodes, sums, replicate_from, adopt_from and reset_fleet through the unit against
    the same calls made on a batch and a fleet directly, bit for bit; snapshot / restore on the homes alone (the
    stand-in fleet has neither)."""
    price = torch.tensor([[0.25, 0.5], [0.0, -0.25], [0.5, 0.5]], dtype=torch.float64)

    def stepped(vehicles=True):
        u = _unit(vehicles)
        u.set_reward_price(price)
        u.step_episodes(*_keys([0, 0, 0]))
        return u
    m, d = stepped(), _unit()
    d.batch.set_reward_price(price)
    d.fleet.set_reward_price(price)
    d.batch.step_episodes(*_keys([0, 0, 0]), noise=None, hist=None)
    d.fleet.step_episodes(*_keys([0, 0, 0])[1:])
    assert _batch_equal(m.batch, d.batch) and _fleet_equal(m.fleet, d.fleet)
    want = d.fleet.aggregate_onto(d.batch.aggregate_groups())
    assert torch.equal(_bits(m.sums()), _bits(want)) and torch.equal(_bits(m.fleet.sums), _bits(d.fleet.sums))
    out = torch.zeros((E, 3), dtype=torch.float64)
    assert m.sums(out=out) is out and torch.equal(_bits(out), _bits(want))
    # a sweep of C candidates, episode 1 idle: replicate, step, hold the step, adopt a choice
    cand = torch.tensor([[[0.5, -0.25], [0.0, 0.75]], [[0.25, 0.25], [0.5, 0.0]], [[-0.5, 0.5], [0.25, -0.25]]],
                        dtype=torch.float64).transpose(0, 1).reshape(C * E, 2)          # copy-major [C * E][P]
    r, rd = m.replica(C * E), d.replica(C * E)
    keys = _keys([1, -1, 1], C)
    r.set_reward_price(cand)
    r.replicate_from(m)
    r.step_episodes(*keys)
    rd.batch.set_reward_price(cand)
    rd.fleet.set_reward_price(cand)
    rd.batch.replicate_from(d.batch)
    rd.fleet.replicate_from(d.fleet)
    rd.batch.step_episodes(*keys, noise=None, hist=None)
    rd.fleet.step_episodes(*keys[1:])
    assert _batch_equal(r.batch, rd.batch) and _fleet_equal(r.fleet, rd.fleet)
    assert torch.equal(_bits(r.sums()), _bits(rd.fleet.aggregate_onto(rd.batch.aggregate_groups())))
    held = Held(r).fill(r)
    r.step_episodes(*_keys([2, -1, 2], C))           # the replicas move on: the held step stays
    choice = torch.tensor([1, 0, 0], dtype=torch.int32)
    for unit, src in ((m, held), (stepped(), rd)):       # ... and adopting from the replicas themselves (K = 1)
        unit.adopt_from(src, choice)
        d2 = stepped()
        d2.batch.adopt_from(rd.batch, choice, hist=None)
        d2.fleet.adopt_from(rd.fleet, choice)
        assert _batch_equal(unit.batch, d2.batch) and _fleet_equal(unit.fleet, d2.fleet)
    assert not _fleet_equal(m.fleet, d.fleet)            # (the adoption moved episode 0 and 2 ...)
    assert _fleet_equal(m.fleet, d.fleet, groups=[1])    # (... and left the idle episode alone)
    # reset_fleet clears the masked groups of the fleet alone
    m, mask = stepped(), torch.tensor([False, True, False])
    m.reset_fleet(mask)
    d.fleet.reset_groups(mask)
    assert _fleet_equal(m.fleet, d.fleet) and _batch_equal(m.batch, d.batch) and bool(torch.isnan(m.fleet.vals[:, 3:6]).all())
    # homes only: the same moves without a fleet; restore puts the snapshot back
    plain = stepped(vehicles=False)
    plain.reset_fleet(mask)
    assert _batch_equal(plain.batch, d.batch) and torch.equal(_bits(plain.sums()), _bits(d.batch.aggregate_groups()))
    snap = plain.snapshot()
    assert len(snap) == 2 and snap[0].data_ptr() != plain.batch.vals.data_ptr()
    plain.step_episodes(*_keys([1, 1, 1]))
    assert not _batch_equal(plain.batch, d.batch)
    plain.restore(snap)
    assert all(torch.equal(_bits(getattr(plain.batch, k)), _bits(getattr(d.batch, k))) for k in ("vals", "fc"))
