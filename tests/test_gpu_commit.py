"""Playing a swept candidate on the GPU: dragg_mpc_adopt (replica -> live state, a choice per group read
on the device), dragg_mpc_select_groups (the choice made there) and what is built on them --
`DeviceAggregator.sweep(hold=True)` / `commit`, `VectorAggregator.sweep` / `select` / `commit`,
`Aggregator.rl_commit` and `SweepAgent(commit=True)`.

The reference of every test is existing code: torch indexing for the raw copy, the Python rule for the
choice, and for the committed steps a twin that solves the step the ordinary way (`set_reward_price` +
`run_iteration`, `VectorAggregator.step`, `rl_step`).  Everything is compared BIT FOR BIT (int64 views)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import fixtures as F

pytestmark = pytest.mark.gpu

SENT64 = 0x7FF8_0BAD_0BAD_0001          # (a NaN with a payload: an untouched double must keep it)
SENT32 = -77


def _bits(x):
    return x.contiguous().view(torch.int64)


def _eq(x, y):
    """Equal bit for bit (float64 as int64, so that NaNs compare)."""
    return torch.equal(_bits(x), _bits(y)) if x.dtype == torch.float64 else torch.equal(x, y)


# ------------------------------------------------------------------ 1. raw adopt bits
def _patterns(rng, shape):
    """Random 64-bit patterns as float64, a quarter of them NaNs with random payloads."""
    v = rng.integers(-2 ** 63, 2 ** 63 - 1, size=shape, dtype=np.int64)
    nan = (0x7FF0_0000_0000_0001 | rng.integers(0, 2 ** 51, size=shape, dtype=np.int64)) | \
        np.where(rng.random(shape) < 0.5, np.int64(-2 ** 63), np.int64(0))
    return torch.from_numpy(np.where(rng.random(shape) < 0.25, nan, v)).cuda().view(torch.float64)


def _arrays(rng, N, H, L, fill=None):
    """vals, fc, hist, obj, relax_obj (float64) and status, iters, int_path (int32) of N homes: random
    bits, or `fill`ed with the sentinels."""
    f64 = {"vals": (L.NVAL, N), "fc": (N, L.NFC, H), "hist": (L.NVAL, N), "obj": (N,), "relax_obj": (N,)}
    i32 = ("status", "iters", "int_path")
    if fill:
        out = {k: torch.full(s, SENT64, dtype=torch.int64, device="cuda").view(torch.float64) for k, s in f64.items()}
        out.update({k: torch.full((N,), SENT32, dtype=torch.int32, device="cuda") for k in i32})
    else:
        out = {k: _patterns(rng, s) for k, s in f64.items()}
        out.update({k: torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31 - 1, size=N, dtype=np.int32)).cuda()
                    for k in i32})
    return out


def _structs(L, a, leave_out=()):
    p = lambda k: None if k in leave_out else L.ptr(a[k])  # noqa: E731
    return (L.Hash(vals=L.ptr(a["vals"]), fc=L.ptr(a["fc"])),
            L.Out(status=p("status"), iters=p("iters"), obj=p("obj"), relax_obj=p("relax_obj"), hist=p("hist"),
                  cycles=None, int_path=p("int_path")))


def _expected(src, dst0, choice, Nb, E, C, skip=()):
    """The adopted arrays by torch indexing: group e's columns from copy choice[e], else as they were."""
    Nd = Nb * E
    want = {k: v.clone() for k, v in dst0.items()}
    for e, c in enumerate(choice):
        if not 0 <= c < C:
            continue
        d, s = slice(e * Nb, (e + 1) * Nb), slice(c * Nd + e * Nb, c * Nd + (e + 1) * Nb)
        for k in want:
            if k in skip:
                continue
            if k == "fc":
                want[k][d] = src[k][s]
            else:
                want[k][..., d] = src[k][..., s]
    return want


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int64 if a[k].dtype == torch.float64 else torch.int32),
                           b[k].view(torch.int64 if b[k].dtype == torch.float64 else torch.int32)) for k in a)


@pytest.mark.parametrize("Nb,E,C,H,choices", [
    (3, 3, 3, 5, ([2, -1, 3], [0, 1, 2])),          # everything odd: 8-byte units (4-byte for the int32 rows)
    (4, 2, 2, 6, ([1, -1], [2, 0], [0, 1])),        # 16-byte units everywhere
    (5, 1, 4, 6, ([3], [-1], [4], [0])),            # one group, odd Nd: fc in 16-byte units, the rows in 8
])
def test_adopt_moves_bits(gpu, Nb, E, C, H, choices):
    from dragg_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(100 * Nb + E)
    Nd = Nb * E
    dims = L.Dims(n_homes=Nd, horizon=H, sub_steps=6, dt=1, n_groups=E if E > 1 else 0)
    src = _arrays(rng, C * Nd, H, L)
    src0 = {k: v.clone() for k, v in src.items()}
    stream = L.stream_ptr(None, gpu)
    for choice in choices:
        # once with every member; once with hist NULL in the source and int_path NULL in the destination
        for skip, src_skip, dst_skip in (((), (), ()), (("hist", "int_path"), ("hist",), ("int_path",))):
            dst = _arrays(rng, Nd, H, L, fill=True)
            dst0 = {k: v.clone() for k, v in dst.items()}
            ch = torch.tensor(choice, dtype=torch.int32, device=gpu)
            sh, so = _structs(L, src, src_skip)
            dh, do = _structs(L, dst, dst_skip)
            assert lib.dragg_mpc_adopt(dims, C, L.ptr(ch), sh, so, dh, do, stream) == 0
            torch.cuda.synchronize()
            want = _expected(src0, dst0, choice, Nb, E, C, skip)
            for k in want:
                assert _same({k: dst[k]}, {k: want[k]}), (choice, skip, k)
            assert _same(src, src0), (choice, "the source changed")
            # an untouched group keeps the sentinel in every array
            for e, c in enumerate(choice):
                if not 0 <= c < C:
                    sl = slice(e * Nb, (e + 1) * Nb)
                    assert bool((dst["vals"][:, sl].view(torch.int64) == SENT64).all())
                    assert bool((dst["fc"][sl].view(torch.int64) == SENT64).all())
                    assert bool((dst["status"][sl] == SENT32).all()) and bool((dst["iters"][sl] == SENT32).all())


def test_adopt_arguments(gpu):
    from dragg_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(1)
    Nb, E, C, H = 3, 2, 2, 4
    src, dst = _arrays(rng, C * Nb * E, H, L), _arrays(rng, Nb * E, H, L, fill=True)
    dst0 = {k: v.clone() for k, v in dst.items()}
    ch = torch.tensor([1, 0], dtype=torch.int32, device=gpu)
    sh, so = _structs(L, src)
    dh, do = _structs(L, dst)
    stream = L.stream_ptr(None, gpu)
    dims = lambda **kw: L.Dims(**{**dict(n_homes=Nb * E, horizon=H, sub_steps=6, dt=1, n_groups=E), **kw})  # noqa: E731
    E_ARG = -1
    # n_homes == 0: a no-op
    assert lib.dragg_mpc_adopt(dims(n_homes=0), C, L.ptr(ch), sh, so, dh, do, stream) == 0
    assert lib.dragg_mpc_adopt(dims(), 0, L.ptr(ch), sh, so, dh, do, stream) == E_ARG             # copies < 1
    assert lib.dragg_mpc_adopt(dims(n_homes=Nb * E - 1), C, L.ptr(ch), sh, so, dh, do, stream) == E_ARG   # N % E
    assert lib.dragg_mpc_adopt(dims(), C, None, sh, so, dh, do, stream) == E_ARG                  # NULL choice
    assert lib.dragg_mpc_adopt(dims(), C, L.ptr(ch), None, so, dh, do, stream) == E_ARG
    assert lib.dragg_mpc_adopt(dims(), C, L.ptr(ch), sh, so, None, do, stream) == E_ARG
    assert lib.dragg_mpc_adopt(dims(), C, L.ptr(ch), L.Hash(vals=None, fc=L.ptr(src["fc"])), so, dh, do, stream) == E_ARG
    assert lib.dragg_mpc_adopt(dims(), C, L.ptr(ch), sh, so, L.Hash(vals=L.ptr(dst["vals"]), fc=None), do, stream) == E_ARG
    torch.cuda.synchronize()
    assert _same(dst, dst0)                               # none of them wrote anything
    # the hash arrays alone (both out structs NULL)
    assert lib.dragg_mpc_adopt(dims(), C, L.ptr(ch), sh, None, dh, None, stream) == 0
    torch.cuda.synchronize()
    want = _expected(src, dst0, [1, 0], Nb, E, C, skip=("hist", "obj", "relax_obj", "status", "iters", "int_path"))
    assert _same(dst, want)


# raw pointers at chosen byte offsets (tests/arena.py): every unit width, the one-block-per-group loop, the refusal
ADOPT_F64, ADOPT_I32 = ("vals", "fc", "hist", "obj", "relax_obj"), ("status", "iters", "int_path")


def _adopt_arena(L, Nb, E, C, H, offs):
    from tests.arena import Arena
    ar = Arena()
    for side, n, (f8, i4) in (("src_", C * Nb * E, offs[0::2]), ("dst_", Nb * E, offs[1::2])):
        for k in ADOPT_F64:
            ar.add(side + k, np.float64, {"vals": (L.NVAL, n), "hist": (L.NVAL, n), "fc": (n, L.NFC, H)}.get(k, (n,)), f8)
        for k in ADOPT_I32:
            ar.add(side + k, np.int32, (n,), i4)
    return ar


def _adopt_rule(ar, src_buf, dst_buf, choice, Nb, E, C):
    """The index rule on the host bytes: group e's Nb columns of every row (fc: its Nb homes' blocks) from columns
    [c * Nd + e * Nb, ...) of the source, c = choice[e] in [0, C); any other group: nothing."""
    Nd = Nb * E
    for e, c in enumerate(choice):
        if not 0 <= c < C:
            continue
        d, s = slice(e * Nb, (e + 1) * Nb), slice(c * Nd + e * Nb, c * Nd + (e + 1) * Nb)
        for k in ADOPT_F64 + ADOPT_I32:
            src, dst = ar.view(src_buf, "src_" + k), ar.view(dst_buf, "dst_" + k)
            if k == "fc":
                dst[d] = src[s]
            else:
                dst[..., d] = src[..., s]


def _adopt_raw(L, lib, ar, dev, Nb, E, C, H, choice, gpu):
    ch = torch.tensor(choice, dtype=torch.int32, device=gpu)
    p = lambda k: ar.ptr(dev, k)  # noqa: E731
    structs = []
    for side in ("src_", "dst_"):
        structs += [L.Hash(vals=p(side + "vals"), fc=p(side + "fc")),
                    L.Out(status=p(side + "status"), iters=p(side + "iters"), obj=p(side + "obj"),
                          relax_obj=p(side + "relax_obj"), hist=p(side + "hist"), cycles=None,
                          int_path=p(side + "int_path"))]
    dims = L.Dims(n_homes=Nb * E, horizon=H, sub_steps=6, dt=1, n_groups=E if E > 1 else 0)
    rc = lib.dragg_mpc_adopt(dims, C, L.ptr(ch), structs[0], structs[1], structs[2], structs[3], L.stream_ptr(None, gpu))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("Nb", [1, 3, 4])
@pytest.mark.parametrize("E", [1, 3])
def test_adopt_every_unit_width(gpu, Nb, E):
    """Bases 0 / 8 (doubles) and 0 / 4 / 8 / 12 (int32) bytes past a 16-byte boundary: by the unit rule the
    double rows move in 16-byte units at Nb = 4 with both bases aligned and in 8-byte units otherwise, the int32
    rows in 16-, 8- and 4-byte units (Nb = 4 at offsets 0 / 8 / 4 and 12; Nb odd: 4), fc in 16-byte units at
    Nb = 4 and in 8-byte units otherwise.  Every byte of the allocation is compared, the idle groups', the
    source's and the guards' included."""
    from dragg_amd import _lib as L
    from tests.arena import OFFSETS, same_bytes
    lib, C, H = L.load(), 2, 3
    rng = np.random.default_rng(10 * Nb + E)
    for offs in OFFSETS:
        ar = _adopt_arena(L, Nb, E, C, H, offs)
        for choice in (([1, -1, 0], [2, 0, 1]) if E == 3 else ([1], [-1])):
            h0 = ar.random(rng)
            want = h0.copy()
            _adopt_rule(ar, h0, want, choice, Nb, E, C)
            dev = ar.upload(h0, gpu)
            assert _adopt_raw(L, lib, ar, dev, Nb, E, C, H, choice, gpu) == 0
            assert same_bytes(dev.cpu().numpy(), want, ar), (offs, choice)
            for e, c in enumerate(choice):                       # (the restatement left the idle groups alone)
                if not 0 <= c < C:
                    assert np.array_equal(ar.view(want, "dst_vals")[:, e * Nb:(e + 1) * Nb].view(np.int64),
                                          ar.view(h0, "dst_vals")[:, e * Nb:(e + 1) * Nb].view(np.int64))


def test_adopt_one_block_per_group(gpu):
    """E = 5,000 groups of 3 homes, H = 24, about half of them idle: the grid is one block per group, and a
    block walks its group's ~1,200 units (8-byte units: the doubles lie 8 bytes past a 16-byte boundary) over
    all eight segments in its stride loop."""
    from dragg_amd import _lib as L
    from tests.arena import same_bytes
    lib, Nb, E, C, H = L.load(), 3, 5000, 2, 24
    rng = np.random.default_rng(7)
    choice = rng.integers(-1, C + 1, E).tolist()                 # (-1 and C: idle)
    assert 0.4 * E < sum(0 <= c < C for c in choice) < 0.6 * E
    ar = _adopt_arena(L, Nb, E, C, H, (8, 8, 0, 0))
    h0 = ar.random(rng)
    want = h0.copy()
    _adopt_rule(ar, h0, want, choice, Nb, E, C)
    dev = ar.upload(h0, gpu)
    assert _adopt_raw(L, lib, ar, dev, Nb, E, C, H, choice, gpu) == 0
    assert same_bytes(dev.cpu().numpy(), want, ar)


def test_adopt_refuses_a_misaligned_double_array(gpu):
    """A double array 4 bytes past an 8-byte boundary: DRAGG_E_ARG, and no byte is written."""
    from dragg_amd import _lib as L
    lib, Nb, E, C, H = L.load(), 3, 2, 2, 3
    rng = np.random.default_rng(3)
    for offs in ((4, 0, 0, 0), (0, 4, 0, 0), (12, 12, 0, 0)):
        ar = _adopt_arena(L, Nb, E, C, H, offs)
        h0 = ar.random(rng)
        dev = ar.upload(h0, gpu)
        assert _adopt_raw(L, lib, ar, dev, Nb, E, C, H, [1, 0], gpu) == -1, offs
        assert np.array_equal(dev.cpu().numpy(), h0), offs


def test_adopt_from_checks_its_arguments(gpu):
    from dragg_amd.community import synthetic_homes, synthetic_weather
    from dragg_amd.mpc import MPCBatch
    homes = synthetic_homes(8, seed=5, days=2, dt=4, horizon_hours=6)[:3]
    oat, ghi, tou = synthetic_weather(2, 4, 24, seed=5, month=7)
    live = MPCBatch(homes, oat, ghi, tou)
    src = MPCBatch(homes, oat, ghi, tou, groups=2)
    ok = torch.zeros(1, dtype=torch.int32, device=gpu)
    live.adopt_from(src, ok)
    for bad in (torch.zeros(1, dtype=torch.int64, device=gpu), torch.zeros(2, dtype=torch.int32, device=gpu),
                torch.zeros(1, dtype=torch.int32), [0]):
        with pytest.raises(ValueError):
            live.adopt_from(src, bad)
    with pytest.raises(ValueError):
        live.adopt_from(MPCBatch(homes[:2], oat, ghi, tou, groups=2), ok)       # not whole copies


# ------------------------------------------------------------------ 2. select
def test_select_groups_rule(gpu):
    from dragg_amd import _lib as L
    lib = L.load()
    nan = float("nan")
    E, C, n_rp = 4, 3, 2
    # [C][E]: loads, prices (first entry), per group e
    loads = [[8.0, 5.0, nan, nan],
             [20.0, 7.0, 9.0, nan],
             [12.0, 7.0, 11.0, nan]]
    price = [[0.5, 0.0, 0.0, 0.0],
             [0.0, 0.125, -0.25, 0.0],
             [-0.25, -0.125, -0.25, 0.0]]
    target = [10.0, 7.0, 10.0, 1.0]
    # group 0: |8 - 10| == |12 - 10|, broken by |price| (0.5 against 0.25) -> 2;  group 1: copies 1 and 2 tie on
    # the load and on |price| -> the smaller index, 1;  group 2: copy 0 has no load, 1 and 2 tie twice -> 1;
    # group 3: no copy has a load -> -1
    sums = torch.tensor([[loads[c][e], 1e9, -1e9] for c in range(C) for e in range(E)], dtype=torch.float64, device=gpu)
    prices = torch.tensor([[price[c][e], 99.0] for c in range(C) for e in range(E)], dtype=torch.float64, device=gpu)
    tgt = torch.tensor(target, dtype=torch.float64, device=gpu)
    choice = torch.full((E,), 7, dtype=torch.int32, device=gpu)
    dims = L.Dims(n_homes=2 * E, horizon=4, sub_steps=6, dt=1, n_groups=E)
    assert lib.dragg_mpc_select_groups(dims, C, L.ptr(sums), L.ptr(tgt), L.ptr(prices), n_rp, L.ptr(choice),
                                       L.stream_ptr(None, gpu)) == 0
    want = []
    for e in range(E):
        valid = [c for c in range(C) if not np.isnan(loads[c][e])]
        want.append(min(valid, key=lambda c: (abs(loads[c][e] - target[e]), abs(price[c][e]), c)) if valid else -1)
    assert want == [2, 1, 1, -1]
    assert choice.tolist() == want
    assert lib.dragg_mpc_select_groups(dims, 0, L.ptr(sums), L.ptr(tgt), L.ptr(prices), n_rp, L.ptr(choice), None) == -1
    assert lib.dragg_mpc_select_groups(dims, C, None, L.ptr(tgt), L.ptr(prices), n_rp, L.ptr(choice), None) == -1


# ------------------------------------------------------------------ 3. DeviceAggregator
@pytest.fixture(scope="module")
def community():
    from dragg_amd.community import synthetic_homes, synthetic_weather
    homes = synthetic_homes(64, seed=5, days=2, dt=4, horizon_hours=6)
    assert {h["type"] for h in homes} == {"base", "pv_only", "battery_only", "pv_battery"}
    return homes, synthetic_weather(2, 4, 24, seed=5, month=7)


def _agg(community, n=64, steps=2, **kw):
    """The community after `steps` committed steps under a zero reward price."""
    from dragg_amd.aggregator import DeviceAggregator
    homes, (oat, ghi, tou) = community
    agg = DeviceAggregator(homes[:n], oat, ghi, tou, 0, 8, reward_price=[0.0] * 24, seed=5, **kw)
    for _ in range(steps):
        agg.run_iteration()
        agg.collect_data()
    return agg


def _candidates():
    """A scalar price, a negative one, and a list that changes at every stage (so the later launches run)."""
    return np.stack([np.full(24, 0.05), np.full(24, -0.03), -0.03 * np.cos(np.arange(24))])


def _assert_same_step(a, b, t, sums_a, sums_b, what):
    a.drain()
    b.drain()
    assert a.timestep == b.timestep == t + 1, what
    for name, x, y in (("hist", a.hist[t], b.hist[t]), ("vals", a.batch.vals, b.batch.vals),
                       ("fc", a.batch.fc_store, b.batch.fc_store), ("sums", sums_a, sums_b),
                       ("agg_hist", a.agg_hist[t], b.agg_hist[t]), ("reward price", a.batch.rp, b.batch.rp),
                       ("obj", a.batch.obj, b.batch.obj), ("relax_obj", a.batch.relax_obj, b.batch.relax_obj)):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y)), (what, name)
    for name, x, y in (("status_hist", a.status_hist[t], b.status_hist[t]), ("path_hist", a.path_hist[t], b.path_hist[t]),
                       ("status", a.batch.status, b.batch.status), ("iters", a.batch.iters, b.batch.iters),
                       ("int_path", a.batch.int_path, b.batch.int_path)):
        assert torch.equal(x, y), (what, name)
    assert a.batch.dims.n_rp == b.batch.dims.n_rp, what


@pytest.mark.parametrize("int_mode,steps", [("round", 1), ("round", 2), ("relax", 1)])
def test_commit_equals_the_solved_step(gpu, community, int_mode, steps):
    P = _candidates()
    agg, twin = _agg(community, int_mode=int_mode), _agg(community, int_mode=int_mode)
    t = agg.timestep
    assert t == 2
    plain = agg.sweep(P, steps).clone()
    sw = agg.sweep(P, steps, hold=True)
    assert tuple(sw.shape) == (3, steps, 3) and torch.equal(_bits(sw), _bits(plain))
    assert agg.holds() and agg.holds(2) and not agg.holds(3)
    agg.commit(2)
    sums = agg.collect_data().clone()
    assert not agg.holds()
    twin.set_reward_price(P[2])
    twin.run_iteration()
    twin_sums = twin.collect_data().clone()
    _assert_same_step(agg, twin, t, sums, twin_sums, "the committed step")
    assert torch.equal(_bits(sums), _bits(sw[2, 0]))
    assert not torch.isnan(agg.hist[t]).all() and int((agg.status_hist[t] == 0).sum()) > 0
    assert agg.approx_counts() == twin.approx_counts()
    # one more ordinary step on both
    agg.run_iteration()
    twin.run_iteration()
    _assert_same_step(agg, twin, t + 1, agg.collect_data().clone(), twin.collect_data().clone(), "the step after")


def test_commit_refusals(gpu, community):
    P = _candidates()
    agg = _agg(community, n=16)
    with pytest.raises(ValueError):
        agg.commit(0)                                   # nothing held
    agg.sweep(P, 1)
    with pytest.raises(ValueError):
        agg.commit(0)                                   # a sweep without hold holds nothing
    agg.sweep(P, 1, hold=True)
    with pytest.raises(ValueError):
        agg.commit(3)                                   # g = G
    with pytest.raises(ValueError):
        agg.commit(-1)
    agg.run_iteration()
    agg.collect_data()
    with pytest.raises(ValueError):
        agg.commit(0)                                   # the live state has moved
    agg.sweep(P, 1, hold=True)
    snap = agg.snapshot()
    agg.restore(snap)
    with pytest.raises(ValueError):
        agg.commit(0)
    agg.sweep(P, 1, hold=True)
    agg.commit(1)
    with pytest.raises(ValueError):
        agg.commit(1)                                   # the hold is spent
    lag = _agg(community, n=16, steps=0, overlap=True)
    assert lag.overlap
    with pytest.raises(ValueError):
        lag.commit(0)


# ------------------------------------------------------------------ 4. VectorAggregator
def test_vector_sweep_select_commit(gpu, community):
    from dragg_amd.vector import VectorAggregator
    homes, (oat, ghi, tou) = community
    homes = homes[::4][:15]                              # Nb odd, all four types
    assert len({h["type"] for h in homes}) == 4
    E, C, T = 3, 2, 4
    mk = lambda: VectorAggregator(homes, oat, ghi, tou, E, [5, 6, 7], [0, 7, 12], T)  # noqa: E731
    va, twin = mk(), mk()
    rp = -0.03 * np.cos(np.arange(24))
    first = np.stack([np.zeros(24), rp, rp + 0.2])
    for v in (va, twin):                                # episode 0 stays at t = 0, 1 and 2 take two steps
        v.park([0])
        v.step(first)
        v.step(first)
        v.resume([0])
        v.park([2])                                     # ... and episode 2 sits the sweep out
    assert va.clocks_host() == [0, 2, 2]
    cands = np.stack([np.stack([np.full(24, 0.05), rp]), np.stack([rp + 0.1, np.full(24, -0.02)]),
                      np.stack([rp, rp])])              # [E][C][24]
    b = va.batch
    keep = {k: getattr(b, k).clone() for k in ("vals", "fc_store", "status", "iters", "obj", "relax_obj", "int_path")}
    hists = (va.hist.clone(), va.status_hist.clone(), va.path_hist.clone(), va.agg_hist.clone())
    sums = va.sweep(cands)
    assert tuple(sums.shape) == (E, C, 3)
    # the sweep only reads the live batch
    assert all(_eq(getattr(b, k), v) for k, v in keep.items())
    setpoints = [0.0, 1e9, 5.0]                          # episode 0: the smaller load, episode 1: the larger
    choice = va.select(sums, setpoints, cands)
    s = sums.cpu().numpy()
    want = [min(range(C), key=lambda c: (abs(s[e, c, 0] - setpoints[e]), abs(cands[e, c, 0]), c)) for e in range(E)]
    assert choice.dtype == torch.int32 and choice.tolist() == want
    assert s[0, 0, 0] != s[0, 1, 0] and s[1, 0, 0] != s[1, 1, 0]       # the candidates differ: a choice was made
    got = va.commit(choice).clone()
    assert va.adopted.tolist() == [True, True, False]
    ref = twin.step(np.stack([cands[e, want[e]] for e in range(E)])).clone()
    assert va.clocks_host() == twin.clocks_host() == [1, 3, 2]
    tb = twin.batch
    for k in keep:
        assert _eq(getattr(b, k), getattr(tb, k)), k
    for name, x, y in (("hist", va.hist, twin.hist), ("agg_hist", va.agg_hist, twin.agg_hist), ("sums", got, ref)):
        assert torch.equal(_bits(x), _bits(y)), name
    assert torch.equal(va.status_hist, twin.status_hist) and torch.equal(va.path_hist, twin.path_hist)
    for e in range(2):                                   # the swept sums were the committed step's
        assert torch.equal(_bits(sums[e, want[e]]), _bits(got[e])), e
    # the parked episode: unchanged in every array
    sl = slice(2 * va.Nb, 3 * va.Nb)
    for k, v in keep.items():
        x = getattr(b, k)
        assert _eq(x[sl], v[sl]) if k == "fc_store" else _eq(x[..., sl], v[..., sl]), k
    for x, v in zip((va.hist, va.status_hist, va.path_hist), hists[:3]):
        assert _eq(x[..., sl], v[..., sl])
    assert torch.equal(_bits(va.agg_hist[:, 2]), _bits(hists[3][:, 2]))
    # a hold is spent by its commit, and voided by a step
    with pytest.raises(ValueError):
        va.commit(choice)
    va.sweep(cands)
    va.step(first)
    with pytest.raises(ValueError):
        va.commit(choice)


# ------------------------------------------------------------------ 5. the runner
def _synthetic_data(root, days=3, n_profiles=4, seed=0):
    """NSRDB-format weather and minute-resolution water-draw profiles (synthetic)."""
    from dragg_amd.community import half_hourly_weather
    oat, ghi = half_hourly_weather(days, seed=seed)
    rows = []
    for k in range(days * 48):
        day, hh = divmod(k, 48)
        rows.append(f"2015,1,{day + 1},{hh // 2},{30 * (hh % 2)},{ghi[k]},90.0,{oat[k]},1020.0")
    with open(os.path.join(root, "nsrdb.csv"), "w") as f:
        f.write("Source,Location ID\nNSRDB,0\nYear,Month,Day,Hour,Minute,GHI,Relative Humidity,Temperature,Pressure\n")
        f.write("\n".join(rows) + "\n")
    rng = np.random.default_rng(seed)
    mins = 2 * 24 * 60
    flow = np.where(rng.random((mins, n_profiles)) < 0.03, 3.78 * rng.integers(1, 4, (mins, n_profiles)), 0.0)
    ts = np.datetime64("2020-01-01T00:00") + np.arange(mins).astype("timedelta64[m]")
    with open(os.path.join(root, "waterdraw_profiles.csv"), "w") as f:
        f.write("," + ",".join(f"Flow_{j}" for j in range(n_profiles)) + "\n")
        for i in range(mins):
            f.write(str(ts[i]).replace("T", " ") + ":00," + ",".join(f"{v:.2f}" for v in flow[i]) + "\n")


RL_EXTRA = """
[rl.utility]
action_space = [-5, 5]
action_scale = 100

[rl.parameters]
policy = "sweep"
candidates = 4
commit = {commit}
"""


def test_run_rl_agg_commit_writes_the_same_results(gpu, tmp_path, monkeypatch):
    """6 steps, 4 candidates: the run that commits the swept candidate and the run that solves it again
    write byte-identical results.json (the Summary's solve_time pinned: the clock is frozen for both)."""
    import datetime as dt_mod
    from dragg_amd import runner
    from dragg_amd.rl import agent_policy

    class Frozen(dt_mod.datetime):
        @classmethod
        def now(cls, tz=None):
            return cls(2015, 1, 1)
    monkeypatch.setattr(runner, "datetime", Frozen)
    params = dict(n=12, batt=3, pv=3, pvb=2, start="2015-01-01 00", end="2015-01-01 03", dt=2, horizon=6,
                  action_horizon=6, seed=21)
    out, counts, commits = {}, {}, {}
    for commit in ("true", "false"):
        data = tmp_path / f"data_{commit}"
        data.mkdir()
        _synthetic_data(str(data))
        with open(data / "config.toml", "w") as f:
            f.write(F.config_text(params) + RL_EXTRA.format(commit=commit))
        a = runner.Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / f"outputs_{commit}"))
        assert a.num_timesteps == 6
        a.checkpoint_interval, a.run_dir = 10 ** 9, str(tmp_path / f"run_{commit}")
        n = {"commit": 0, "step": 0}
        rl_commit, rl_step = a.rl_commit, a.rl_step
        a.rl_commit = lambda g, f=rl_commit, n=n: (n.__setitem__("commit", n["commit"] + 1), f(g))[1]
        a.rl_step = lambda p, f=rl_step, n=n: (n.__setitem__("step", n["step"] + 1), f(p))[1]
        with open(a.run_rl_agg(agent_policy(a)), "rb") as f:
            out[commit] = f.read()
        counts[commit], commits[commit] = a.dev.approx_counts(), n
    assert commits["true"] == {"commit": 6, "step": 0} and commits["false"] == {"commit": 0, "step": 6}
    assert out["true"] == out["false"]
    assert counts["true"] == counts["false"]
    assert len(json.loads(out["true"])["Summary"]["RP"]) == 6
