"""Price classes on the GPU (dragg_mpc_step_classes, dragg_mpc_plan_classes and the layers above them): a reward
price per class of homes in one community.

The oracle is existing code.  Homes do not interact within a step and the season noise is keyed by the global
home index, so the columns of episode e's class-c homes must equal, BIT FOR BIT and at every step, the same
columns of a plain single `DeviceAggregator` run with e's seed and start under class c's price trajectory alone
(the int64 views of vals, fc and the history row, plus status and int_path), and the episode's sums must equal the
existing `aggregate` of the vals assembled from those columns.

Community: tests/test_gpu_vector.py's (16 homes of all four types, H = 24, April, E = 3, T = 4).  Trajectories:
tests/test_gpu_sweep.py's three (flat, RL-priced, RL-priced and shifted) and a fourth that starts below -TOU and
rises to +0.1 (mixed-sign total prices: a home is paid to draw power now).  Episode 0 plays class scalars, two of
them below -TOU, episodes 1 and 2 class lists (rotated, so that every class carries an RL-priced list somewhere
and the deferred, cell and mid launches read class rows).  Why negative prices: at night in April a base or
PV-only home under any positive price draws nothing in its first stages, its vals are then the same under every
positive trajectory, and a lookup that ignored the class would pass for that class; a home that is paid to draw
power does draw, and cost_opt = p_grid * price tells the trajectories apart.  The single runs are computed once
and shared."""
import ctypes
import types

import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from tests.test_gpu_env import _cfg, _same_obs, _same_state
from tests.test_gpu_sweep import _prices
from tests.test_gpu_vector import SEEDS, STARTS, T, _bits, _check_episode, _single, _singles3, community  # noqa: F401

pytestmark = pytest.mark.gpu

E, P, H = 3, 4, 24
SCALARS = (-0.12, -0.1, 0.05, 0.12)               # episode 0's class scalars (TOU is 0.07 off peak)
KEYS, ROWS = ("p_grid", "p_load"), ("p_grid", "cost", "p_pv")
MOD3 = [i % 3 for i in range(16)]                 # classes interleave within a group; class 3 is empty


def _traj():
    return np.concatenate([_prices(), [0.1 - 0.25 * np.exp(-np.arange(24) / 4.0)]])


def _class_price(e, c):
    """Episode e's price list of class c, 24 entries."""
    return np.full(24, SCALARS[c]) if e == 0 else _traj()[(c + 2 * e + 1) % 4]


def _class_prices():
    return torch.as_tensor(np.array([[_class_price(e, c) for c in range(P)] for e in range(E)]))     # [E][P][24]


def _vector(community, price_classes, n_classes=None, steps=T):
    from dragg_amd.vector import VectorAggregator
    homes, (oat, ghi, tou) = community
    return VectorAggregator(homes, oat, ghi, tou, E, list(SEEDS), list(STARTS), steps, price_classes=price_classes,
                            n_classes=n_classes)


def _refs(community):
    """refs[e][c]: the single run with e's seed and start under class c's trajectory alone."""
    homes, weather = community
    return [[_single(homes, weather, SEEDS[e], STARTS[e], _class_price(e, c), T) for c in range(P)] for e in range(E)]


def _masked_plans(b, cm, keys, rows):
    """dragg_mpc_plan_groups (existing code) on NaN-masked copies of the batch's hash arrays, one copy per class
    -> curve, count, stats stacked on a class axis: [G][P][...]."""
    out = []
    for c in range(P):
        other = torch.as_tensor(np.tile(np.asarray(cm) != c, b.groups), device=b.device)
        vals, fc = b.vals.clone(), b.fc_store.clone()
        vals[:, other] = float("nan")
        fc[other] = float("nan")
        src = types.SimpleNamespace(vals=vals, fc_store=fc, N=b.N, groups=b.groups, H=b.H)
        out.append(tuple(x.clone() for x in b.plan_groups(keys, rows, src=src)))
    return tuple(torch.stack([o[k] for o in out], dim=1) for k in range(3))


def _run(community, price_classes, n_classes=None):
    """T class steps; per step clones of what the oracle compares, and after the second step the class plans and
    the masked plan_groups rows."""
    va = _vector(community, price_classes, n_classes)
    prices = _class_prices().to(va.device)
    out = {"va": va, "steps": []}
    for t in range(T):
        sums = va.step(prices)
        b = va.batch
        out["steps"].append({"vals": b.vals.clone(), "fc": b.fc_store.clone(), "status": b.status.clone(),
                             "path": b.int_path.clone(), "sums": sums.clone()})
        if t == 1:
            out["plan"] = tuple(x.clone() for x in va.plan(KEYS, ROWS, classes=True))
            out["masked"] = _masked_plans(b, va.price_class_host, KEYS, ROWS)
            out["whole"] = tuple(x.clone() for x in va.plan(KEYS, ROWS))
    out["hist"] = [va.episode_history(e).clone() for e in range(E)]
    return out


@pytest.fixture(scope="module")
def type_run(gpu, community):
    return _run(community, "type")


@pytest.fixture(scope="module")
def mod3_run(gpu, community):
    return _run(community, MOD3, 4)


@pytest.fixture(scope="module")
def plain_batch(gpu, community):
    """A plain batch of the 16 homes, for the existing `aggregate` on assembled vals."""
    from dragg_amd.mpc import MPCBatch
    homes, (oat, ghi, tou) = community
    return MPCBatch(homes, oat, ghi, tou, 0, [0.0])


def _precondition(refs, cm, classes):
    """For every class some home of it has vals bits that differ between the single run under its own trajectory
    and under another class's (in some episode, at some step): a lookup that ignored the class would not pass."""
    cm = np.asarray(cm)
    for c in classes:
        cols = torch.as_tensor(np.flatnonzero(cm == c))
        assert len(cols), c
        differs = [any(not torch.equal(refs[e][c]["vals"][t][:, cols], refs[e][o]["vals"][t][:, cols])
                       for o in range(P) if o != c for t in range(T)) for e in range(E)]
        print(f"class {c}: its homes' vals differ from another class's trajectory in episodes {differs}")
        assert any(differs), c


def _check_oracle(run, refs, cm, plain_batch):
    cm = np.asarray(cm)
    va, Nb = run["va"], run["va"].Nb
    for t in range(T):
        s = run["steps"][t]
        for e in range(E):
            assembled = torch.zeros((L.NVAL, Nb), dtype=torch.int64, device=va.device)
            for c in range(P):
                cols = torch.as_tensor(np.flatnonzero(cm == c), device=va.device)
                if not len(cols):
                    continue
                ref, at = refs[e][c], e * Nb + cols
                assert torch.equal(_bits(s["vals"][:, at]), ref["vals"][t][:, cols]), (t, e, c, "vals")
                assert torch.equal(_bits(s["fc"][at]), ref["fc"][t][cols]), (t, e, c, "fc")
                assert torch.equal(s["status"][at], ref["status"][t][cols]), (t, e, c, "status")
                assert torch.equal(s["path"][at], ref["path"][t][cols]), (t, e, c, "int_path")
                assert torch.equal(_bits(run["hist"][e][t][:, cols]), ref["hist"][t][:, cols]), (t, e, c, "hist")
                assembled[:, cols] = ref["vals"][t][:, cols]
            plain_batch.vals.copy_(assembled.view(torch.float64))
            want = plain_batch.aggregate().clone()
            assert torch.equal(_bits(s["sums"][e]), _bits(want)), (t, e, "sums")


# ------------------------------------------------------------------ 1, 2: the oracle
def test_type_classes_equal_single_runs_under_each_class_price(gpu, community, type_run, plain_batch):
    refs = _refs(community)
    va = type_run["va"]
    assert va.n_classes == 4 and va.class_names == ["base", "pv_only", "battery_only", "pv_battery"]
    cm = va.price_class_host
    assert cm.tolist() == va.batch.types_host[:16].tolist() and set(cm.tolist()) == {0, 1, 2, 3}
    _precondition(refs, cm, range(P))
    _check_oracle(type_run, refs, cm, plain_batch)
    # the class rows reached every launch: some home under an RL-priced list left the hot launch
    later = sum(int((s["path"] & L.PATH_SECOND != 0).sum()) for s in type_run["steps"])
    print("home-steps finished by a later launch:", later)
    assert later > 0


def test_interleaved_classes_with_an_empty_class(gpu, community, mod3_run, plain_batch):
    refs = _refs(community)
    assert mod3_run["va"].n_classes == 4 and mod3_run["va"].price_class_host.tolist() == MOD3
    _precondition(refs, MOD3, range(3))
    _check_oracle(mod3_run, refs, MOD3, plain_batch)


# ------------------------------------------------------------------ 3: no classes is today's path
def test_one_class_and_no_classes_are_todays_results(gpu, community):
    refs = _singles3(community)
    prices = torch.as_tensor(_prices(), dtype=torch.float64)
    for pc, n in ((None, None), ([0] * 16, 1)):
        va = _vector(community, pc, n)
        assert va.n_classes == 1 and va.batch.n_classes == 1 and va.batch.price_class is None
        for t in range(T):
            sums = va.step(prices)
            for e in range(E):
                _check_episode(va, e, refs[e], t, sums, what=str(pc))
    # the entry point itself with classes NULL and with P = 1: dragg_mpc_step_episodes
    for cls in (None, L.Classes(n_classes=1, price_class=None)):
        va = _vector(community, None)
        b = va.batch
        b.set_reward_price(prices.to(b.device))
        ep, keep = b._episodes(va.seeds, va.starts, va.clocks)
        b._call(b.lib.dragg_mpc_step_classes, b._problem(), ep, cls, b._hash(), b._out(None), 0, None)
        for e in range(E):
            _check_episode(va, e, refs[e], 0, what="entry")


# ------------------------------------------------------------------ 4: plan_classes
def _same_plans(got, want, what):
    for g, w, k in zip(got, want, ("curve", "count", "stats")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert torch.equal(_bits(g) if g.dtype == torch.float64 else g,
                           _bits(w) if w.dtype == torch.float64 else w), (what, k)


def test_plan_classes_equals_plan_groups_on_masked_copies(gpu, community, type_run, mod3_run):
    from dragg_amd.vector import plan_classes_reference
    for name, run in (("type", type_run), ("mod3", mod3_run)):
        curve, count, stats = run["plan"]
        assert tuple(curve.shape) == (E, P, 2, H) and tuple(count.shape) == (E, P, 2, H) and count.dtype == torch.int32
        assert tuple(stats.shape) == (E, P, 3, 4)
        _same_plans(run["plan"], run["masked"], name)
        assert int(count.sum()) > 0 and bool((count[:, :3, :, 0] > 0).all())
        # the classes partition each episode's homes: the counts add up to plan_groups'
        assert torch.equal(count.sum(1), run["whole"][1]) and torch.equal(stats[..., 0].sum(1), run["whole"][2][..., 0])
    # PV rows and class masks overlap: the battery_only class has no PV value, the PV classes do (once solved)
    stats = type_run["plan"][2]
    assert float(stats[:, 2, 2, 0].abs().sum()) == 0.0 and float(stats[:, [1, 3], 2, 0].sum()) > 0
    # the empty class: sum +0.0, count 0, min +inf, max -inf
    curve, count, stats = (x.cpu() for x in mod3_run["plan"])
    assert not count[:, 3].any() and torch.equal(_bits(curve[:, 3]), torch.zeros_like(_bits(curve[:, 3])))
    empty = torch.tensor([0.0, 0.0, float("inf"), -float("inf")], dtype=torch.float64)
    assert torch.equal(_bits(stats[:, 3]), _bits(empty.expand(E, 3, 4)))
    # the numpy restatement agrees on the live state (after the last step)
    va = mod3_run["va"]
    got = va.plan(KEYS, ROWS, classes=True)
    ref = plan_classes_reference(va.batch.vals.cpu().numpy(), va.batch.fc_store.cpu().numpy(), E, MOD3, P, KEYS, ROWS)
    _same_plans([g.cpu() for g in got], [torch.as_tensor(r) for r in ref], "reference")
    # classes NULL and P = 1 give plan_groups' output
    b = va.batch
    whole = b.plan_groups(KEYS, ROWS)
    for cls in (None, L.Classes(n_classes=1, price_class=None)):
        out = tuple(torch.full_like(x, 7) for x in whole)
        plan = L.Plan(fc_keys=L.plan_select(KEYS, ROWS)[0], val_rows=L.plan_select(KEYS, ROWS)[1],
                      curve=L.ptr(out[0]), count=L.ptr(out[1]), stats=L.ptr(out[2]))
        L.check(b.lib.dragg_mpc_plan_classes(b.dims, b._hash(), cls, plan, L.stream_ptr(None, b.device)))
        _same_plans(out, whole, "no classes")
    # a class value outside 0 .. P - 1 cannot be set from Python
    with pytest.raises(ValueError):
        b.set_price_classes([4] + [0] * 15, 4)


# ------------------------------------------------------------------ 5: sweep and commit
def _state_equal(a, b, what):
    for k in ("vals", "fc_store", "status", "iters", "obj", "relax_obj", "int_path", "rp"):
        x, y = getattr(a.batch, k), getattr(b.batch, k)
        assert torch.equal(_bits(x) if x.dtype == torch.float64 else x, _bits(y) if y.dtype == torch.float64 else y), (what, k)
    for k in ("clocks", "hist", "status_hist", "path_hist", "agg_hist"):
        x, y = getattr(a, k), getattr(b, k)
        assert torch.equal(_bits(x) if x.dtype == torch.float64 else x, _bits(y) if y.dtype == torch.float64 else y), (what, k)


def test_sweep_and_commit_under_class_prices(gpu, community):
    C = 3
    va, twin = _vector(community, "type"), _vector(community, "type")
    first = _class_prices()
    va.step(first)
    twin.step(first)
    rng = np.random.default_rng(11)
    cand = torch.as_tensor(rng.uniform(-0.15, 0.15, size=(E, C, P)))           # [E][C][P]: class scalars, some below -TOU
    sums = va.sweep(cand, hold=True)
    assert tuple(sums.shape) == (E, C, 3) and not torch.isnan(sums).any()
    _state_equal(va, twin, "a sweep only reads the live state")
    choice = torch.tensor([2, 0, 1], dtype=torch.int32, device=va.device)
    got = va.commit(choice)
    chosen = cand[torch.arange(E), choice.cpu().long()]                        # [E][P]
    want = twin.step(chosen)
    assert torch.equal(_bits(got), _bits(want))
    _state_equal(va, twin, "commit")
    for e in range(E):
        assert torch.equal(_bits(sums[e, int(choice[e])]), _bits(want[e])), e
    for e in range(E):                                                         # the candidates differ
        assert len({tuple(_bits(sums[e, c]).tolist()) for c in range(C)}) == C, e
    # two steps ahead: the sums equal two class steps of a twin under each candidate
    paths = va.sweep(cand, steps=2, hold=False)
    assert tuple(paths.shape) == (E, C, 2, 3)
    for c in range(C):
        t2 = _vector(community, "type")
        t2.step(first)
        t2.step(chosen)
        for j in range(2):
            s = t2.step(cand[:, c].contiguous())
            assert torch.equal(_bits(paths[:, c, j]), _bits(s)), (c, j)
    # the device tie key: sum over the classes of |first entry|, ascending
    key = va.tie_key(cand, C).cpu()
    ref = cand[..., 0].abs()
    for k in range(1, P):
        ref = ref + cand[..., k].abs()
    assert torch.equal(_bits(key), _bits(ref.t().reshape(C * E, 1)))
    assert va.select(sums, torch.zeros(E, dtype=torch.float64), cand).dtype == torch.int32


# ------------------------------------------------------------------ 6: the environments
def test_device_env_with_classes_equals_the_host_env(gpu, community):
    from dragg_amd.rl import DeviceVectorEnv, VectorEnv
    from dragg_amd.vector import plan_classes_reference, plan_groups_reference
    host = VectorEnv(_vector(community, "type"), _cfg())
    dev = DeviceVectorEnv(_vector(community, "type"), _cfg(), plan_keys=KEYS, plan_rows=ROWS)
    assert host.n_classes == dev.n_classes == 4 and dev.class_names[3] == "pv_battery"

    def check(obs_h, obs_d, what):
        _same_obs(obs_h, obs_d, what)
        _same_state(host, dev, what)
        b = dev.va.batch
        vals, fc = b.vals.cpu().numpy(), b.fc_store.cpu().numpy()
        ref = plan_classes_reference(vals, fc, E, dev.va.price_class_host, P, KEYS, ROWS)
        _same_plans([obs_d[k].cpu() for k in ("class_plan", "class_plan_count", "class_stats")],
                    [torch.as_tensor(r) for r in ref], what)
        ref = plan_groups_reference(vals, fc, E, KEYS, ROWS)
        _same_plans([obs_d[k].cpu() for k in ("plan", "plan_count", "plan_stats")], [torch.as_tensor(r) for r in ref], what)

    obs_d = dev.reset()
    assert tuple(obs_d["class_plan"].shape) == (E, P, 2, H) and tuple(obs_d["class_stats"].shape) == (E, P, 3, 4)
    views = {k: obs_d[k].data_ptr() for k in ("class_plan", "class_plan_count", "class_stats")}
    check(host.reset(), obs_d, "reset")
    scal = torch.as_tensor(np.array([[SCALARS[(c + e) % P] for c in range(P)] for e in range(E)]))      # [E][P]
    oh, _ = host.step(scal)
    od, _ = dev.step(scal.to(gpu))
    check(oh, od, "step 1: class scalars")
    one = torch.tensor([False, True, False], device=gpu)
    check(host.reset([1], seeds=[0, 77, 0]), dev.reset(one, seeds=torch.tensor([0, 77, 0], device=gpu)), "masked reset")
    assert int(dev.observations()["class_plan_count"][1].sum()) == 0           # a fresh episode's plan is empty
    lists = _class_prices()
    oh, _ = host.step(lists)
    od, _ = dev.step(lists.to(gpu))
    check(oh, od, "step 2: class lists")
    cand = torch.as_tensor(np.random.default_rng(3).uniform(-0.15, 0.15, size=(E, 3, P)))
    oh, _ = host.step_swept(cand)
    od, _ = dev.step_swept(cand.to(gpu))
    check(oh, od, "step 3: swept")
    assert host.choice.tolist() == dev.choice.cpu().tolist()
    assert views == {k: od[k].data_ptr() for k in views}                       # buffers allocated once
    # without classes the environment has no class observations
    plain = DeviceVectorEnv(_vector(community, None), _cfg(), plan_keys=KEYS, plan_rows=ROWS)
    assert "class_plan" not in plain.reset() and plain.n_classes == 1
