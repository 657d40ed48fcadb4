"""Price classes, host side (CPU): the ABI surface and argument errors of dragg_mpc_step_classes /
dragg_mpc_plan_classes, `MPCBatch.set_price_classes` and the class shapes of `set_reward_price`,
`vector.plan_classes_reference` against `plan_groups_reference` on hand-masked arrays, and the glue above them --
`VectorAggregator` (class prices reach each home by its class, sweep / commit install the chosen candidate's P
rows, the tie key), `VectorEnv`, `SweepAgent.act_vector(classes=P)` and the "type" map -- on a stand-in batch in
the style of tests/test_commit_host.py's, whose home step depends on the price row the home reads."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from tests.test_lookahead_host import AheadBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")
CPU = torch.device("cpu")
ENV = [0.0] * 64
TYPES = ["base", "pv_only", "battery_only", "pv_battery", "base", "battery_only"]
HOMES = [{"name": f"h{i}", "type": t} for i, t in enumerate(TYPES)]
CFG = {"agg": {"rl": {"prev_timesteps": 3}}, "rl": {"utility": {"action_space": [-1.0, 1.0], "action_scale": 100.0}}}


class ClassBatch(AheadBatch):
    """AheadBatch (HoldBatch with the K-step surface) with MPCBatch's class surface: `set_price_classes`, reward prices [G][P][n], and a step in
    which home r of group g reads row (g, class[r % Nb])."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n_classes, self.cls = 1, [0] * self.Nb
        self.seen = {}                      # (group, base home) -> the first price entry its last step read

    def set_price_classes(self, classes, n_classes=None):
        cm, self.n_classes = L.price_class_map(classes, self.Nb, n_classes)
        self.cls = cm.tolist()
        self.rp = torch.zeros((self.groups, self.n_classes, 1), dtype=torch.float64)

    def set_reward_price(self, rp):
        self.rp = rp.clone().reshape(self.groups, self.n_classes, -1)

    def step_episodes(self, seeds, starts, clocks, noise=None, hist=None, stream=None):
        self.solves += 1
        for g in range(self.groups):
            c = int(clocks[g])
            if c < 0:
                continue
            for i in range(self.Nb):
                r = g * self.Nb + i
                prev = 0.0 if c == 0 else float(self.vals[0, r])
                p = float(self.rp[g, self.cls[i], 0])
                self.seen[(g, i)] = p
                v = prev + (i + 1) * (1 + p) * (c + 1) + 0.001 * int(seeds[g]) + int(starts[g])
                self.vals[0, r], self.vals[1, r], self.vals[L.K["cost_opt"], r] = v, 2 * v, v * p
                self.fc[0, 0, r] = v
                self.status[r] = L.ST_OPTIMAL
                self.int_path[r] = 0
                if hist is not None:
                    hist[:, r] = self.vals[:, r]


def _va(E, price_classes, n_classes=None, T=5):
    from dragg_amd.vector import VectorAggregator
    return VectorAggregator(HOMES, ENV, ENV, ENV, E, list(range(5, 5 + E)), [0] * E, T, device=CPU,
                            batch_cls=ClassBatch, price_classes=price_classes, n_classes=n_classes)


def _same(a, b):
    nn = lambda x: x.nan_to_num(-7.5)  # noqa: E731
    return all(torch.equal(nn(getattr(a.batch, k)), nn(getattr(b.batch, k))) for k in ("vals", "fc", "rp")) \
        and torch.equal(a.clocks, b.clocks) and torch.equal(nn(a.hist), nn(b.hist)) \
        and torch.equal(a.agg_hist, b.agg_hist)


# ------------------------------------------------------------------ ABI surface, argument errors
def test_abi_surface_of_the_class_entry_points(tmp_path):
    from dragg_amd import build
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    new = ["dragg_mpc_step_classes", "dragg_mpc_plan_classes"]
    assert all(n in names and n in L.EXPORTS for n in new)
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and L.ABI_VERSION == 10
    assert re.search(r"#define\s+DRAGG_CLASS_MAX\s+64\b", h) and L.CLASS_MAX == 64
    lib = ctypes.CDLL(build.build())
    assert all(hasattr(lib, n) for n in new) and lib.dragg_mpc_abi_version() == 10
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(dragg_mpc_classes));']
    for f, _ in L.Classes._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(dragg_mpc_classes, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.Classes) == 16
    assert [f for f, _ in L.Classes._fields_] == ["n_classes", "price_class"]
    for f, _ in L.Classes._fields_:
        assert int(got[f]) == getattr(L.Classes, f).offset, f
    # the earlier structs keep their layouts
    assert ctypes.sizeof(L.Episodes) == 24 and ctypes.sizeof(L.Plan) == 32
    assert [f for f, _ in L.Dims._fields_][-1] == "n_groups"


def test_argument_errors_of_the_class_entry_points():
    """Empty shards and NULL device pointers only: no launch, no GPU."""
    lib = L.load()
    E_ARG = -1
    empty = L.Dims(n_homes=0, horizon=24, sub_steps=6, dt=4, n_draw_hours=48, n_env=100, n_rp=1,
                   int_mode=L.INT_ROUND, discount=0.92, n_groups=0)
    some = L.Dims.from_buffer_copy(empty)
    some.n_homes = 8
    prob, ep, hsh, out, plan = L.Problem(), L.Episodes(), L.Hash(), L.Out(), L.Plan()
    fake = ctypes.c_void_p(4096)             # never read: every call below returns before a launch
    ws_before = lib.dragg_mpc_workspace_bytes(ctypes.byref(some))

    def step(dims, cls):
        return lib.dragg_mpc_step_classes(dims, prob, ep, cls, hsh, out, 0, None, None)

    def plan_c(dims, cls, p=plan):
        return lib.dragg_mpc_plan_classes(dims, hsh, cls, p, None)

    bad = [L.Classes(n_classes=0, price_class=fake), L.Classes(n_classes=L.CLASS_MAX + 1, price_class=fake),
           L.Classes(n_classes=-3, price_class=fake), L.Classes(n_classes=2, price_class=None)]
    for cls in bad:
        for dims in (empty, some):
            assert step(dims, cls) == E_ARG, (cls.n_classes, dims.n_homes)
            assert plan_c(dims, cls) == E_ARG, (cls.n_classes, dims.n_homes)
    # n_homes == 0: a no-op, with and without classes (NULL, P == 1 with a NULL map, P == 2 and P == CLASS_MAX)
    for cls in (None, L.Classes(n_classes=1, price_class=None), L.Classes(n_classes=2, price_class=fake),
                L.Classes(n_classes=L.CLASS_MAX, price_class=fake)):
        assert step(empty, cls) == 0
        assert plan_c(empty, cls) == 0       # (no keys and no rows chosen: nothing to write)
    # wherever step_episodes / plan_groups return DRAGG_E_ARG: NULL ep, NULL per-home pointers, a key bit past NFC
    two = L.Classes(n_classes=2, price_class=fake)
    assert lib.dragg_mpc_step_classes(some, prob, None, two, hsh, out, 0, None, None) == E_ARG
    assert lib.dragg_mpc_step_classes(some, prob, None, None, hsh, out, 0, None, None) == E_ARG
    assert step(some, two) == E_ARG and step(some, None) == E_ARG          # NULL params, vals, ...
    assert plan_c(some, two, L.Plan(fc_keys=1 << L.NFC)) == E_ARG
    assert plan_c(some, two, L.Plan(fc_keys=1, curve=None, count=None)) == E_ARG
    assert plan_c(some, two, L.Plan(val_rows=1, stats=fake)) == E_ARG          # NULL hash.vals with homes
    odd = L.Dims.from_buffer_copy(some)
    odd.n_groups = 3                                                             # 8 homes are not 3 groups
    assert step(odd, two) == E_ARG and plan_c(odd, two, L.Plan(val_rows=1, stats=fake)) == E_ARG
    assert lib.dragg_mpc_workspace_bytes(ctypes.byref(some)) == ws_before


# ------------------------------------------------------------------ MPCBatch: the map and the price shapes
def _bare_batch(G=2, Nb=5, H=24):
    """An MPCBatch without a device: what set_price_classes / set_reward_price touch."""
    from dragg_amd.mpc import MPCBatch
    b = MPCBatch.__new__(MPCBatch)
    b.groups, b.Nb, b.N, b.H, b.device = G, Nb, G * Nb, H, CPU
    b.dims, b.workspace, b.lag = L.Dims(n_rp=1), None, None
    b.n_classes, b.price_class, b.price_class_host = 1, None, None
    return b


def test_set_price_classes_refuses_bad_maps():
    b = _bare_batch()
    for classes, P in (([0, 1, 2, 0], None), ([0, 1, 2, 0, 1, 2], None),          # wrong length
                       ([0, -1, 1, 0, 1], None), ([0, 1, 2, 0, 1], 2),             # negative, >= P
                       ([0, 1, 2, 3, L.CLASS_MAX], None), ([0] * 5, L.CLASS_MAX + 1), ([0] * 5, 0),
                       ([0, 0.5, 1, 0, 1], None)):
        with pytest.raises(ValueError):
            b.set_price_classes(classes, P)
        assert b.n_classes == 1 and b.price_class is None
    b.set_price_classes([0, 1, 2, 0, 1], 4)                 # (class 3 empty)
    assert b.n_classes == 4 and b.price_class.dtype == torch.int32 and b.price_class.tolist() == [0, 1, 2, 0, 1]
    assert tuple(b.rp.shape) == (2 * 4,) and b.dims.n_rp == 1 and float(b.rp.abs().sum()) == 0.0
    c = b._classes()
    assert c.n_classes == 4 and c.price_class == b.price_class.data_ptr()
    b.set_price_classes(list(range(5)), L.CLASS_MAX)
    assert b.n_classes == L.CLASS_MAX
    b.set_price_classes(None)
    assert b.n_classes == 1 and b.price_class is None and tuple(b.rp.shape) == (2,)
    # like a grouped batch: no lag mode, no explicit inputs, and step_episodes is the solve
    b.set_price_classes([0, 1, 0, 1, 0])
    for call in (lambda: b.enable_lag(), lambda: b.solve_explicit(*[None] * 10), lambda: b.step(0)):
        with pytest.raises(ValueError):
            call()


def test_set_reward_price_class_shapes():
    G, P, H = 2, 3, 24
    b = _bare_batch(G=G, H=H)
    b.set_price_classes([0, 1, 2, 0, 1])
    gp = torch.arange(G * P, dtype=torch.float64).reshape(G, P) / 8
    b.set_reward_price(gp)                                                  # [G][P]
    assert b.dims.n_rp == 1 and torch.equal(b.rp, gp.reshape(-1))
    gpn = torch.arange(G * P * H, dtype=torch.float64).reshape(G, P, H) / 64
    b.set_reward_price(gpn)                                                 # [G][P][n]
    assert b.dims.n_rp == H and torch.equal(b.rp, gpn.reshape(-1))
    b.set_reward_price([0.25, 0.5, 0.75])                                   # [P] for every group
    assert b.dims.n_rp == 1 and b.rp.tolist() == [0.25, 0.5, 0.75] * G
    pn = np.arange(P * (H + 2), dtype=float).reshape(P, H + 2)
    b.set_reward_price(pn)                                                  # [P][n], n >= H
    assert b.dims.n_rp == H + 2 and torch.equal(b.rp.reshape(G, P, H + 2)[1], torch.as_tensor(pn))
    for bad in ([0.0], [0.0] * 4, np.zeros((G, P + 1)), np.zeros((G + 1, P)), np.zeros((G, P, 0)),
                np.zeros((G, 2, P, 1)), np.zeros((G, P, 4)), np.zeros((P, H - 1))):      # the length rule: 1 or >= H
        with pytest.raises(ValueError):
            b.set_reward_price(bad)
    assert b.dims.n_rp == H + 2                                              # (a refused price changes nothing)
    # without classes the grouped shapes are today's
    b.set_price_classes(None)
    b.set_reward_price(torch.tensor([[0.5], [0.25]], dtype=torch.float64))
    assert b.rp.tolist() == [0.5, 0.25] and b.dims.n_rp == 1
    with pytest.raises(ValueError):
        b.set_reward_price(np.zeros((G, P, 1)))


# ------------------------------------------------------------------ plan_classes_reference
def _plan_arrays(G, Nb, H, seed=3):
    rng = np.random.default_rng(seed)
    N = G * Nb
    vals, fc = rng.normal(size=(L.NVAL, N)) * 1e3, rng.normal(size=(N, L.NFC, H)) * 1e3
    vals[L.K["solve_counter"]] = rng.integers(0, H + 2, size=N)
    vals[L.K["solve_counter"], ::7] = np.nan                 # homes that never solved
    vals[L.K["p_pv_opt"], 1::2] = np.nan                     # absent fields overlap the class masks
    fc[1::2, L.K["p_pv_opt"]] = np.nan
    vals[L.K["cost_opt"], 5] = np.nan
    return vals, fc


def test_plan_classes_reference_is_plan_groups_on_masked_arrays():
    from dragg_amd.vector import plan_classes_reference, plan_groups_reference
    G, Nb, H, P = 2, 37, 6, 4                                # 37 homes: ragged ways; class 3: empty
    vals, fc = _plan_arrays(G, Nb, H)
    cm = np.array([(i * 5 + i // 3) % 3 for i in range(Nb)])
    assert set(cm.tolist()) == {0, 1, 2}
    keys, rows = ("p_grid", "p_load", "p_pv"), ("p_grid", "cost", "p_pv", "solve_counter")
    curve, count, stats = plan_classes_reference(vals, fc, G, cm, P, keys, rows)
    assert curve.shape == (G, P, 3, H) and count.shape == (G, P, 3, H) and stats.shape == (G, P, 4, 4)
    assert count.dtype == np.int32
    whole = plan_groups_reference(vals, fc, G, keys, rows)
    for c in range(P):
        v, f = vals.copy(), fc.copy()
        for g in range(G):
            for i in range(Nb):
                if cm[i] != c:
                    v[:, g * Nb + i] = np.nan
                    f[g * Nb + i] = np.nan
        ref = plan_groups_reference(v, f, G, keys, rows)
        for got, want in zip((curve, count, stats), ref):
            assert np.array_equal(got[:, c].view(np.int64) if got.dtype == np.float64 else got[:, c],
                                  want.view(np.int64) if want.dtype == np.float64 else want), c
    # the classes partition the homes
    assert np.array_equal(count.sum(axis=1), whole[1]) and np.array_equal(stats[:, :, :, 0].sum(axis=1), whole[2][:, :, 0])
    assert np.allclose(curve.sum(axis=1), whole[0], rtol=1e-12, atol=1e-9)
    # the empty class: sum +0.0, count 0, min +inf, max -inf
    assert not count[:, 3].any() and not curve[:, 3].any() and not np.signbit(curve[:, 3]).any()
    assert np.array_equal(stats[:, 3], np.tile([0.0, 0.0, np.inf, -np.inf], (G, 4, 1)))
    # P = 1: plan_groups_reference itself
    one = plan_classes_reference(vals, fc, G, np.zeros(Nb, dtype=int), 1, keys, rows)
    for got, want in zip(one, whole):
        assert got.shape == (G, 1) + want.shape[1:] and np.array_equal(got[:, 0], want, equal_nan=True)
    with pytest.raises(ValueError):
        plan_classes_reference(vals, fc, G, cm[:-1], P, keys, rows)
    with pytest.raises(ValueError):
        plan_classes_reference(vals, fc, G, cm, 2, keys, rows)


# ------------------------------------------------------------------ VectorAggregator, VectorEnv, SweepAgent
def test_type_classes_and_explicit_maps():
    from dragg_amd.vector import resolve_price_classes
    cm, P, names = resolve_price_classes("type", HOMES)
    assert cm.tolist() == [0, 1, 2, 3, 0, 2] and P == 4
    assert names == ["base", "pv_only", "battery_only", "pv_battery"]
    cm, P, _ = resolve_price_classes("type", HOMES[:2])       # P is 4 even if a type is absent
    assert cm.tolist() == [0, 1] and P == 4
    assert resolve_price_classes(None, HOMES) == (None, 1, None)
    cm, P, names = resolve_price_classes([i % 3 for i in range(6)], HOMES, 4)
    assert cm.tolist() == [0, 1, 2, 0, 1, 2] and P == 4 and names == ["0", "1", "2", "3"]
    for bad in ("kind", [0, 1], [0, 1, 2, 3, 4, 64]):
        with pytest.raises(ValueError):
            resolve_price_classes(bad, HOMES)
    va = _va(2, "type")
    assert va.n_classes == 4 and va.batch.n_classes == 4 and va.batch.cls == [0, 1, 2, 3, 0, 2]
    assert _va(2, None).n_classes == 1 and _va(2, None).batch.n_classes == 1


def test_class_prices_reach_each_home_by_its_class():
    E, P = 3, 4
    va, cls = _va(E, "type"), [0, 1, 2, 3, 0, 2]
    prices = torch.arange(E * P, dtype=torch.float64).reshape(E, P) / 16 - 0.25
    for t in range(2):
        out = va.step(prices)                                # [E][P]: class scalars
        assert tuple(out.shape) == (E, 3)
        for e in range(E):
            for i in range(6):
                assert va.batch.seen[(e, i)] == float(prices[e, cls[i]]), (e, i)
    # each class's homes equal a run of the community under that class's price alone (homes do not interact)
    for e in range(E):
        for c in range(P):
            one = _va(E, None)
            for t in range(2):
                one.step(prices[:, c].contiguous())
            cols = [e * 6 + i for i in range(6) if cls[i] == c]
            assert torch.equal(va.batch.vals[:2, cols], one.batch.vals[:2, cols]), (e, c)
    # [E][P][n] lists: the row's first entry is what the stand-in reads
    lists = torch.stack([prices + 1, prices * 0], dim=2)
    va.step(lists)
    assert va.batch.seen[(2, 3)] == float(prices[2, 3]) + 1
    for bad in (prices[:, :3], prices.reshape(-1), torch.zeros(E, 3, 2), torch.zeros(E)):
        with pytest.raises(ValueError):
            va.step(bad)


def test_sweep_commit_installs_the_chosen_candidates_rows():
    E, C, P = 3, 3, 4
    va, twin = _va(E, [i % 3 for i in range(6)], 4), _va(E, [i % 3 for i in range(6)], 4)
    first = torch.full((E, P), 0.125, dtype=torch.float64)
    va.step(first)
    twin.step(first)
    cand = (torch.arange(E * C * P, dtype=torch.float64).reshape(E, C, P) - 7) / 32
    sums = va.sweep(cand, hold=True)
    assert tuple(sums.shape) == (E, C, 3)
    rb = va._sweep_batches[C]
    assert rb.n_classes == 4 and rb.cls == va.batch.cls                   # the sweep batch has the same map
    assert torch.equal(rb.rp.reshape(C, E, P), cand.transpose(0, 1))
    choice = torch.tensor([2, 0, 1], dtype=torch.int32)
    got = va.commit(choice)
    chosen = cand[torch.arange(E), choice.long()]                          # [E][P]
    want = twin.step(chosen)
    assert torch.equal(got, want) and _same(va, twin)
    assert torch.equal(va.batch.rp.reshape(E, P), chosen)                  # the chosen candidate's P rows
    for e in range(E):
        assert torch.equal(sums[e, int(choice[e])], want[e])
    # K-step sweeps carry the class rows through every step
    paths = va.sweep(cand, steps=2, hold=False)
    assert tuple(paths.shape) == (E, C, 2, 3)
    for c in range(C):
        t2 = _va(E, [i % 3 for i in range(6)], 4)
        for p in (first, chosen, cand[:, c], cand[:, c]):
            last = t2.step(p.contiguous())
        assert torch.equal(paths[:, c, 1], last), c
    for bad in (cand[:, :, :3], cand.reshape(E, -1), torch.zeros(E, C)):
        with pytest.raises(ValueError):
            va.sweep(bad)


def test_tie_key_sums_the_classes_in_ascending_order():
    E, C, P = 2, 3, 4
    va = _va(E, "type")
    # magnitudes whose sum depends on the order of the adds
    cand = torch.tensor([1e16, -1.0, 1.0, -0.0], dtype=torch.float64).repeat(E, C, 1)
    cand[1, 2] = torch.tensor([-0.1, 0.2, -0.3, 0.4], dtype=torch.float64)
    key = va.tie_key(cand, C)
    assert tuple(key.shape) == (C * E, 1)
    for e in range(E):
        for c in range(C):
            acc = np.float64(0.0)
            for k in range(P):
                acc = acc + np.abs(np.float64(cand[e, c, k]))
            assert float(key[c * E + e, 0]) == acc, (e, c)
    assert float(key[0, 0]) == ((1e16 + 1.0) + 1.0) + 0.0 == 1e16 != 1e16 + (1.0 + 1.0 + 0.0)
    # [E][C][P][n]: the first entry of every class's row
    lists = torch.stack([cand, cand * 0 + 9], dim=3)
    assert torch.equal(va.tie_key(lists, C), key)
    assert torch.equal(va._tie_rows(lists, C), key)
    # one class: |first column| of today's rows, bit for bit -- the key the select kernels take of them
    v1 = _va(E, None)
    p1 = torch.tensor([[-0.25, 0.5, -0.0], [0.125, -1e-300, 3.0]], dtype=torch.float64)
    rows = v1._tie_rows(p1, C)
    assert torch.equal(rows, p1.t().reshape(C * E, 1))                     # today's rows, untouched
    assert torch.equal(v1.tie_key(p1, C).view(torch.int64), rows[:, :1].abs().view(torch.int64))
    # select: ties in the load go to the smaller key
    va.step(torch.zeros(E, P, dtype=torch.float64))
    tie = torch.zeros(E, C, P, dtype=torch.float64)
    tie[:, 0, 3], tie[:, 2, 3] = 0.0, 0.0
    tie[:, 0, 0], tie[:, 1, 0], tie[:, 2, 0] = 0.5, -0.25, 0.375       # only class 0 differs: homes 0 and 4
    sums = va.sweep(tie)
    flat = sums.clone()
    flat[:, :, 0] = 1.0                                                   # every load ties
    assert va.select(flat, torch.ones(E, dtype=torch.float64), tie).tolist() == [1, 1]


def test_vector_env_and_sweep_agent_take_class_shapes():
    from dragg_amd.rl import SweepAgent, VectorEnv
    E, P = 2, 4
    env = VectorEnv(_va(E, "type", T=3), CFG, max_poss_load=40.0)
    assert env.n_classes == 4 and env.class_names == ["base", "pv_only", "battery_only", "pv_battery"]
    plain = VectorEnv(_va(E, None, T=3), CFG, max_poss_load=40.0)
    assert plain.n_classes == 1 and plain.class_names is None
    env.reset()
    plain.reset()
    agent = SweepAgent(CFG, n_candidates=3)
    cand = agent.act_vector(env.observations(), classes=P)
    assert cand.shape == (E, 3, P) and np.array_equal(cand[:, :, 0], agent.act_vector(env.observations()))
    assert all(np.array_equal(cand[:, :, 0], cand[:, :, c]) for c in range(P))
    # the same grid value in every class: the class environment lives the plain one's episode
    for k in range(3):
        obs, done = env.step_swept(cand, lookahead=1 + k % 2)
        ref, rdone = plain.step_swept(cand[:, :, 0], lookahead=1 + k % 2)
        assert env.choice.tolist() == plain.choice.tolist()
        for key in ref:
            assert np.array_equal(obs[key], ref[key]), (k, key)
    assert done.all() and rdone.all()
    # class actions
    env.reset()
    obs, _ = env.step(np.full((E, P), 0.25))
    assert obs["timestep"].tolist() == [1, 1]
    with pytest.raises(ValueError):
        env.step(np.zeros(E))


def test_rl_vector_passes_the_map_on():
    from dragg_amd.runner import Aggregator
    a = Aggregator.__new__(Aggregator)
    a.world, a.start_hour_index, a.num_timesteps, a.int_mode, a.device = 1, 0, 4, "round", CPU
    a.batch_cls, a.all_homes, a.check_type = ClassBatch, HOMES, "all"
    a.config = {"simulation": {"random_seed": 12}, **CFG}
    a._checked_community = lambda: ([h for h in a.all_homes if a.check_type == "all" or h["type"] == a.check_type],
                                    ENV, ENV, ENV)
    import dragg_amd.inputs as I
    keep, I.max_load = I.max_load, lambda h: 5.0
    try:
        env = a.rl_vector(2, price_classes="type")
        assert env.n_classes == 4 and env.va.batch.cls == [0, 1, 2, 3, 0, 2]
        assert a.rl_vector(2).n_classes == 1
        env = a.rl_vector(2, price_classes=[0, 1, 0, 1, 0, 2])
        assert env.n_classes == 3 and env.va.batch.cls == [0, 1, 0, 1, 0, 2]
        # the config's default, and one class per LOADED home when only one type is checked
        a.config["rl"] = {"utility": {**CFG["rl"]["utility"], "price_classes": [0, 1, 0, 1, 2, 1]}}
        assert a.rl_vector(2).va.batch.cls == [0, 1, 0, 1, 2, 1]
        a.check_type = "base"
        env = a.rl_vector(2)
        assert env.n_classes == 3 and env.va.batch.cls == [0, 2]
        with pytest.raises(ValueError):
            a.rl_vector(2, price_classes=[0, 1])
    finally:
        I.max_load = keep
