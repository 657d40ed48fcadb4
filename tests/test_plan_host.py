"""Plan observations, host side (CPU): the ABI surface of dragg_mpc_plan_groups, its numpy restatement
(`vector.plan_groups_reference`) against an independent formulation (masks per home and stage, `math.fsum`),
hand-made counters, the summation order, group independence, and the Python layers on stand-in batches whose
`plan_groups` is served by the restatement (tests/test_env_host.py's stand-ins): `rl.DeviceVectorEnv`'s
observations, `DeviceAggregator.sweep_plan` without a hold, and `DeviceAggregator.plan` over two gloo ranks."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dragg_amd import _lib as L
from tests.test_distributed import _free_port
from tests.test_env_host import EnvBatch, _cfg, _va

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")
NAN = float("nan")
CNT = L.K["solve_counter"]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _random_hash(rng, N, H, nan_share=0.15):
    """Random hash arrays: counters in and out of [0, H) and NaN, NaN fields scattered over both arrays."""
    vals = rng.uniform(-50.0, 50.0, (L.NVAL, N))
    fc = rng.uniform(-50.0, 50.0, (N, L.NFC, H))
    vals[rng.random(vals.shape) < nan_share] = NAN
    fc[rng.random(fc.shape) < nan_share] = NAN
    vals[CNT] = rng.choice([0.0, 1.0, 2.0, H - 1.0, float(H), H + 3.0, NAN], N)
    return vals, fc


def _independent(vals, fc, G, ki, ri):
    """Another formulation of the contract: a [Nb][H] table of values and a presence mask per key, then
    `math.fsum` (the exactly rounded sum) and exact counts, min and max."""
    N, H = vals.shape[1], fc.shape[2]
    Nb = N // G
    cnt = vals[CNT]
    ok = (cnt >= 0) & (cnt < H)                                      # (NaN: False)
    c = np.where(ok, np.nan_to_num(cnt), H).astype(int)
    curve, count = np.zeros((G, len(ki), H)), np.zeros((G, len(ki), H), dtype=np.int64)
    stats = np.zeros((G, len(ri), 4))
    for g in range(G):
        n = np.arange(g * Nb, (g + 1) * Nb)
        for a, k in enumerate(ki):
            table = np.full((Nb, H), NAN)
            table[:, 0] = vals[k, n]
            for j in range(1, H):
                src = c[n] + j
                inside = src < H
                table[inside, j] = fc[n[inside], k, src[inside]]
            present = ~np.isnan(table)
            count[g, a] = present.sum(0)
            curve[g, a] = [math.fsum(table[present[:, j], j]) for j in range(H)]
        for a, r in enumerate(ri):
            v = vals[r, n]
            v = v[~np.isnan(v)]
            stats[g, a] = (len(v), math.fsum(v), v.min() if len(v) else np.inf, v.max() if len(v) else -np.inf)
    return curve, count, stats


# ------------------------------------------------------------------ ABI surface
def test_abi_surface_of_the_plan_entry_point(tmp_path):
    from dragg_amd import build
    h = open(HEADER).read()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", h, re.M)
    assert "dragg_mpc_plan_groups" in names and "dragg_mpc_plan_groups" in L.EXPORTS
    assert "typedef struct dragg_mpc_plan" in h
    assert re.search(r"#define\s+DRAGG_MPC_ABI_VERSION\s+10\b", h) and L.ABI_VERSION == 10
    assert re.search(r"#define\s+DRAGG_PLAN_WAYS\s+16\b", h) and L.PLAN_WAYS == 16
    assert len(L.PLAN_KEYS) == L.NFC and len(L.PLAN_ROWS) == L.NVAL
    # the short names are the header's enumerators, in its order
    enum = re.search(r"enum dragg_fc_key \{(.*?)DRAGG_NFC", h, re.S).group(1)
    assert [n.lower() for n in re.findall(r"DRAGG_K_(\w+)", enum)] == list(L.PLAN_KEYS)
    enum = re.search(r"enum dragg_val \{(.*?)DRAGG_NVAL", h, re.S).group(1)
    assert [n.lower() for n in re.findall(r"DRAGG_V_(\w+)", enum)] == list(L.PLAN_ROWS[L.NFC:])
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "dragg_mpc_plan_groups") and lib.dragg_mpc_abi_version() == 10
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(dragg_mpc_plan));']
    for f, _ in L.Plan._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(dragg_mpc_plan, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(L.Plan) == 32
    assert [f for f, _ in L.Plan._fields_] == ["fc_keys", "val_rows", "curve", "count", "stats"]
    for f, _ in L.Plan._fields_:
        assert int(got[f]) == getattr(L.Plan, f).offset, f


def test_plan_select_and_shape():
    km, rm, ki, ri = L.plan_select(("p_load", "p_grid", "p_grid_opt", 2), ("solve_counter", "e_batt"))
    assert (km, ki) == (0b101, [0, 2]) and ri == [L.NFC - 1, L.NVAL - 1] and rm == (1 << 14) | (1 << 18)
    assert L.plan_select((), ()) == (0, 0, [], [])
    assert L.plan_select("cost")[2] == [8]
    assert L.plan_shape(("p_grid", "p_load"), ("e_batt",), G=3, H=24) == ((3, 2, 24), (3, 1, 4))
    for bad in (("nope",), (L.NFC,), (-1,), ("temp_in_opt",)):
        with pytest.raises(ValueError):
            L.plan_select(bad)
    with pytest.raises(ValueError):
        L.plan_select((), (L.NVAL,))


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("G,Nb,H", [(1, 1, 6), (2, 15, 7), (3, 17, 6), (1, 33, 24), (2, 40, 5)])
def test_restatement_against_an_independent_formulation(G, Nb, H):
    from dragg_amd.vector import plan_groups_reference
    rng = np.random.default_rng(1000 * G + 10 * Nb + H)
    vals, fc = _random_hash(rng, G * Nb, H)
    keys, rows = list(range(L.NFC)), list(range(L.NVAL))
    curve, count, stats = plan_groups_reference(vals, fc, G, keys, rows)
    assert curve.shape == (G, L.NFC, H) and count.shape == curve.shape and count.dtype == np.int32
    assert stats.shape == (G, L.NVAL, 4)
    c2, n2, s2 = _independent(vals, fc, G, keys, rows)
    assert np.array_equal(count, n2)
    # (1e-12 relative to the sum of magnitudes: the values have both signs, so a sum may cancel to nothing)
    scale = 50.0 * np.maximum(n2, 1)
    assert np.all(np.abs(curve - c2) <= 1e-12 * scale)
    assert np.array_equal(stats[..., 0], s2[..., 0])
    assert np.all(np.abs(stats[..., 1] - s2[..., 1]) <= 1e-12 * 50.0 * np.maximum(s2[..., 0], 1))
    assert np.array_equal(stats[..., 2], s2[..., 2]) and np.array_equal(stats[..., 3], s2[..., 3])
    assert 0 < count.max() <= Nb and (Nb < 4 or count.min() < count.max())      # (present and absent values both occur)
    # a subset of the keys, in any order: the same rows, ascending
    sub = plan_groups_reference(vals, fc, G, ("e_batt", "p_grid", "cost"), ("solve_counter",))
    assert np.array_equal(_bits(sub[0]), _bits(curve[:, [0, 8, 14]])) and np.array_equal(sub[1], count[:, [0, 8, 14]])
    assert np.array_equal(_bits(sub[2]), _bits(stats[:, [CNT]]))


def test_positive_sums_agree_to_1e12_relative():
    """All values positive: the restatement's sums against `math.fsum` to 1e-12 relative to the sum itself."""
    from dragg_amd.vector import plan_groups_reference
    rng = np.random.default_rng(7)
    N, H = 70, 9
    vals, fc = rng.uniform(0.1, 9.0, (L.NVAL, N)), rng.uniform(0.1, 9.0, (N, L.NFC, H))
    vals[CNT] = rng.integers(0, H + 2, N)
    curve, count, stats = plan_groups_reference(vals, fc, 2, (0, 2), ("temp_in_opt",))
    c2, n2, s2 = _independent(vals, fc, 2, [0, 2], [L.K["temp_in_opt"]])
    assert np.array_equal(count, n2)
    assert np.all(np.abs(curve - c2) <= 1e-12 * np.abs(c2))
    assert np.all(np.abs(stats[..., 1] - s2[..., 1]) <= 1e-12 * np.abs(s2[..., 1]))


def test_hand_made_counters():
    """One home per counter in {0, 1, H-1, H, H+3, NaN}: fc[n][k][s] = 1000 n + s, vals[k][n] = -(n + 1)."""
    from dragg_amd.vector import plan_groups_reference
    H = 6
    counters = [0.0, 1.0, H - 1.0, float(H), H + 3.0, NAN]
    N = len(counters)
    vals = np.full((L.NVAL, N), NAN)
    fc = np.zeros((N, L.NFC, H))
    for n in range(N):
        fc[n, :, :] = 1000.0 * n + np.arange(H)
    vals[0] = -(np.arange(N) + 1.0)
    vals[CNT] = counters
    curve, count, stats = plan_groups_reference(vals, fc, 1, ("p_grid",), ("solve_counter",))
    # entry 0: the collected values of all six homes
    assert curve[0, 0, 0] == -21.0 and count[0, 0, 0] == 6
    # entry j >= 1: home 0 (c = 0) gives fc[.][j]; home 1 (c = 1) fc[.][1 + j] while 1 + j < H; the others nothing
    for j in range(1, H):
        want, n = float(j), 1
        if 1 + j < H:
            want, n = want + 1000.0 + 1 + j, 2
        assert curve[0, 0, j] == want and count[0, 0, j] == n, j
    # home 2 (c = H - 1) contributes to entry 0 only: c + 1 == H
    # the counter row itself: five present values, NaN absent
    assert stats[0, 0].tolist() == [5.0, 0.0 + 1.0 + (H - 1.0) + H + (H + 3.0), 0.0, H + 3.0]
    # a negative counter is treated like one at or past H
    vals[CNT, 0] = -1.0
    curve, count, _ = plan_groups_reference(vals, fc, 1, ("p_grid",))
    assert count[0, 0].tolist() == [6, 1, 1, 1, 1, 0] and curve[0, 0, 1] == 1002.0


def test_all_nan_group_and_a_key_nobody_has():
    from dragg_amd.vector import plan_groups_reference
    H, Nb = 5, 4
    rng = np.random.default_rng(3)
    vals, fc = rng.uniform(1.0, 2.0, (L.NVAL, 2 * Nb)), rng.uniform(1.0, 2.0, (2 * Nb, L.NFC, H))
    vals[CNT] = 0.0
    vals[:, Nb:] = NAN                                      # group 1: a fresh batch's state
    fc[Nb:] = NAN
    vals[L.K["p_pv_opt"]] = NAN                             # nobody has PV
    fc[:, L.K["p_pv_opt"]] = NAN
    curve, count, stats = plan_groups_reference(vals, fc, 2, ("p_grid", "p_pv"), ("e_batt", "p_pv"))
    assert count[0, 0].tolist() == [Nb] * H and count[0, 1].tolist() == [0] * H
    assert not count[1].any() and not curve[1].any() and not np.signbit(curve[1]).any()
    assert not np.signbit(curve[0, 1]).any() and not curve[0, 1].any()
    for row in (stats[0, 0], stats[1, 0], stats[1, 1]):      # (p_pv sorts before e_batt: stats[., 0] is p_pv's)
        assert row.tolist() == [0.0, 0.0, np.inf, -np.inf] and not np.signbit(row[1])
    assert stats[0, 1, 0] == Nb and stats[0, 1, 2] >= 1.0 and stats[0, 1, 3] <= 2.0


def test_the_summation_order_is_the_contracts():
    """1e16, 1.0 and -1e16 (1.0 is half an ulp of 1e16: 1e16 + 1.0 == 1e16) placed so that the order shows: the
    order inside a way, homes spread over the ways against a left-to-right sum over the homes, and the tree's
    pairing against a left-to-right sum over the partials."""
    from dragg_amd.vector import plan_groups_reference
    H, N = 2, 48
    big = np.float64(1e16)
    assert big + 1.0 == big and -big + 1.0 == -big

    def run(homes, values):
        vals = np.full((L.NVAL, N), NAN)
        vals[CNT] = 0.0
        vals[0] = 0.0
        vals[0, homes] = values
        return plan_groups_reference(vals, np.zeros((N, L.NFC, H)), 1, (0,))[0][0, 0, 0], vals[0]
    # inside way 0 (homes 0, 16, 32), ascending: (big + 1) - big = 0; the exact sum is 1
    got, col = run([0, 16, 32], [big, 1.0, -big])
    assert got == 0.0 and math.fsum(col) == 1.0
    # ... and with the cancellation first: (big - big) + 1 = 1
    assert run([0, 16, 32], [big, -big, 1.0])[0] == 1.0
    # homes over the ways: p0 = big - big = 0 (homes 0, 16), p1 = 1 + 1 (homes 1, 17) -> 2, where a left-to-right
    # sum over homes 0, 1, 16, 17 gives ((big + 1) - big) + 1 = 1
    got, col = run([0, 1, 16, 17], [big, 1.0, -big, 1.0])
    assert got == 2.0
    ltr = np.float64(0.0)
    for x in col:
        ltr = ltr + x
    assert ltr == 1.0
    # the tree over the partials p0..p3 = big, 1, -big, 1: (big + 1) + (-big + 1) = big - big = 0, where a
    # left-to-right sum of the partials gives ((big + 1) - big) + 1 = 1 and the pairing (p0 + p2) + (p1 + p3) gives 2
    got, col = run([0, 1, 2, 3], [big, 1.0, -big, 1.0])
    assert got == 0.0 and ((col[0] + col[1]) + col[2]) + col[3] == 1.0 and (col[0] + col[2]) + (col[1] + col[3]) == 2.0
    # the second level: ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)) = ((big + 0) + (1 + 0)) + ((-big + 0) + (1 + 0))
    # = big + (-big) = 0
    assert run([0, 2, 4, 6], [big, 1.0, -big, 1.0])[0] == 0.0


def test_group_independence():
    """Rows of group g of a [G * Nb] array equal the restatement on the sliced group alone, bit for bit."""
    from dragg_amd.vector import plan_groups_reference
    rng = np.random.default_rng(11)
    G, Nb, H = 3, 19, 7
    vals, fc = _random_hash(rng, G * Nb, H)
    keys, rows = (0, 1, 10, 14), ("temp_in_opt", "e_batt", "correct_solve", "solve_counter")
    whole = plan_groups_reference(vals, fc, G, keys, rows)
    for g in range(G):
        cols = slice(g * Nb, (g + 1) * Nb)
        alone = plan_groups_reference(vals[:, cols], fc[cols], 1, keys, rows)
        assert np.array_equal(_bits(whole[0][g]), _bits(alone[0][0])) and np.array_equal(whole[1][g], alone[1][0])
        assert np.array_equal(_bits(whole[2][g]), _bits(alone[2][0]))
    with pytest.raises(ValueError):
        plan_groups_reference(vals, fc, 2, keys)


# ------------------------------------------------------------------ the Python layers on stand-in batches
class PlanBatch(EnvBatch):
    """tests/test_env_host.py's stand-in with `plan_groups` served by the restatement."""

    def plan_groups(self, keys, rows=(), out=None, stream=None, src=None):
        from dragg_amd.vector import plan_groups_reference
        b = self if src is None else src
        got = plan_groups_reference(b.vals.numpy(), b.fc.permute(2, 0, 1).numpy(), b.groups, keys, rows)
        got = tuple(torch.as_tensor(x) for x in got)
        if out is None:
            return got
        for o, x in zip(out, got):
            o.copy_(x)
        return tuple(out)


def test_default_observations_have_exactly_todays_keys():
    from dragg_amd.rl import DeviceVectorEnv
    env = DeviceVectorEnv(_va(2, [1, 2], [0, 0], 4, EnvBatch), _cfg(3), max_poss_load=40.0)   # (a batch without plan_groups)
    obs = env.reset()
    assert tuple(obs) == L.OBS_KEYS
    obs, _ = env.step([0.1, 0.2])
    assert tuple(obs) == L.OBS_KEYS and tuple(env.observations()) == L.OBS_KEYS


def test_plan_observations_on_a_stand_in():
    from dragg_amd.rl import DeviceVectorEnv
    from dragg_amd.vector import plan_groups_reference
    E, T = 3, 4
    va = _va(E, [1, 2, 3], [0, 1, 2], T, PlanBatch)
    env = DeviceVectorEnv(va, _cfg(3), max_poss_load=40.0, plan_keys=("p_load", "p_grid"), plan_rows=("solve_counter",))
    assert env.plan_key_names == ["p_grid", "p_load"] and env.plan_row_names == ["solve_counter"]
    obs = env.reset()
    assert tuple(obs) == L.OBS_KEYS + ("plan", "plan_count", "plan_stats")
    assert tuple(obs["plan"].shape) == (E, 2, va.H) and obs["plan_count"].dtype == torch.int32
    assert tuple(obs["plan_stats"].shape) == (E, 1, 4) and not obs["plan_count"].any()       # fresh: nothing planned
    buffers = [obs[k].data_ptr() for k in ("plan", "plan_count", "plan_stats")]
    env.park([1])
    for k in range(2):
        obs, _ = env.step([0.1, 0.2, 0.3])
        ref = plan_groups_reference(va.batch.vals.numpy(), va.batch.fc.permute(2, 0, 1).numpy(), E, (0, 2), (CNT,))
        assert np.array_equal(_bits(obs["plan"].numpy()), _bits(ref[0])) and np.array_equal(obs["plan_count"].numpy(), ref[1])
        assert np.array_equal(_bits(obs["plan_stats"].numpy()), _bits(ref[2]))
        assert [obs[k].data_ptr() for k in ("plan", "plan_count", "plan_stats")] == buffers   # allocated once
        # entry 0 of p_grid is the step's load (the stand-in's vals[0]); the parked episode has none
        assert obs["plan"][0, 0, 0] == obs["agg_load"][0] and int(obs["plan_count"][1].sum()) == 0
    c, n, s = va.plan(("p_grid",))
    assert tuple(c.shape) == (E, 1, va.H) and tuple(s.shape) == (E, 0, 4)


def test_sweep_plan_raises_without_a_hold():
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.vector import plan_groups_reference
    from tests.test_sweep_host import PRICES, SweepBatch

    class Batch(SweepBatch):
        plan_groups = PlanBatch.plan_groups
    homes = [{"name": f"h{i}"} for i in range(5)]
    agg = DeviceAggregator(homes, None, None, None, 0, 6, device=torch.device("cpu"), batch_cls=Batch)
    agg.run_iteration()
    agg.collect_data()
    assert not agg.holds()
    with pytest.raises(ValueError, match="held"):
        agg.sweep_plan(("p_grid",))
    agg.sweep(PRICES, 1)                                             # (not held)
    with pytest.raises(ValueError, match="held"):
        agg.sweep_plan(("p_grid",))
    for steps in (1, 2):                                             # the replica batch itself / a Held
        agg.sweep(PRICES, steps, hold=True)
        src = agg._hold["src"]
        assert (src is agg._sweep_batches[3]) == (steps == 1)
        got = agg.sweep_plan(("p_grid",), ("p_grid",))
        ref = plan_groups_reference(src.vals.numpy(), src.fc.permute(2, 0, 1).numpy(), 3, (0,), (0,))
        assert tuple(got[0].shape) == (3, 1, 4) and float(got[0][0, 0, 0]) != float(got[0][1, 0, 0])
        for x, y in zip(got, ref):
            assert np.array_equal(x.numpy(), y)
    agg.run_iteration()                                              # the live state moves: the hold is void
    with pytest.raises(ValueError, match="held"):
        agg.sweep_plan(("p_grid",))


class ShardBatch:
    """A shard's hash arrays, filled from the global home index (so that every sharding sees the same homes)."""
    H = 5

    def __init__(self, homes, *a, home_offset=0, home_stride=1, device=None, **kw):
        self.N, self.groups = len(homes), 1
        gidx = home_offset + home_stride * np.arange(self.N)
        rng = np.random.default_rng(99)
        vals_all, fc_all = _random_hash(rng, 64, self.H)
        self.vals = torch.as_tensor(vals_all[:, gidx].copy())
        self.fc = torch.as_tensor(fc_all[gidx].copy()).permute(1, 2, 0)
        self.status = torch.zeros(self.N, dtype=torch.int32)
        self.iters = torch.zeros(self.N, dtype=torch.int32)

    plan_groups = PlanBatch.plan_groups


KEYS, ROWS = ("p_grid", "p_load", "p_pv"), ("temp_in_opt", "solve_counter")


def _plan_worker(rank, world, port, n, q):
    from dragg_amd.aggregator import DeviceAggregator
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    homes = [{"name": f"h{i}"} for i in range(n)]
    agg = DeviceAggregator(homes, None, None, None, 0, 2, rank=rank, world=world, device=torch.device("cpu"),
                           batch_cls=ShardBatch)
    q.put((rank, [x.numpy() for x in agg.plan(KEYS, ROWS)]))
    dist.destroy_process_group()


def test_plan_over_two_ranks_equals_the_single_rank_result():
    from dragg_amd.aggregator import DeviceAggregator
    n, world = 37, 2
    homes = [{"name": f"h{i}"} for i in range(n)]
    one = [x.numpy() for x in DeviceAggregator(homes, None, None, None, 0, 2, device=torch.device("cpu"),
                                               batch_cls=ShardBatch).plan(KEYS, ROWS)]
    assert one[0].shape == (1, 3, ShardBatch.H) and one[1].max() > n // 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_plan_worker, args=(r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=120) for _ in procs), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    for rank, (curve, count, stats) in res:
        assert np.array_equal(count, one[1]), rank
        assert np.all(np.abs(curve - one[0]) <= 1e-12 * 50.0 * np.maximum(one[1], 1)), rank
        assert np.array_equal(stats[..., 0], one[2][..., 0]), rank
        assert np.all(np.abs(stats[..., 1] - one[2][..., 1]) <= 1e-12 * 50.0 * np.maximum(one[2][..., 0], 1)), rank
        assert np.array_equal(stats[..., 2:], one[2][..., 2:]), rank


def test_runner_rl_plan_and_rl_vector_plumbing(tmp_path):
    from dragg_amd.rl import DeviceVectorEnv
    from dragg_amd.runner import Aggregator
    from tests.test_rl import _rl_config
    from tests.test_runner import _synthetic_data
    data = tmp_path / "data"
    data.mkdir()
    _synthetic_data(str(data))
    _rl_config(data, dict(n=5, batt=1, pv=1, pvb=1, start="2015-01-01 00", end="2015-01-01 02", dt=4, horizon=1,
                          action_horizon=1, seed=3))
    a = Aggregator(data_dir=str(data), outputs_dir=str(tmp_path / "outputs"), device=torch.device("cpu"), batch_cls=PlanBatch)
    a.get_homes()
    env = a.rl_vector(2, device_env=True, plan_keys=("p_grid",))
    assert isinstance(env, DeviceVectorEnv) and env.plan_key_names == ["p_grid"]
    assert tuple(env.reset()["plan"].shape) == (2, 1, PlanBatch.H)
    assert "plan" not in a.rl_vector(2, device_env=True).reset()
    with pytest.raises(ValueError, match="device_env"):
        a.rl_vector(2, plan_keys=("p_grid",))
    # rl_plan / rl_sweep_plan hand the device aggregator's tensors to the host (the live community without its
    # group axis); a refusal passes through
    import types

    def refuse(keys, rows=()):
        raise ValueError("sweep_plan: no sweep of the live state is held")
    three = (torch.arange(8.0, dtype=torch.float64).view(1, 2, 4), torch.ones((1, 2, 4), dtype=torch.int32),
             torch.zeros((1, 0, 4), dtype=torch.float64))
    a.dev = types.SimpleNamespace(plan=lambda keys, rows=(): three, sweep_plan=refuse)
    curve, count, stats = a.rl_plan(("p_grid", "p_load"))
    assert isinstance(curve, np.ndarray) and curve.shape == (2, 4) and count.dtype == np.int32 and stats.shape == (0, 4)
    assert curve.tolist() == three[0][0].tolist()
    with pytest.raises(ValueError, match="held"):
        a.rl_sweep_plan()
    a.dev.sweep_plan = lambda keys, rows=(): tuple(x.repeat(3, 1, 1) for x in three)
    assert a.rl_sweep_plan(("p_grid", "p_load"))[0].shape == (3, 2, 4)
    for name in ("rl_plan", "rl_sweep_plan"):
        doc = getattr(Aggregator, name).__doc__
        assert "open-loop" in doc.lower().replace("open loop", "open-loop") and "rl_forecast" in doc
