"""Lookahead sweeps on the GPU: dragg_mpc_select_paths alone on synthetic sums against its numpy restatement
(`vector.select_paths_reference`) and against dragg_mpc_select_groups, its argument checks,
`VectorAggregator.sweep(steps=K)` and the commit from its held first step against twin aggregators that step the
ordinary way, and `rl.DeviceVectorEnv.step_swept(lookahead=K)` in a closed loop against `rl.VectorEnv`, bit for
bit.  Community: tests/test_gpu_vector.py's (16 homes of all four types, H = 24, April)."""
import numpy as np
import pytest
import torch

from dragg_amd import _lib as L
from tests.test_gpu_env import SEEDS, STARTS, _bits, _cfg, _pair, _same_obs, _same_state
from tests.test_gpu_vector import community                       # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

NB = 3                                  # homes per group of the synthetic dims (the kernel reads n_homes % E only)


def _dims(E, n_homes=None):
    return L.Dims(n_homes=NB * E if n_homes is None else n_homes, horizon=4, sub_steps=6, dt=1,
                  n_groups=E if E > 1 else 0)


def _case(E, C, K, P, T, seed):
    """Random rollouts with every special case the contract names: `ran` cycling through -1, 0, 1, T - 2, T - 1, T;
    NaN loads before and after the steps an episode has left; an episode whose candidates are all NaN; an episode
    whose candidates all tie on the score (the price, then the index decides)."""
    rng = np.random.default_rng(seed)
    a = {"sums": rng.uniform(0.0, 40.0, (K, C * E, 3)), "tracked": rng.uniform(0.0, 40.0, (E, P)),
         "target": rng.uniform(5.0, 30.0, E), "weights": rng.uniform(0.1, 1.0, K),
         "prices": rng.choice([-0.5, -0.25, 0.25, 0.5], (C * E, 2)),
         "ran": np.resize(np.array([1, 0, -1, T - 2, T - 1, T], dtype=np.int32), E)}
    if K == 1:
        a["weights"][:] = 1.0
    nan = rng.random((K, C * E)) < 0.08
    a["sums"][..., 0][nan] = np.nan
    if E > 4:
        a["sums"][0, np.arange(C) * E + 4, 0] = np.nan               # episode 4 (ran T - 1): no candidate valid
    tie = 1 if E > 1 else 0                                          # this episode's candidates are all one path
    for c in range(C):
        a["sums"][:, c * E + tie] = a["sums"][:, tie]
        a["sums"][:, c * E + tie, 0] = np.nan_to_num(a["sums"][:, tie, 0], nan=11.0)
        a["prices"][c * E + tie, 0] = (0.5, -0.25, 0.25)[c] if c < 3 else 0.5
    return a


def _call(gpu, E, C, T, a, with_score=True, dims=None, **over):
    """The entry point on device copies of `a` -> (rc, choice, score, the device tensors)."""
    t = {k: torch.as_tensor(v).to(gpu) for k, v in a.items()}
    K, P = a["sums"].shape[0], a["tracked"].shape[1]
    choice = torch.full((E,), 12345, dtype=torch.int32, device=gpu)
    score = torch.full((C * E,), 7.5, dtype=torch.float64, device=gpu)
    kw = dict(steps=K, num_timesteps=T, prev_timesteps=P, fresh_load=0.5 * 37.3, sums=L.ptr(t["sums"]),
              ran=L.ptr(t["ran"]), tracked=L.ptr(t["tracked"]), target=L.ptr(t["target"]), weights=L.ptr(t["weights"]),
              prices=L.ptr(t["prices"]), n_rp=a["prices"].shape[1], choice=L.ptr(choice),
              score=L.ptr(score) if with_score else None)
    copies = over.pop("copies", C)
    kw.update(over)
    p = None if over.get("null_p") else L.Paths(**{k: v for k, v in kw.items() if k != "null_p"})
    rc = L.load().dragg_mpc_select_paths(dims or _dims(E), copies, p, L.stream_ptr(None, gpu))
    torch.cuda.synchronize()
    return rc, choice.cpu().numpy(), score.cpu().numpy(), t


# ------------------------------------------------------------------ the kernel alone
@pytest.mark.parametrize("P", [1, 7, 8, 9, 12, 128])
@pytest.mark.parametrize("E,C,K", [(1, 1, 1), (5, 3, 2), (70, 65, 5), (4, 3, 9)])
def test_select_paths_alone_equals_the_restatement(gpu, E, C, K, P):
    from dragg_amd.vector import select_paths_reference
    T = K + 3
    a = _case(E, C, K, P, T, seed=1000 * P + 10 * E + K)
    want, want_score = select_paths_reference(a["sums"], a["ran"], a["tracked"], a["target"], a["weights"], a["prices"],
                                              T, 37.3)
    rc, choice, score, t = _call(gpu, E, C, T, a)
    assert rc == 0
    assert choice.tolist() == want.tolist()
    assert np.array_equal(score.view(np.int64), want_score.view(np.int64))
    for k, v in a.items():                                       # the inputs are only read
        assert np.array_equal(t[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k
    rc, again, untouched, _ = _call(gpu, E, C, T, a, with_score=False)
    assert rc == 0 and again.tolist() == want.tolist() and set(untouched.tolist()) == {7.5}
    # what the case was built to hold
    k_e = [min(K, T - r) if 0 <= r < T else 0 for r in a["ran"].tolist()]
    for e in range(E):
        sc = want_score[np.arange(C) * E + e]
        if k_e[e] == 0:
            assert want[e] == -1 and np.isnan(sc).all()
        else:
            ok = [c for c in range(C) if not np.isnan(a["sums"][:k_e[e], c * E + e, 0]).any()]
            assert [c for c in range(C) if not np.isnan(sc[c])] == ok and (want[e] in ok if ok else want[e] == -1)
    if E > 4:
        assert want[4] == -1 and k_e[4] == 1
    if E > 1:
        assert k_e[1] == K and want[1] == (1 if C >= 3 else 0) and len(set(want_score[np.arange(C) * E + 1])) == 1
    if (E, K) == (4, 9):
        assert k_e == [9, 9, 0, 2]                               # (P < 8: the window is all rollout loads by the end)


def test_one_step_choice_equals_select_groups(gpu):
    E, C, T = 70, 65, 5
    a = _case(E, C, 1, 12, T, seed=3)
    a["ran"] = np.resize(np.array([0, 1, T - 1], dtype=np.int32), E)
    rc, choice, _, t = _call(gpu, E, C, T, a)
    old = torch.full((E,), 12345, dtype=torch.int32, device=gpu)
    rc2 = L.load().dragg_mpc_select_groups(_dims(E), C, L.ptr(t["sums"]), L.ptr(t["target"]), L.ptr(t["prices"]), 2,
                                           L.ptr(old), L.stream_ptr(None, gpu))
    torch.cuda.synchronize()
    assert rc == rc2 == 0 and choice.tolist() == old.cpu().tolist()
    assert -1 in choice.tolist() and len(set(choice.tolist())) > 10


def test_select_paths_refuses_bad_arguments(gpu):
    E, C, K, P, T = 5, 3, 2, 12, 5
    a = _case(E, C, K, P, T, seed=4)

    def untouched(res):
        rc, choice, score, _ = res
        return rc == -1 and set(choice.tolist()) == {12345} and set(score.tolist()) == {7.5}
    assert _call(gpu, E, C, T, a)[0] == 0
    assert untouched(_call(gpu, E, C, T, a, null_p=True))
    for k in ("sums", "ran", "tracked", "target", "weights", "prices", "choice"):
        assert untouched(_call(gpu, E, C, T, a, **{k: None})), k
    for bad in (dict(steps=0), dict(prev_timesteps=0), dict(prev_timesteps=L.ENV_PREV_MAX + 1), dict(num_timesteps=0),
                dict(n_rp=0), dict(copies=0)):
        assert untouched(_call(gpu, E, C, T, a, **bad)), bad
    assert untouched(_call(gpu, E, C, T, a, dims=_dims(E, n_homes=NB * E + 1)))
    assert untouched(_call(gpu, E, C, T, a, dims=_dims(E, n_homes=-NB * E)))
    # an empty community has no step to choose
    rc, choice, score, _ = _call(gpu, E, C, T, a, dims=_dims(E, n_homes=0))
    assert rc == 0 and set(choice.tolist()) == {-1} and np.isnan(score).all()


# ------------------------------------------------------------------ rollouts and the held first step
T6, CANDS = 6, [[0.02, -0.02, 0.0], [0.01, 0.0, -0.01], [0.0, 0.03, -0.03], [0.0, 0.01, 0.02]]
FIRST = [0.0, 0.01, -0.01, 0.0]


def _prepared(community):
    """E = 4, T = 6: episode 2 at clock T - 2 (a masked run of four steps), episode 3 parked, the others fresh."""
    from dragg_amd.vector import VectorAggregator
    homes, (oat, ghi, tou) = community
    va = VectorAggregator(homes, oat, ghi, tou, 4, list(SEEDS), list(STARTS), T6)
    va.park([0, 1, 3])
    for _ in range(4):
        va.step(FIRST)
    va.resume([0, 1])
    return va


def _live(va):
    return [x.clone() for x in (va.batch.vals, va.batch.fc_store, va.clocks, va.hist, va.status_hist, va.path_hist,
                                va.agg_hist)]


def test_rollouts_equal_twins_stepped_on(gpu, community):
    E, C, K = 4, 3, 3
    va = _prepared(community)
    assert va.clocks_host() == [0, 0, T6 - 2, 0]
    cands = torch.tensor(CANDS, dtype=torch.float64, device=gpu)
    before = _live(va)
    paths = va.sweep(cands, steps=K)
    assert tuple(paths.shape) == (E, C, K, 3) and paths.is_cuda
    assert va.sweep_steps.dtype == torch.int32 and va.sweep_steps.cpu().tolist() == [3, 3, 2, 0]
    for x, y in zip(before, _live(va)):
        assert torch.equal(_bits(x), _bits(y))
    assert not bool(torch.isnan(paths[:3]).any())
    for c in range(C):
        twin = _prepared(community)
        for j in range(K):
            got = twin.step(cands[:, c].contiguous())
            for e in range(E):
                if j < [3, 3, 2, 0][e]:
                    assert torch.equal(_bits(paths[e, c, j]), _bits(got[e])), (e, c, j)
    assert torch.equal(_bits(paths[2, :, 2]), _bits(paths[2, :, 1]))                 # rows j >= k_e repeat row k_e - 1
    assert torch.equal(_bits(paths[3, :, 1]), _bits(paths[3, :, 0])) and torch.equal(_bits(paths[3, :, 2]), _bits(paths[3, :, 0]))
    assert torch.equal(_bits(paths[:, :, 0]), _bits(va.sweep(cands)))                # step 0 is the one-step sweep


def test_commit_adopts_the_held_first_step(gpu, community):
    C, K = 3, 3
    va, twin = _prepared(community), _prepared(community)
    cands = torch.tensor(CANDS, dtype=torch.float64, device=gpu)
    va.sweep(cands, steps=K)
    held = va._hold["src"]
    assert held is va._held[C] and held is not va._sweep_batches[C]
    keys = ("vals", "fc_store", "status", "iters", "obj", "relax_obj", "int_path")
    ptrs = [getattr(held, k).data_ptr() for k in keys]
    choice = torch.tensor([2, 0, 1, 1], dtype=torch.int32, device=gpu)
    got = va.commit(choice)
    assert va.adopted.cpu().tolist() == [True, True, True, False]
    want = twin.step(torch.tensor([CANDS[e][int(c)] for e, c in enumerate([2, 0, 1, 1])], dtype=torch.float64, device=gpu))
    assert torch.equal(_bits(got), _bits(want)) and va.clocks_host() == twin.clocks_host() == [1, 1, T6 - 1, 0]
    for x, y, k in ((va.batch.vals, twin.batch.vals, "vals"), (va.batch.fc_store, twin.batch.fc_store, "fc"),
                    (va.hist, twin.hist, "hist"), (va.status_hist, twin.status_hist, "status_hist"),
                    (va.path_hist, twin.path_hist, "path_hist"), (va.agg_hist, twin.agg_hist, "agg_hist")):
        assert torch.equal(_bits(x), _bits(y)), k
    assert int((va.status_hist[0].view(4, -1)[:2] == L.ST_OPTIMAL).sum()) > 0
    va.sweep(cands, steps=K)                                     # a second sweep at the same C: the same buffers
    assert va._hold["src"] is held and [getattr(held, k).data_ptr() for k in keys] == ptrs
    assert va.sweep_steps.cpu().tolist() == [3, 3, 1, 0]


# ------------------------------------------------------------------ closed loop, host against device
def test_closed_loop_with_lookahead_equals_the_host_environment(gpu, community):
    """E = 4, T = 5, C = 3, lookahead 3 with weights 1, 1/2, 1/4; episode 3 is parked during step 1 and finishes a
    step late.  Observations, choices, scores and the full state bit-identical at every step; at least half of the
    home-steps optimal, so the run is not all fallbacks."""
    from dragg_amd.rl import SweepAgent
    T, w = 5, [1, .5, .25]
    host, dev = _pair(community, T)
    agent = SweepAgent(_cfg(), n_candidates=3, lookahead=3, discount=0.5)
    assert agent.weights() == w
    obs_h, obs_d = host.reset(), dev.reset()
    k = 0
    while not host.done().all():
        if k == 1:
            host.park([3])
            dev.park([3])
        if k == 2:
            host.resume([3])
            dev.resume([3])
        obs_h, done_h = host.step_swept(agent.act_vector(obs_h), lookahead=3, weights=w)
        obs_d, done_d = dev.step_swept(agent.act_device(obs_d), lookahead=3, weights=w)
        assert dev.choice.is_cuda and dev.choice.dtype == torch.int32 and dev.scores.is_cuda
        assert host.choice.tolist() == dev.choice.cpu().tolist(), k
        assert torch.equal(_bits(torch.as_tensor(host.scores)), _bits(dev.scores.cpu())), k
        assert done_h.tolist() == done_d.cpu().tolist()
        _same_obs(obs_h, obs_d, k)
        _same_state(host, dev, k)
        if k == 1:
            assert host.choice[3] == -1 and np.isnan(host.scores[3]).all() and not np.isnan(host.scores[:3]).any()
        k += 1
        assert k <= T + 1
    assert k == T + 1 and host.va.clocks_host() == [T] * 4
    st = dev.va.status_hist
    n_opt = int((st == L.ST_OPTIMAL).sum())
    print("optimal home-steps of the lookahead closed loop:", n_opt, "of", st.numel())
    assert n_opt * 2 >= st.numel()


def test_lookahead_step_makes_no_host_round_trip(gpu, community):
    from dragg_amd.rl import DeviceVectorEnv, SweepAgent
    from dragg_amd.vector import VectorAggregator
    homes, (oat, ghi, tou) = community
    va = VectorAggregator(homes, oat, ghi, tou, 4, list(SEEDS), list(STARTS), 3)
    env = DeviceVectorEnv(va, _cfg())
    sw = SweepAgent(_cfg(), n_candidates=3, lookahead=2)
    obs = env.reset()
    cands = sw.act_device(obs)
    obs, _ = env.step_swept(cands, lookahead=2, weights=sw.weights())    # (the first call: code objects, buffers,
    torch.cuda.synchronize()                                             #  the weights' upload)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        obs, done = env.step_swept(sw.act_device(obs), lookahead=2, weights=sw.weights())    # (cached)
        obs, done = env.step_swept(sw.act_device(obs), lookahead=2)                          # (ones, made on the device)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert va.clocks_host() == [3] * 4 and bool(done.all()) and int(env.choice.min()) >= 0
    assert va.sweep_steps.cpu().tolist() == [1] * 4 and not bool(torch.isnan(env.scores).any())
