#!/usr/bin/env python3
"""Lookahead sweeps in the device-resident vector environment against the same rollouts done one candidate at a time.

The community of tools/env_bench.py (Nb = 20, H = 24, July, one price value per step) as E = 8, 64 and 512
episodes with C = 8 candidate prices per episode, stepped in closed loops:

  swept_k1     `DeviceVectorEnv.step_swept(candidates)`: the one-step sweep (this build and its parent);
  swept_kK     `DeviceVectorEnv.step_swept(candidates, lookahead=K)`, K = 2 and 4: K grouped steps of C * E groups,
               one scoring kernel, the first step adopted (builds that have `lookahead` only);
  serial_kK    K = 1, 2 and 4, written with calls every build has: for each candidate the live E-group batch's
               `vals` / `fc_store` are saved, the batch is stepped K times under that price (`MPCBatch.step_episodes`,
               `aggregate_groups`) and restored -- C * K grouped steps of E groups --, the K-step paths are scored
               by a few torch ops on the device (the sum over the steps of |load - setpoint|, the setpoint held),
               and the chosen price is solved again by `DeviceVectorEnv.step`.

Every repetition times --steps environment steps of each loop after a reset of all episodes and --warmup steps
(untimed), between two HIP events on the stream, the loops in an order rotated by one every repetition; medians,
minima, maxima and every repetition are reported.  On a build with `lookahead`, `dragg_mpc_select_paths` alone
(`VectorAggregator.select_paths` on the buffers of the last sweep, --select-calls calls between two events) is timed
too.  Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/lookahead_bench.py --out profiles/r14/lookahead/lookahead_line.json
    python tools/lookahead_bench.py --combine parent_a.json branch.json parent_b.json --out bench_parent_vs_branch.json

--combine puts a branch line beside two lines of its parent (the same command, run before and after it): the
ratios swept / serial per (E, K), and whether the branch's one-step sweep lies inside the parent's own repetitions.
"""
import argparse
import inspect
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "reps": [round(x, 4) for x in xs]}


def combine(paths, out):
    a, b, c = (json.load(open(p)) for p in paths)
    rows = []
    for ra, rb, rc in zip(a["rows"], b["rows"], c["rows"]):
        pa, pb = ra["ms_per_step"], rc["ms_per_step"]
        br = rb["ms_per_step"]
        reps = pa["swept_k1"]["reps"] + pb["swept_k1"]["reps"]
        row = {"E": rb["E"], "C": rb["C"],
               "swept_k1_ms": {"parent_first": pa["swept_k1"], "branch": br["swept_k1"], "parent_second": pb["swept_k1"]},
               "swept_k1_branch_over_parent": round(2 * br["swept_k1"]["median"] /
                                                    (pa["swept_k1"]["median"] + pb["swept_k1"]["median"]), 4),
               "swept_k1_parent_second_over_first": round(pb["swept_k1"]["median"] / pa["swept_k1"]["median"], 4),
               "swept_k1_branch_inside_the_parents_repetitions": bool(min(reps) <= br["swept_k1"]["median"] <= max(reps)),
               "serial_ms": {k: {"parent_first": pa[k], "branch": br[k], "parent_second": pb[k]}
                             for k in sorted(br) if k.startswith("serial")},
               "swept_ms_branch": {k: br[k] for k in sorted(br) if k.startswith("swept")},
               "swept_over_serial": {k[6:]: round(br[k]["median"] / br["serial" + k[5:]]["median"], 4)
                                     for k in sorted(br) if k.startswith("swept") and "serial" + k[5:] in br},
               "select_paths_alone_us": rb.get("select_paths_alone_us")}
        rows.append(row)
    line = {"metric": b["metric"], "config": b["config"], "rows": rows,
            "note": "parent_first and parent_second: the parent commit's build, run by the same command before and "
                    "after the branch's in one session; swept_over_serial from the branch's own run"}
    s = json.dumps(line)
    print(s)
    with open(out, "w") as f:
        f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--lookahead", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--homes", type=int, default=20)
    ap.add_argument("--horizon-hours", type=int, default=6)
    ap.add_argument("--dt", type=int, default=4)
    ap.add_argument("--month", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--select-calls", type=int, default=200)
    ap.add_argument("--prev-timesteps", type=int, default=12)
    ap.add_argument("--combine", nargs=3, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.combine:
        return combine(args.combine, args.out)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lookahead_bench.py: no GPU (a timing needs one)")
    from dragg_amd.community import reference_completable, synthetic_homes, synthetic_weather
    from dragg_amd.rl import DeviceVectorEnv, SweepAgent
    from dragg_amd.vector import VectorAggregator
    has_lookahead = "steps" in inspect.signature(VectorAggregator.sweep).parameters

    Nb, dt, W, S, C = args.homes, args.dt, args.warmup, args.steps, args.candidates
    H = args.horizon_hours * dt
    Ks = sorted(set(args.lookahead))
    total, max_start = W + S + max(Ks), 7                    # (every rollout step of every timed step exists)
    sim_hours = math.ceil((total + max_start + 1) / dt)
    days = math.ceil((sim_hours + args.horizon_hours + 2) / 24) + 1
    homes = synthetic_homes(Nb, seed=12, days=days, dt=dt, horizon_hours=args.horizon_hours)
    oat, ghi, tou = synthetic_weather(days, dt, sim_hours, seed=3, month=args.month)
    homes, _ = reference_completable(homes, oat, ghi, tou, seed=12)
    cfg = {"agg": {"rl": {"prev_timesteps": args.prev_timesteps}},
           "rl": {"utility": {"action_space": [-2.0, 2.0], "action_scale": 100.0}}}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end)

    rows = []
    for E in args.episodes:
        seeds, starts = [12 + e for e in range(E)], [e % (max_start + 1) for e in range(E)]
        va = VectorAggregator(homes, oat, ghi, tou, E, seeds, starts, total)
        env = DeviceVectorEnv(va, cfg)
        agent = SweepAgent(cfg, n_candidates=C)
        cands = agent.act_device(env.reset())                # [E][C], the same every step
        b = va.batch
        snap = (torch.empty_like(b.vals), torch.empty_like(b.fc_store))
        paths = torch.zeros((max(Ks), C, E), dtype=torch.float64, device=va.device)
        rows_e = torch.arange(E, device=va.device)

        def swept(K):
            def step():
                if K == 1:
                    env.step_swept(cands)
                else:
                    env.step_swept(cands, lookahead=K)
            return step

        def serial(K):
            def step():
                snap[0].copy_(b.vals)
                snap[1].copy_(b.fc_store)
                for c in range(C):
                    b.set_reward_price(cands[:, c:c + 1].contiguous())
                    for j in range(K):
                        b.step_episodes(va.seeds, va.starts, va.clocks + j)
                        paths[j, c].copy_(b.aggregate_groups()[:, 0])
                    b.vals.copy_(snap[0])
                    b.fc_store.copy_(snap[1])
                score = (paths[:K] - env.state.obs[3]).abs().sum(0)              # [C][E]
                env.step(cands[rows_e, score.argmin(0)])
            return step

        loops = {f"serial_k{K}": serial(K) for K in Ks}
        loops.update({f"swept_k{K}": swept(K) for K in Ks if K == 1 or has_lookahead})
        times = {k: [] for k in loops}
        names = sorted(loops)
        for r in range(args.reps):
            for name in names[r % len(names):] + names[:r % len(names)]:
                env.reset()
                for _ in range(W):
                    loops[name]()
                times[name].append(timed(lambda: [loops[name]() for _ in range(S)]) / S)
        row = {"E": E, "C": C, "ms_per_step": {k: stats(v) for k, v in times.items()}}
        if has_lookahead:
            alone = {}
            for K in (k for k in Ks if k > 1):
                env.reset()
                p = va.sweep(cands, steps=K)
                w = torch.ones(K, dtype=torch.float64, device=va.device)

                def call():
                    va.select_paths(p, env.state.tracked, env.state.obs[3], cands, w, env.max_poss_load)
                call()
                alone[f"k{K}"] = round(min(timed(lambda: [call() for _ in range(args.select_calls)])
                                         for _ in range(3)) / args.select_calls * 1e3, 2)
            row["select_paths_alone_us"] = alone
            row["swept_over_serial"] = {f"k{K}": round(statistics.median(times[f"swept_k{K}"]) /
                                                       statistics.median(times[f"serial_k{K}"]), 4) for K in Ks}
        rows.append(row)
        del va, env, b, snap, loops
        torch.cuda.empty_cache()

    line = {"metric": "ms per environment step (candidates, rollouts, choice, the played step, observations) between "
                      "two HIP events, medians of repetitions in rotated order",
            "config": {"homes": Nb, "horizon": H, "dt": dt, "month": args.month, "candidates": C, "lookahead": Ks,
                       "steps": S, "warmup": W, "reps": args.reps, "prev_timesteps": args.prev_timesteps,
                       "price": "scalar", "has_lookahead": has_lookahead, "device": torch.cuda.get_device_name(0)},
            "rows": rows,
            "note": "swept: DeviceVectorEnv.step_swept; serial: per candidate save, K steps of the live batch, restore, "
                    "then the chosen price solved again; select_paths_alone_us: microseconds per back-to-back call "
                    "(launch-bound), the least of three windows"}
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
