#!/usr/bin/env python3
"""What the episodes' EV fleet costs (dragg_mpc_ev_step_episodes, VectorAggregator(vehicles=True)), on one build.

(a) The episode launch against dragg_mpc_ev_step: tools/ev_bench.py's fleet (--fleet-homes 10,000 homes of which
    --share 0.3 carry a vehicle: 3,000 at H = 48, mid-run),
    --launches back-to-back launches between two device events, the entries alternated --rounds times in one
    process: the plain step, the episode entry with shared keys (every member of the episodes struct NULL) and
    the episode entry with the keys read from the device.  The three leave bit-identical state, or the tool fails.
(b) The environment step with and without vehicles: tools/env_bench.py's community (20 homes, H = 24, July), half
    of the homes with a vehicle, E = 8 / 64 / 512 episodes in a `rl.DeviceVectorEnv` under fixed prices; --steps
    steps after --warmup, wall clock between two `torch.cuda.synchronize()` calls, the two alternated and the order
    swapped every repetition.  The homes' hash arrays of the two must be bit-identical at the end, or the tool
    fails.  Beside the times: the launches a step with vehicles adds, as the code makes them (two of the library,
    six elementwise torch ops that publish the prices and file ev_agg_hist).

Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/ev_vector_bench.py --out profiles/r19/ev_vector/ev_vector_line.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs, nd=4):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd),
            "reps": [round(x, nd) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fleet-homes", type=int, default=10000)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--committed", type=int, default=4)
    ap.add_argument("--episodes", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--homes", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ev_vector_bench.py: no GPU (a timing needs one)")
    from dragg_amd.community import ev_sections, reference_completable, synthetic_homes, synthetic_weather
    from dragg_amd.ev import EVFleet
    from dragg_amd.rl import DeviceVectorEnv
    from dragg_amd.vector import VectorAggregator

    def bits(x):
        return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x

    # ---------------------------------------------------------------- (a) the launch
    dt, hh, days = 4, 12, 3
    homes = synthetic_homes(args.fleet_homes, seed=12, days=days, dt=dt, horizon_hours=hh, ev_share=args.share)
    _, _, tou = synthetic_weather(days, dt, 24, seed=3, month=7)
    f = EVFleet(homes, tou, 0, [0.0], day_offset=6 * dt)
    for t in range(args.committed):
        f.step(t)
    t_mid = args.committed
    snap = f.snapshot()
    starts = torch.zeros(1, dtype=torch.int32, device=f.device)
    clocks = torch.full((1,), t_mid, dtype=torch.int32, device=f.device)
    entries = {"ev_step": lambda: f.step(t_mid),
               "ev_step_episodes_shared_keys": lambda: f.step_episodes(None, None, t=t_mid),
               "ev_step_episodes_device_keys": lambda: f.step_episodes(starts, clocks)}

    def events_us(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        f.restore(snap)
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    states = {}
    for k, fn in entries.items():
        f.restore(snap)
        fn()
        torch.cuda.synchronize()
        states[k] = [bits(x).clone() for x in f.snapshot()]
    if not all(all(torch.equal(x, y) for x, y in zip(states["ev_step"], s)) for s in states.values()):
        raise SystemExit("ev_vector_bench.py: the episode entry and dragg_mpc_ev_step differ")
    us = {k: [] for k in entries}
    for _ in range(args.rounds):
        for k, fn in entries.items():
            us[k].append(events_us(fn, args.launches))
    launch = {k: stats(v, 2) for k, v in us.items()}
    launch["episodes_minus_step_us"] = round(statistics.median(us["ev_step_episodes_device_keys"]) -
                                             statistics.median(us["ev_step"]), 2)
    launch["spread_of_ev_step_us"] = round(max(us["ev_step"]) - min(us["ev_step"]), 2)
    M = f.M
    del f

    # ---------------------------------------------------------------- (b) the environment step
    Nb, hh, W, S = args.homes, 6, args.warmup, args.steps
    total, max_start = W + S, 7
    sim_hours = math.ceil((total + max_start + 1) / dt)
    days = math.ceil((sim_hours + hh + 2) / 24) + 1
    homes = synthetic_homes(Nb, seed=12, days=days, dt=dt, horizon_hours=hh)
    oat, ghi, tou = synthetic_weather(days, dt, sim_hours, seed=3, month=7)
    homes, _ = reference_completable(homes, oat, ghi, tou, seed=12)
    homes = [dict(h) for h in homes]
    for i, sec in ev_sections(len(homes), 0.5, dt, 9).items():
        homes[i]["ev"] = sec
    cfg = {"agg": {"rl": {"prev_timesteps": 12}}, "rl": {"utility": {"action_space": [-2.0, 2.0], "action_scale": 100.0}}}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rows = []
    for E in args.episodes:
        seeds, startl = [12 + e for e in range(E)], [e % (max_start + 1) for e in range(E)]
        envs = {}
        for name, kw in (("homes", {}), ("vehicles", dict(vehicles=True, day_offset=6 * dt))):
            envs[name] = DeviceVectorEnv(VectorAggregator(homes, oat, ghi, tou, E, seeds, startl, total, **kw), cfg)
        dev = envs["homes"].va.device
        fixed = torch.as_tensor(np.random.default_rng(5).uniform(-0.02, 0.02, (total, E)), dtype=torch.float64, device=dev)

        def run(env, lo, n):
            for k in range(lo, lo + n):
                env.step(fixed[k])

        times = {k: [] for k in envs}
        for r in range(args.reps):
            order = list(envs.items())
            if r % 2:
                order.reverse()
            for name, env in order:
                env.reset()
                run(env, 0, W)
                times[name].append(wall(lambda e=env: run(e, W, S)) / S)
        a, b = envs["homes"].va, envs["vehicles"].va
        if not (torch.equal(bits(a.batch.vals), bits(b.batch.vals)) and torch.equal(bits(a.hist), bits(b.hist))
                and torch.equal(bits(b.agg_hist), bits(a.agg_hist + b.ev_agg_hist))):
            raise SystemExit(f"ev_vector_bench.py: E = {E}: the homes differ with and without the vehicles")
        mh, mv = statistics.median(times["homes"]), statistics.median(times["vehicles"])
        rows.append({"E": E, "vehicles_per_episode": int(b.fleet.Mb), "step_ms_homes_only": stats(times["homes"]),
                     "step_ms_with_vehicles": stats(times["vehicles"]), "added_ms": round(mv - mh, 4),
                     "ratio": round(mv / mh, 4), "library_launches_added": 2,
                     "torch_elementwise_ops_added": 6, "homes_bit_identical": True})
        del envs, a, b
        torch.cuda.empty_cache()

    line = {"tool": "ev_vector_bench", "device": torch.cuda.get_device_name(0),
            "launch": {"vehicles": M, "horizon": 48, "launches": args.launches, "rounds": args.rounds, **launch},
            "environment": {"homes": Nb, "horizon": hh * dt, "steps": S, "warmup": W, "reps": args.reps, "rows": rows},
            "note": "launch: us per launch between two device events over back-to-back launches, the entries "
                    "alternated; environment: ms per DeviceVectorEnv.step under fixed prices, wall clock between two "
                    "device synchronisations, order swapped every repetition; library_launches_added: the episode "
                    "step and aggregate_onto; torch_elementwise_ops_added: the fleet's copy of the price rows, the "
                    "row index (clamp, cast) and the filing of ev_agg_hist (gather, where, scatter)"}
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(s + "\n")


if __name__ == "__main__":
    main()
