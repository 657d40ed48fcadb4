#!/usr/bin/env python3
"""Vectorised episodes against the loop they replace: E episodes of an Nb-home community (defaults E = 512,
Nb = 20, H = 24: the shape of BASELINE.json configs[0]), each with its own season-noise seed, start index
and reward price, stepped

* together, as one grouped batch (`dragg_amd.vector.VectorAggregator.step`: publish the prices, one
  dragg_mpc_step_episodes, the per-episode sums, the history rows), and
* one after another, each episode a fresh `DeviceAggregator` run with that seed, start index and price
  trajectory (`set_reward_price`, `run_iteration`, `collect_data`): the existing path on the same build.

Both run `--warmup` untimed steps and then `--steps` steps timed with HIP events on the stream (the events
of the sequential runs are summed over the episodes; constructing the aggregators is not timed).  The
per-episode sums of the last step must be equal bit for bit, or the tool fails.  Prints one JSON line and
writes it to --out.  Needs a GPU (there is no fallback).

    python tools/vector_bench.py --out profiles/r08/vector/vector_line.json
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=512)
    ap.add_argument("--homes", type=int, default=20)
    ap.add_argument("--horizon-hours", type=int, default=6)
    ap.add_argument("--dt", type=int, default=4)
    ap.add_argument("--month", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--price", choices=("scalar", "smooth"), default="scalar",
                    help="each episode's reward price: one value per step (a SetpointAgent's action), or that value "
                         "on a list that changes at every stage (RL-priced chains: the later launches)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("vector_bench.py: no GPU (a timing needs one)")
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.community import reference_completable, synthetic_homes, synthetic_weather
    from dragg_amd.vector import VectorAggregator

    E, Nb, dt, W, T = args.episodes, args.homes, args.dt, args.warmup, args.steps
    H = args.horizon_hours * dt
    total = W + T
    max_start = 7
    sim_hours = math.ceil((total + max_start + 1) / dt)
    days = math.ceil((sim_hours + args.horizon_hours + 2) / 24) + 1
    homes = synthetic_homes(Nb, seed=12, days=days, dt=dt, horizon_hours=args.horizon_hours)
    oat, ghi, tou = synthetic_weather(days, dt, sim_hours, seed=3, month=args.month)
    homes, _ = reference_completable(homes, oat, ghi, tou, seed=12)
    seeds = [12 + e for e in range(E)]
    starts = [e % (max_start + 1) for e in range(E)]
    rng = np.random.default_rng(5)
    act = rng.uniform(-0.02, 0.02, (total, E))                      # $/kWh, per step and episode
    shape = -0.03 * np.cos(np.arange(H) / 3.0) if args.price == "smooth" else np.zeros(1)
    prices = act[:, :, None] + shape[None, None, :]                 # [total][E][n]

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    # ---- together
    va = VectorAggregator(homes, oat, ghi, tou, E, seeds, starts, total)
    P = torch.as_tensor(prices, dtype=torch.float64, device=va.device)
    for k in range(W):
        va.step(P[k])
    torch.cuda.synchronize()
    e0, e1 = events()
    e0.record()
    for k in range(W, total):
        last = va.step(P[k])
    e1.record()
    torch.cuda.synchronize()
    vec_ms = e0.elapsed_time(e1)
    vec_last = last.cpu()
    counts = va.status_counts()
    paths = {k: int(sum(v)) for k, v in va.approx_counts().items()}
    del va
    torch.cuda.empty_cache()

    # ---- one after another
    seq_ms, seq_last = 0.0, []
    for e in range(E):
        agg = DeviceAggregator(homes, oat, ghi, tou, starts[e], total, reward_price=prices[0, e], seed=seeds[e])
        for k in range(W):
            agg.set_reward_price(P[k, e])
            agg.run_iteration()
            agg.collect_data()
        torch.cuda.synchronize()
        e0, e1 = events()
        e0.record()
        for k in range(W, total):
            agg.set_reward_price(P[k, e])
            agg.run_iteration()
            s = agg.collect_data()
        e1.record()
        torch.cuda.synchronize()
        seq_ms += e0.elapsed_time(e1)
        seq_last.append(s.cpu().clone())
        del agg
    seq_last = torch.stack(seq_last)
    if not torch.equal(vec_last.view(torch.int64), seq_last.view(torch.int64)):
        raise SystemExit("vector_bench.py: the episodes' sums differ from the single runs'")

    line = {
        "metric": "episode-steps per second (E episodes x steps, per-episode sums and history kept)",
        "config": {"baseline_config": "BASELINE.json configs[0] shape", "episodes": E, "homes": Nb, "horizon": H,
                   "dt": dt, "month": args.month, "steps": T, "warmup": W, "price": args.price, "gpus": 1,
                   "device": torch.cuda.get_device_name(0)},
        "vectorised_ms": round(vec_ms, 3),
        "sequential_ms": round(seq_ms, 3),
        "vectorised_ms_per_step": round(vec_ms / T, 4),
        "sequential_ms_per_episode_step": round(seq_ms / (T * E), 4),
        "vectorised_episode_steps_per_s": round(E * T / vec_ms * 1e3, 1),
        "sequential_episode_steps_per_s": round(E * T / seq_ms * 1e3, 1),
        "ratio": round(seq_ms / vec_ms, 3),
        "sums_bit_identical": True,
        "status_counts": counts,
        "solve_paths": paths,
        "note": "HIP events around the timed steps on the stream (host launch gaps included); the sequential "
                "runs' events summed over the episodes, their construction untimed",
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
