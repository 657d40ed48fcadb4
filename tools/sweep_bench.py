#!/usr/bin/env python3
"""Price sweep against the loop it replaces, on the RL bench community (BASELINE.json configs[4], the
community of `bench.py --workload rl`): the responses to G candidate reward-price lists over
`--forecast-horizon` timesteps, once as one grouped launch per step (`DeviceAggregator.sweep`, what
`Aggregator.rl_sweep` runs) and once as G rollouts in sequence (`set_reward_price` + `forecast`, what G
`Aggregator.rl_forecast` calls run), both ending with the responses on the host.

The two are alternated `--reps` times after a warm-up of each (code objects, the replica batch and its
workspace are allocated there); a call is timed by the host clock around work that ends in the
device-to-host copy of its result.  The responses must be equal bit for bit, or the tool fails.
Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/sweep_bench.py --out profiles/r07/sweep/sweep_line.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--homes", type=int, default=10000)
    ap.add_argument("--horizon-hours", type=int, default=12)
    ap.add_argument("--dt", type=int, default=4)
    ap.add_argument("--month", type=int, default=7)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--forecast-horizon", type=int, default=1, help="rollout timesteps per candidate")
    ap.add_argument("--warmup", type=int, default=4, help="committed RL steps before the measurement")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sweep_bench.py: no GPU (a timing needs one)")
    import bench
    from dragg_amd.aggregator import DeviceAggregator

    G, fh = args.candidates, args.forecast_horizon
    args.steps = fh + 1                                   # (bench_community sizes the weather by warmup + steps)
    homes, oat, ghi, tou = bench.bench_community(args)
    homes, _ = bench.reference_completable(homes, oat, ghi, tou, seed=12)
    H = args.horizon_hours * args.dt
    shape = -0.03 * np.cos(np.arange(H) / 3.0)            # bench.py --rl-price smooth: a change at every stage
    live = np.random.default_rng(5).uniform(-0.02, 0.02, (args.warmup + 1, 1)) + shape[None, :]
    cands = np.linspace(-0.02, 0.02, G)[:, None] + shape[None, :]

    agg = DeviceAggregator(homes, oat, ghi, tou, 0, args.warmup + fh + 1, reward_price=[0.0], seed=12)
    for k in range(args.warmup):                          # the community mid-run, under RL prices
        agg.set_reward_price(live[k])
        agg.run_iteration()
        agg.collect_data()
    agg.set_reward_price(live[args.warmup])

    def loop():
        outs = []
        for p in cands:
            agg.set_reward_price(p)
            outs.append(agg.forecast(fh))
        agg.set_reward_price(live[args.warmup])
        return torch.stack(outs).cpu()

    def sweep():
        return agg.sweep(cands, fh).cpu()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()                                        # (ends in a device-to-host copy: synchronised)
        return out, (time.perf_counter() - t0) * 1e3

    ref, _ = timed(loop)
    got, _ = timed(sweep)
    if not torch.equal(ref, got):
        raise SystemExit("sweep_bench.py: the sweep's responses differ from the per-candidate forecasts")
    t_loop, t_sweep = [], []
    for _ in range(args.reps):
        t_loop.append(timed(loop)[1])
        t_sweep.append(timed(sweep)[1])
    rb = agg._sweep_batches[G]
    ws = rb.workspace.numel() * 8 if rb.workspace is not None else 0
    med_l, med_s = statistics.median(t_loop), statistics.median(t_sweep)
    line = {
        "metric": "ms per price-response curve (G candidates x forecast_horizon steps, responses on the host)",
        "config": {"baseline_config": "BASELINE.json configs[4]", "homes": len(homes), "horizon": H, "dt": args.dt,
                   "month": args.month, "candidates": G, "forecast_horizon": fh, "committed_steps": args.warmup,
                   "gpus": 1, "device": torch.cuda.get_device_name(0)},
        "sweep_ms": {"median": round(med_s, 3), "min": round(min(t_sweep), 3), "max": round(max(t_sweep), 3),
                     "reps": [round(x, 3) for x in t_sweep]},
        "forecast_loop_ms": {"median": round(med_l, 3), "min": round(min(t_loop), 3), "max": round(max(t_loop), 3),
                             "reps": [round(x, 3) for x in t_loop]},
        "speedup_median": round(med_l / med_s, 3),
        "responses_bit_identical": True,
        "sweep_counts": agg.sweep_counts,
        "replica_batch_bytes": {"workspace": ws, "vals": rb.vals.numel() * 8, "fc": rb.fc_store.numel() * 8},
        "note": "alternated loop / sweep after one warm-up call of each; host clock around a call that ends in "
                "the device-to-host copy of its [G][steps][3] result",
    }
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
