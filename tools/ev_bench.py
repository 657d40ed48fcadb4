#!/usr/bin/env python3
"""What an EV fleet costs beside the homes (dragg_mpc_ev_step, dragg_mpc_ev_aggregate), on one build.

The community of bench.py's size: --homes homes (10,000) at H = 48 (dt = 4, a 12 h horizon, July), of which
--share (0.3: 3,000) carry a vehicle (community.synthetic_homes(ev_share=...)).

(a) The EV launches alone, mid-run (after --committed steps of the fleet): --launches back-to-back
    dragg_mpc_ev_step launches between two device events, and as many dragg_mpc_ev_aggregate launches; per launch
    and per vehicle.  Beside them the launch's algorithmic bytes (params and the state row read, vals and fc
    written) over the 8,000 GB/s HBM figure of bench.py's roofline: the least possible time.  The launch is
    latency-bound (a chain of H dependent wave scans), so it lies far above that.
(b) The step with and without the fleet: two DeviceAggregators on the same community, `run_iteration` +
    `collect_data`, --steps steps after --warmup, wall clock between two `torch.cuda.synchronize()` calls, the two
    alternated and the order swapped every repetition; medians, every repetition kept.  The homes' hash arrays of
    the two must be bit-identical at the end, or the tool fails.

--only-launches N: nothing but N EV step launches after the warm-up (for a kernel trace in a run of its own).
Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/ev_bench.py --out profiles/r17/ev/ev_line.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0


def stats(xs, nd=4):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd),
            "reps": [round(x, nd) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--homes", type=int, default=10000)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--committed", type=int, default=4)
    ap.add_argument("--only-launches", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ev_bench.py: no GPU (a timing needs one)")
    from dragg_amd import _lib as L
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.community import synthetic_homes, synthetic_weather
    from dragg_amd.ev import EVFleet

    dt, hh, days = 4, 12, 3
    H = hh * dt
    homes = synthetic_homes(args.homes, seed=12, days=days, dt=dt, horizon_hours=hh, ev_share=args.share)
    oat, ghi, tou = synthetic_weather(days, dt, 24, seed=3, month=7)
    total = args.reps * (args.warmup + args.steps) + 1
    day_offset = 6 * dt                                      # 06:00: departures inside the horizon from the start

    def fleet():
        return EVFleet(homes, tou, 0, [0.0], day_offset=day_offset)

    def events_us(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    f = fleet()
    for t in range(args.committed):
        f.step(t)
    t_mid = args.committed
    if args.only_launches:
        for _ in range(args.only_launches):
            f.step(t_mid)
        torch.cuda.synchronize()
        print(json.dumps({"only_launches": args.only_launches, "vehicles": f.M, "horizon": H}))
        return
    snap = f.snapshot()

    def one_step():
        f.step(t_mid)
    step_us = events_us(one_step, args.launches)
    f.restore(snap)
    agg_us = events_us(lambda: f.aggregate(), args.launches)
    torch.cuda.synchronize()
    n_opt = int((f.status == L.EV_OPTIMAL).sum())
    M = f.M
    bytes_alg = M * 8 * (L.NEVP + 1 + L.NEVV + L.NEVK * H + 1) + M * 4 + 8 * 2 * H
    floor_us = bytes_alg / (HBM_GBS * 1e9) * 1e6

    def run(agg, n):
        for _ in range(n):
            agg.run_iteration()
            agg.collect_data()

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    kw = dict(reward_price=[0.0], seed=12, keep_history=False)
    bare = DeviceAggregator(homes, oat, ghi, tou, 0, total, **kw)
    full = DeviceAggregator(homes, oat, ghi, tou, 0, total, ev=fleet(), **kw)
    times = {"bare": [], "fleet": []}
    for rep in range(args.reps):
        order = [("bare", bare), ("fleet", full)]
        if rep % 2:
            order.reverse()
        for name, agg in order:
            run(agg, args.warmup)
        for name, agg in order:
            times[name].append(wall_ms(lambda a=agg: run(a, args.steps)) / args.steps)
    same = (torch.equal(bare.batch.vals.view(torch.int64), full.batch.vals.view(torch.int64)) and
            torch.equal(bare.batch.fc_store.view(torch.int64), full.batch.fc_store.view(torch.int64)))
    if not same:
        raise SystemExit("ev_bench.py: the homes' hash arrays differ with and without the fleet")
    line = {"tool": "ev_bench", "homes": args.homes, "vehicles": M, "horizon": H, "device": torch.cuda.get_device_name(0),
            "ev_step_us_per_launch": round(step_us, 2), "ev_step_ns_per_vehicle": round(step_us * 1e3 / max(M, 1), 2),
            "ev_aggregate_us_per_launch": round(agg_us, 2), "launches": args.launches, "optimal_vehicles": n_opt,
            "algorithmic_bytes": bytes_alg, "hbm_floor_us": round(floor_us, 3),
            "step_ms_without_fleet": stats(times["bare"]), "step_ms_with_fleet": stats(times["fleet"]),
            "steps_per_rep": args.steps, "homes_bit_identical": same}
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fo:
            fo.write(text + "\n")


if __name__ == "__main__":
    main()
