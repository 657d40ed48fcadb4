#!/usr/bin/env python3
"""What price classes cost (dragg_mpc_step_classes, dragg_mpc_plan_classes), on one build.

(a) The step.  The community of tools/env_bench.py (Nb = 20, H = 24, July, one price value per step) as E = 8, 64
    and 512 episodes in two `VectorAggregator`s: one without classes (P = 1: dragg_mpc_step_episodes), one with
    `price_classes="type"` (P = 4: dragg_mpc_step_classes).  Both play the same numeric price in every class --
    different prices would change which chains are RL-priced, i.e. the work itself -- so the two must leave
    bit-identical hash arrays and sums, or the tool fails.  Each repetition times --steps steps of each after a
    reset and --warmup steps, wall clock between two `torch.cuda.synchronize()` calls, the two alternated and the
    order swapped every repetition; medians, every repetition kept.

(b) dragg_mpc_plan_classes alone at bench size: --homes homes (10,000), H = 48, July, mid-run under RL prices
    (tools/plan_bench.py's community and state), keys p_grid and p_load, P = 4 by home type, beside
    dragg_mpc_plan_groups on the same batch.  Cache-warm: --launches back-to-back launches between two device
    events.  Cold: one launch between two events after a 1 GiB device fill, --reps times.  Four plan_groups launches
    on masked copies is what the same rows cost without the entry point.  The class rows must equal plan_groups'
    rows of NaN-masked copies bit for bit, or the tool fails.

Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/classes_bench.py --out profiles/r15/classes/classes_line.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("p_grid", "p_load")


def stats(xs, nd=4):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd),
            "reps": [round(x, nd) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="*", default=[8, 64, 512])
    ap.add_argument("--env-homes", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--homes", type=int, default=10000, help="part (b): community size (0: skip part (b))")
    ap.add_argument("--committed", type=int, default=4, help="part (b): committed RL steps before the measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("classes_bench.py: no GPU (a timing needs one)")
    from dragg_amd.community import reference_completable, synthetic_homes, synthetic_weather
    from dragg_amd.vector import VectorAggregator

    def bits(x):
        return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

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

    # ------------------------------------------------------------------ (a) the step, P = 1 against P = 4
    Nb, dt, hh, W, S = args.env_homes, 4, 6, args.warmup, args.steps
    H = hh * dt
    total, max_start = W + S, 7
    sim_hours = math.ceil((total + max_start + 1) / dt)
    days = math.ceil((sim_hours + hh + 2) / 24) + 1
    homes = synthetic_homes(Nb, seed=12, days=days, dt=dt, horizon_hours=hh)
    oat, ghi, tou = synthetic_weather(days, dt, sim_hours, seed=3, month=7)
    homes, _ = reference_completable(homes, oat, ghi, tou, seed=12)
    rows = []
    for E in args.episodes:
        seeds, starts = [12 + e for e in range(E)], [e % (max_start + 1) for e in range(E)]
        va1 = VectorAggregator(homes, oat, ghi, tou, E, seeds, starts, total)
        va4 = VectorAggregator(homes, oat, ghi, tou, E, seeds, starts, total, price_classes="type")
        P = va4.n_classes
        act = torch.as_tensor(np.random.default_rng(5).uniform(-0.02, 0.02, (total, E)), device=va1.device)
        act4 = act[:, :, None].expand(total, E, P).contiguous()         # the same price in every class

        def loop(va, prices, lo, hi, start=True):
            if start:
                va.reset()
            for k in range(lo, hi):
                last = va.step(prices[k])
            return last

        s1, s4 = loop(va1, act, 0, W + 3), loop(va4, act4, 0, W + 3)
        torch.cuda.synchronize()
        if not all(torch.equal(bits(x), bits(y)) for x, y in (
                (s1, s4), (va1.batch.vals, va4.batch.vals), (va1.batch.fc_store, va4.batch.fc_store),
                (va1.batch.status, va4.batch.status), (va1.batch.int_path, va4.batch.int_path), (va1.hist, va4.hist))):
            raise SystemExit(f"classes_bench.py: E = {E}: equal class prices do not give the plain step's bits")

        def timed(va, prices):
            loop(va, prices, 0, W)
            return wall(lambda: loop(va, prices, W, total, start=False)) / S
        t1, t4 = [], []
        for r in range(args.reps):
            for which in ((1, 4) if r % 2 == 0 else (4, 1)):
                (t1 if which == 1 else t4).append(timed(va1, act) if which == 1 else timed(va4, act4))
        m1, m4 = statistics.median(t1), statistics.median(t4)
        rows.append({"E": E, "P": P, "classes": "type", "p1_ms_per_step": stats(t1), "p4_ms_per_step": stats(t4),
                     "p4_over_p1_medians": round(m4 / m1, 4),
                     "p4_median_inside_p1_repetitions": bool(min(t1) <= m4 <= max(t1)),
                     "states_and_sums_bit_identical": True})
        print(f"classes_bench.py: E = {E} done", file=sys.stderr, flush=True)
        del va1, va4
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ (b) plan_classes at bench size
    big = None
    if args.homes > 0:
        import bench
        from dragg_amd.aggregator import DeviceAggregator
        b_args = argparse.Namespace(homes=args.homes, horizon_hours=12, dt=4, month=7, warmup=args.committed, steps=2)
        homes, oat, ghi, tou = bench.bench_community(b_args)
        homes, _ = bench.reference_completable(homes, oat, ghi, tou, seed=12)
        Hb = 48
        shape = -0.03 * np.cos(np.arange(Hb) / 3.0)
        live = np.random.default_rng(5).uniform(-0.02, 0.02, (args.committed + 1, 1)) + shape[None, :]
        agg = DeviceAggregator(homes, oat, ghi, tou, 0, args.committed + 2, reward_price=[0.0], seed=12)
        for k in range(args.committed):
            agg.set_reward_price(live[k])
            agg.run_iteration()
            agg.collect_data()
        b = agg.batch
        cm = b.types_host[:b.Nb].astype(np.int64)
        b.set_price_classes(cm, 4)           # (only the plan reads the map: no step follows)
        print(f"classes_bench.py: {len(homes)} homes mid-run", file=sys.stderr, flush=True)
        out_c = b.plan_groups(KEYS, classes=True)
        out_g = b.plan_groups(KEYS)
        # the contract at this size: class c's rows are plan_groups' of the copy with the other classes absent
        for c in range(4):
            other = torch.as_tensor(cm != c, device=b.device)
            vals, fc = b.vals.clone(), b.fc_store.clone()
            vals[:, other] = float("nan")
            fc[other] = float("nan")
            ref = b.plan_groups(KEYS, src=types.SimpleNamespace(vals=vals, fc_store=fc, N=b.N, groups=1, H=b.H))
            if not (torch.equal(bits(ref[0][0]), bits(out_c[0][0, c])) and torch.equal(ref[1][0], out_c[1][0, c])):
                raise SystemExit(f"classes_bench.py: class {c}: not plan_groups' rows of the masked copy")
            del vals, fc
        flush = torch.empty(1 << 27, dtype=torch.float64, device=agg.device)          # 1 GiB

        def measure(fn):
            warm = events_us(fn, args.launches)
            cold = []
            for _ in range(args.reps):
                flush.fill_(1.0)
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                e.record()
                torch.cuda.synchronize()
                cold.append(a.elapsed_time(e) * 1e3)
            return {"cache_warm_us": round(warm, 2), "cold_us": stats(cold, 2)}
        mc = measure(lambda: b.plan_groups(KEYS, out=out_c, classes=True))
        mg = measure(lambda: b.plan_groups(KEYS, out=out_g))
        big = {"homes": len(homes), "horizon": Hb, "keys": list(KEYS), "P": 4, "classes": "type",
               "homes_per_class": np.bincount(cm, minlength=4).tolist(), "committed_steps": args.committed,
               "plan_classes": mc, "plan_groups_same_batch": mg,
               "plan_classes_over_4x_plan_groups_cache_warm": round(mc["cache_warm_us"] / (4 * mg["cache_warm_us"]), 4),
               "plan_classes_over_4x_plan_groups_cold": round(mc["cold_us"]["median"] / (4 * mg["cold_us"]["median"]), 4),
               "class_rows_equal_masked_plan_groups_rows": True}

    line = {"metric": "(a) ms per VectorAggregator.step without classes (P = 1) and with P = 4 classes by home type under "
                      "the same numeric prices, wall clock between two device synchronisations, medians of alternated "
                      "repetitions; (b) microseconds per dragg_mpc_plan_classes / dragg_mpc_plan_groups launch from "
                      "device events",
            "config": {"env_homes": Nb, "env_horizon": H, "steps": S, "warmup": W, "reps": args.reps,
                       "launches": args.launches, "device": torch.cuda.get_device_name(0)},
            "step_rows": rows, "plan_classes_alone": big,
            "note": "cache-warm: back-to-back launches re-reading the same arrays; cold: after a 1 GiB device fill; a "
                    "device-event time of one short launch includes its launch gap"}
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
