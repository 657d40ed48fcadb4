#!/usr/bin/env python3
"""Playing a swept candidate: adopt its solved step against solving it again, on the same build.

Two workloads: the RL bench community (`bench.py --workload rl`: 10k homes, H = 48, the smooth price,
`DeviceAggregator`) and the vector shape of tools/vector_bench.py (Nb = 20, H = 24, E = 64 episodes,
`VectorAggregator`).  For G (or C) candidates in --candidates, from the same live state every time:

  (a) today's path:  sweep, then the chosen candidate solved again (`set_reward_price` + `run_iteration` +
      `collect_data`; vector: `select` + `step` under the chosen rows);
  (b) the held path: sweep(hold=True), then `commit` + `collect_data` (vector: `select` + `commit`).

First (a) and (b) are run once each and must leave bit-identical state (hash arrays, history row, status and
path rows, sums), or the tool fails.  Then they are timed --reps times each, alternating and swapping the
order every repetition (a b, b a, ...), with HIP events on the stream around the whole action; the state is
put back between actions outside the timed window.  Separately: the adopt kernel alone (events around
--kernel-reps back-to-back `adopt_from` calls, the adopted copy rotated from call to call; bytes moved =
2 x (NVAL 8 + NFC H 8 + the out members) per adopted home; at G = 1 the same bytes are copied every time and
stay in the memory-side cache: a cache-warm rate), for the RL workload the replicate kernel alone (the same
events around back-to-back `replicate_from` calls) and, at --forecast-horizon > 1 steps, the clone of the
first step's arrays.
Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/commit_bench.py --out profiles/r10/commit/commit_line.json
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--homes", type=int, default=10000)
    ap.add_argument("--horizon-hours", type=int, default=12)
    ap.add_argument("--dt", type=int, default=4)
    ap.add_argument("--month", type=int, default=7)
    ap.add_argument("--candidates", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--forecast-horizon", type=int, default=2, help="the rollout length of the clone measurement")
    ap.add_argument("--warmup", type=int, default=4, help="committed steps before the measurement")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--vector-homes", type=int, default=20)
    ap.add_argument("--vector-horizon-hours", type=int, default=6)
    ap.add_argument("--skip", choices=("rl", "vector"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("commit_bench.py: no GPU (a timing needs one)")
    import bench
    from dragg_amd import _lib as L
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.members import Held
    from dragg_amd.community import reference_completable, synthetic_homes, synthetic_weather
    from dragg_amd.vector import VectorAggregator

    def bits(x):
        return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def rotate(a, b, reset, reps):
        """a and b alternated, the order swapped every repetition; `reset` before each (untimed)."""
        ta, tb = [], []
        for r in range(reps):
            for which in ((a, b) if r % 2 == 0 else (b, a)):
                reset()
                (ta if which is a else tb).append(timed(which))
        return ta, tb

    def adopt_bytes(H, hist):
        return 2 * (L.NVAL * 8 + L.NFC * H * 8 + 3 * 4 + 2 * 8 + (L.NVAL * 8 if hist else 0))

    def kernel_time(fn, reps):
        """ms per call of fn(i), i = 0 .. reps - 1 back to back (the callers rotate the adopted copy with i, so
        that with G > 1 the source is not the same cache-resident bytes every time)."""
        fn(0)
        return timed(lambda: [fn(i) for i in range(reps)]) / reps

    line = {"metric": "ms per RL action (sweep of G candidates + the chosen candidate's step), HIP events",
            "device": torch.cuda.get_device_name(0), "reps": args.reps, "rl": None, "vector": None,
            "note": "(a) and (b) alternated, order swapped every repetition, state put back untimed between "
                    "actions; one untimed action of each first (code objects, replica batch, workspace)"}

    # ------------------------------------------------------------------ the RL bench community
    if args.skip != "rl":
        fh = args.forecast_horizon
        args.steps = fh + 2
        homes, oat, ghi, tou = bench.bench_community(args)
        homes, _ = bench.reference_completable(homes, oat, ghi, tou, seed=12)
        H = args.horizon_hours * args.dt
        shape = -0.03 * np.cos(np.arange(H) / 3.0)        # bench.py --rl-price smooth: a change at every stage
        live = np.random.default_rng(5).uniform(-0.02, 0.02, (args.warmup + 1, 1)) + shape[None, :]
        agg = DeviceAggregator(homes, oat, ghi, tou, 0, args.warmup + fh + 2, reward_price=[0.0], seed=12)
        for k in range(args.warmup):
            agg.set_reward_price(live[k])
            agg.run_iteration()
            agg.collect_data()
        agg.set_reward_price(live[args.warmup])
        t = agg.timestep
        snap = agg.snapshot()
        rows = []
        for G in args.candidates:
            cands = np.linspace(-0.02, 0.02, G)[:, None] + shape[None, :] if G > 1 else shape[None, :] + 0.01
            g = G - 1
            P = torch.as_tensor(cands, dtype=torch.float64, device=agg.device)

            def reset():
                agg.restore(snap)

            def today(steps=1):
                agg.sweep(P, steps)
                agg.set_reward_price(P[g])
                agg.run_iteration()
                return agg.collect_data()

            def held(steps=1):
                agg.sweep(P, steps, hold=True)
                agg.commit(g)
                return agg.collect_data()

            def state(sums):
                agg.drain()
                b = agg.batch
                return [bits(x).clone() for x in (b.vals, b.fc_store, agg.hist[t], agg.status_hist[t], agg.path_hist[t],
                                                  b.status, b.int_path, b.obj, b.rp, sums)]
            reset()
            sa = state(today())
            reset()
            sb = state(held())
            if not all(torch.equal(x, y) for x, y in zip(sa, sb)):
                raise SystemExit(f"commit_bench.py: G = {G}: the committed state differs from the solved step's")
            ta, tb = rotate(today, held, reset, args.reps)
            # the adopt kernel alone (the replica batch still holds the last sweep's step)
            reset()
            agg.sweep(P, 1, hold=True)
            rb, chs = agg._hold["src"], torch.arange(G, dtype=torch.int32, device=agg.device)
            k_ms = kernel_time(lambda i: agg.batch.adopt_from(rb, chs[i % G:i % G + 1], hist=agg.hist[t]),
                               args.kernel_reps)
            nbytes = adopt_bytes(H, True) * agg.batch.N
            # ... and the replicate kernel alone (the live state fanned out to the G replicas again)
            rep_ms = kernel_time(lambda i: rb.replicate_from(agg.batch), args.kernel_reps)
            row = {"G": G, "today_ms": stats(ta), "held_ms": stats(tb),
                   "held_over_today": round(statistics.median(tb) / statistics.median(ta), 4),
                   "replicate_kernel_ms": round(rep_ms, 4),
                   "adopt_kernel_ms": round(k_ms, 4), "adopt_bytes": nbytes,
                   "adopt_GBps": round(nbytes / (k_ms * 1e-3) / 1e9, 1), "state_bit_identical": True}
            if fh > 1:
                ta2, tb2 = rotate(lambda: today(fh), lambda: held(fh), reset, max(2, args.reps // 2))
                reset()
                agg.sweep(P, 1, hold=True)
                unit = agg._hold["unit"]
                row[f"steps{fh}"] = {"today_ms": stats(ta2), "held_ms": stats(tb2),
                                     "clone_ms": round(kernel_time(lambda i: Held(unit).fill(unit, rb.hist_row), 5), 4)}
            rows.append(row)
            reset()
            del agg.members.replicas[G]
            agg._hold = None
            torch.cuda.empty_cache()
        line["rl"] = {"config": {"homes": len(homes), "horizon": H, "dt": args.dt, "month": args.month,
                                 "price": "smooth", "committed_steps": args.warmup, "played_candidate": "G - 1"},
                      "rows": rows}
        del agg
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ the vector shape
    if args.skip != "vector":
        E, Nb, dt, Hh, W = args.episodes, args.vector_homes, args.dt, args.vector_horizon_hours, args.warmup
        H = Hh * dt
        total, max_start = W + 2, 7
        sim_hours = math.ceil((total + max_start + 1) / dt)
        days = math.ceil((sim_hours + Hh + 2) / 24) + 1
        homes = synthetic_homes(Nb, seed=12, days=days, dt=dt, horizon_hours=Hh)
        oat, ghi, tou = synthetic_weather(days, dt, sim_hours, seed=3, month=args.month)
        homes, _ = reference_completable(homes, oat, ghi, tou, seed=12)
        va = VectorAggregator(homes, oat, ghi, tou, E, [12 + e for e in range(E)],
                              [e % (max_start + 1) for e in range(E)], total)
        rng = np.random.default_rng(5)
        for k in range(W):
            va.step(rng.uniform(-0.02, 0.02, E))
        names = ("hist", "status_hist", "path_hist", "agg_hist", "clocks")
        bnames = ("vals", "fc_store", "status", "iters", "obj", "relax_obj", "int_path")
        saved = [getattr(va, k).clone() for k in names] + [getattr(va.batch, k).clone() for k in bnames]
        target = va.batch.aggregate_groups()[:, 0].clone()       # setpoints: the episodes' current loads

        def vreset():
            for k, v in zip(names, saved):
                if k == "clocks":
                    va.clocks = v.clone()
                else:
                    getattr(va, k).copy_(v)
            for k, v in zip(bnames, saved[len(names):]):
                getattr(va.batch, k).copy_(v)

        vrows = []
        for C in args.candidates:
            cands = torch.as_tensor(np.linspace(-0.02, 0.02, C)[None, :] + rng.uniform(-0.005, 0.005, (E, 1)),
                                    dtype=torch.float64, device=va.device) if C > 1 else \
                torch.as_tensor(rng.uniform(-0.02, 0.02, (E, 1)), dtype=torch.float64, device=va.device)
            ar = torch.arange(E, device=va.device)

            def vtoday():
                sums = va.sweep(cands, hold=False)
                ch = va.select(sums, target, cands)
                return va.step(cands[ar, ch.clamp(0).to(torch.int64)])

            def vheld():
                sums = va.sweep(cands)
                return va.commit(va.select(sums, target, cands))

            def vstate(sums):
                return [bits(getattr(va, k)).clone() for k in names] + \
                       [bits(getattr(va.batch, k)).clone() for k in bnames] + [bits(sums).clone()]
            vreset()
            sa = vstate(vtoday())
            vreset()
            sb = vstate(vheld())
            if not all(torch.equal(x, y) for x, y in zip(sa, sb)):
                raise SystemExit(f"commit_bench.py: C = {C}: the committed episodes differ from the solved steps'")
            ta, tb = rotate(vtoday, vheld, vreset, args.reps)
            vreset()
            sums = va.sweep(cands)
            ch = va.select(sums, target, cands)
            rb = va._hold["src"]
            chs = [((ch + i) % C).contiguous() for i in range(C)]
            k_ms = kernel_time(lambda i: va.batch.adopt_from(rb, chs[i % C], hist=va._row), args.kernel_reps)
            nbytes = adopt_bytes(H, True) * va.batch.N
            vrows.append({"C": C, "today_ms": stats(ta), "held_ms": stats(tb),
                          "held_over_today": round(statistics.median(tb) / statistics.median(ta), 4),
                          "adopt_kernel_ms": round(k_ms, 4), "adopt_bytes": nbytes,
                          "adopt_GBps": round(nbytes / (k_ms * 1e-3) / 1e9, 1), "state_bit_identical": True})
            vreset()
        line["vector"] = {"config": {"episodes": E, "homes": Nb, "horizon": H, "dt": dt, "month": args.month,
                                     "price": "scalar", "committed_steps": W}, "rows": vrows}

    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
