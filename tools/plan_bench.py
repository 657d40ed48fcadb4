#!/usr/bin/env python3
"""What the plan observations cost (dragg_mpc_plan_groups), on one build.

(a) The environment step.  The community of tools/env_bench.py (Nb = 20, H = 24, July, one price value per
    step) as E = 8, 64 and 512 episodes in two `rl.DeviceVectorEnv` loops with `SetpointAgent.act_device`: one
    with `plan_keys=("p_grid", "p_load")`, one without.  Each repetition times --steps steps of each loop after
    a reset of all episodes and --warmup steps, wall clock between two `torch.cuda.synchronize()` calls, the two
    loops alternated and the order swapped every repetition; medians, every repetition kept.  Beside them the
    plan launch and the filing launch (dragg_mpc_env_file) alone on the same batch: --launches back-to-back
    launches between two device events (cache-warm: every launch re-reads the same arrays).  The two loops
    must leave bit-identical hash arrays and scalar observations, or the tool fails.

(b) The launch alone at bench size: --homes homes (10,000), H = 48, July, mid-run under RL prices
    (tools/sweep_bench.py's community), keys p_grid and p_load: the live batch (G = 1) and the held sweep's
    replica batch of G = 8.  Cache-warm: --launches back-to-back launches between two device events.  Cold: one
    launch between two events after a 1 GiB device fill (the arrays are out of L2 and the Infinity Cache),
    --reps times.  Bytes read = N x nk x H x 8 of fc plus the vals rows read (the counter row and one row per
    key) over the launch time, against the 8,000 GB/s HBM figure of bench.py's roofline.  Beside them one
    `DeviceAggregator.forecast(1)` (what `rl_forecast(1)` runs), wall clock to its device-to-host copy.

Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/plan_bench.py --out profiles/r12/plan/plan_line.json
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

KEYS = ("p_grid", "p_load")
HBM_GBS = 8000.0


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
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--committed", type=int, default=4, help="part (b): committed RL steps before the measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("plan_bench.py: no GPU (a timing needs one)")
    from dragg_amd import _lib as L
    from dragg_amd.community import reference_completable, synthetic_homes, synthetic_weather
    from dragg_amd.rl import DeviceVectorEnv, SetpointAgent
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
        """Microseconds per call of `fn`, n back-to-back calls between two device events."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    # ------------------------------------------------------------------ (a) the environment step
    Nb, dt, hh, W, S = args.env_homes, 4, 6, args.warmup, args.steps
    H = hh * dt
    total, max_start = W + S, 7
    sim_hours = math.ceil((total + max_start + 1) / dt)
    days = math.ceil((sim_hours + hh + 2) / 24) + 1
    homes = synthetic_homes(Nb, seed=12, days=days, dt=dt, horizon_hours=hh)
    oat, ghi, tou = synthetic_weather(days, dt, sim_hours, seed=3, month=7)
    homes, _ = reference_completable(homes, oat, ghi, tou, seed=12)
    cfg = {"agg": {"rl": {"prev_timesteps": 12}}, "rl": {"utility": {"action_space": [-2.0, 2.0], "action_scale": 100.0}}}
    rows = []
    for E in args.episodes:
        seeds, starts = [12 + e for e in range(E)], [e % (max_start + 1) for e in range(E)]
        va_p, va_o = (VectorAggregator(homes, oat, ghi, tou, E, seeds, starts, total) for _ in range(2))
        env_p, env_o = DeviceVectorEnv(va_p, cfg, plan_keys=KEYS), DeviceVectorEnv(va_o, cfg)
        ag_p, ag_o = SetpointAgent(cfg), SetpointAgent(cfg)

        def loop(env, ag, n, start=True):
            if start:
                ag.reset_device()
            obs = env.reset() if start else env.observations()
            for _ in range(n):
                obs, _ = env.step(ag.act_device(obs, history=False))
            return obs

        op, oo = loop(env_p, ag_p, W + 3), loop(env_o, ag_o, W + 3)
        torch.cuda.synchronize()
        same = all(torch.equal(bits(op[k]), bits(oo[k])) for k in oo)
        same = same and all(torch.equal(bits(x), bits(y)) for x, y in (
            (va_p.batch.vals, va_o.batch.vals), (va_p.batch.fc_store, va_o.batch.fc_store), (va_p.hist, va_o.hist),
            (va_p.clocks, va_o.clocks)))
        if not same:
            raise SystemExit(f"plan_bench.py: E = {E}: the plan observations changed the environment")
        load = op["agg_load"]
        if not bool(((op["plan"][:, 0, 0] - load).abs() <= 1e-12 * load.abs()).all()):
            raise SystemExit(f"plan_bench.py: E = {E}: entry 0 of the p_grid curve is not the step's load")

        def timed(env, ag):
            loop(env, ag, W)
            return wall(lambda: loop(env, ag, S, start=False)) / S
        tp, to = [], []
        for r in range(args.reps):
            for which in (("p", "o") if r % 2 == 0 else ("o", "p")):
                (tp if which == "p" else to).append(timed(env_p, ag_p) if which == "p" else timed(env_o, ag_o))
        # the two launches alone, cache-warm (the filing launch re-files row 0 of every episode)
        ran = torch.zeros(E, dtype=torch.int32, device=va_p.device)
        agg = va_p.batch.aggregate_groups()
        plan_us = events_us(lambda: va_p.plan(KEYS, out=env_p._plan), args.launches)
        file_us = events_us(lambda: va_p.batch.env_file(env_p.state, ran, agg, hist=va_p._row), args.launches)
        mp, mo = statistics.median(tp), statistics.median(to)
        rows.append({"E": E, "plan_on_ms_per_step": stats(tp), "plan_off_ms_per_step": stats(to),
                     "added_us_per_step_medians": round((mp - mo) * 1e3, 2),
                     "added_share_of_the_plan_off_step": round((mp - mo) / mo, 4),
                     "plan_launch_alone_us_cache_warm": round(plan_us, 2),
                     "filing_launch_alone_us_cache_warm": round(file_us, 2),
                     "plan_bytes_read": E * Nb * (len(KEYS) * H + len(KEYS) + 1) * 8,
                     "states_and_scalar_observations_bit_identical": True})
        print(f"plan_bench.py: E = {E} done", file=sys.stderr, flush=True)
        del va_p, va_o, env_p, env_o
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ (b) the launch alone at bench size
    big = None
    if args.homes > 0:
        import bench
        from dragg_amd.aggregator import DeviceAggregator
        G = args.candidates
        b_args = argparse.Namespace(homes=args.homes, horizon_hours=12, dt=4, month=7, warmup=args.committed, steps=2)
        homes, oat, ghi, tou = bench.bench_community(b_args)
        homes, _ = bench.reference_completable(homes, oat, ghi, tou, seed=12)
        Hb = 48
        shape = -0.03 * np.cos(np.arange(Hb) / 3.0)
        live = np.random.default_rng(5).uniform(-0.02, 0.02, (args.committed + 1, 1)) + shape[None, :]
        cands = np.linspace(-0.02, 0.02, G)[:, None] + shape[None, :]
        agg = DeviceAggregator(homes, oat, ghi, tou, 0, args.committed + 2, reward_price=[0.0], seed=12)
        for k in range(args.committed):
            agg.set_reward_price(live[k])
            agg.run_iteration()
            agg.collect_data()
        agg.set_reward_price(live[args.committed])
        print(f"plan_bench.py: {len(homes)} homes mid-run", file=sys.stderr, flush=True)
        t_fc = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agg.forecast(1).cpu()
            t_fc.append((time.perf_counter() - t0) * 1e3)
        agg.sweep(cands, 1, hold=True)
        rb = agg._hold["src"]
        flush = torch.empty(1 << 27, dtype=torch.float64, device=agg.device)          # 1 GiB

        def measure(batch, groups, src=None):
            N = batch.N if src is None else src.N
            out = batch.plan_groups(KEYS, src=src)
            fn = lambda: batch.plan_groups(KEYS, out=out, src=src)                     # noqa: E731
            warm = events_us(fn, args.launches)
            cold = []
            for _ in range(args.reps):
                flush.fill_(1.0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                cold.append(a.elapsed_time(b) * 1e3)
            nbytes = N * (len(KEYS) * Hb + len(KEYS) + 1) * 8
            med = statistics.median(cold)
            return {"G": groups, "homes": N, "bytes_read": nbytes,
                    "cache_warm_us": round(warm, 2), "cache_warm_GBs": round(nbytes / warm / 1e3, 1),
                    "cold_us": stats(cold, 2), "cold_GBs": round(nbytes / med / 1e3, 1),
                    "cold_share_of_hbm_peak": round(nbytes / med / 1e3 / HBM_GBS, 4),
                    "count_p_grid_entry_0": out[1][:, 0, 0].cpu().tolist()}
        big = {"homes": len(homes), "horizon": Hb, "keys": list(KEYS), "committed_steps": args.committed,
               "live_batch": measure(agg.batch, 1), "sweep_batch": measure(agg.batch, G, src=rb),
               "forecast_1_ms": stats(t_fc[1:], 3), "hbm_peak_GBs": HBM_GBS}

    line = {"metric": "(a) ms per environment step with and without plan observations, wall clock between two device "
                      "synchronisations, medians of alternated repetitions; (b) microseconds per dragg_mpc_plan_groups "
                      "launch from device events",
            "config": {"env_homes": Nb, "env_horizon": H, "keys": list(KEYS), "steps": S, "warmup": W, "reps": args.reps,
                       "launches": args.launches, "device": torch.cuda.get_device_name(0)},
            "env_rows": rows, "launch_alone": big,
            "note": "cache-warm: back-to-back launches re-reading the same arrays; cold: after a 1 GiB device fill; bytes "
                    "read: N x nk x H x 8 of fc plus N x (nk + 1) x 8 of vals; a device-event time of one short launch "
                    "includes its launch gap"}
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
