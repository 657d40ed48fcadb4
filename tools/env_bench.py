#!/usr/bin/env python3
"""The vector environment a policy sees, host-driven against device-resident, on the same build.

The community of tools/vector_bench.py (Nb = 20, H = 24, July, one price value per step) as E = 8, 64 and 512
episodes, stepped in two closed loops:

  (a) `rl.VectorEnv` with `SetpointAgent.act_vector`: the sums come to the host every step, the setpoints and
      the controller are numpy and Python over the E episodes;
  (b) `rl.DeviceVectorEnv` with `SetpointAgent.act_device`: one filing kernel after the solve, observations,
      controller and prices stay on the device.

First both loops run the same steps from the same start and must leave bit-identical states (hash arrays,
history stores, clocks) and observations, or the tool fails.  Then each repetition times --steps steps of each
loop after --warmup steps, wall clock between two `torch.cuda.synchronize()` calls, the two loops alternated
and the order swapped every repetition (a b, b a, ...); beside them the bare `VectorAggregator.step` under
fixed prices, timed the same way.  Every timed window starts from a reset of all episodes (untimed).  Last, one
staggered reset (one episode of E, the others mid-run) on both paths, timed the same way.
Prints one JSON line and writes it to --out.  Needs a GPU (there is no fallback).

    python tools/env_bench.py --out profiles/r11/env/env_line.json
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


def stats(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
            "reps": [round(x, 4) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, nargs="+", default=[8, 64, 512])
    ap.add_argument("--homes", type=int, default=20)
    ap.add_argument("--horizon-hours", type=int, default=6)
    ap.add_argument("--dt", type=int, default=4)
    ap.add_argument("--month", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--prev-timesteps", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("env_bench.py: no GPU (a timing needs one)")
    from dragg_amd.community import reference_completable, synthetic_homes, synthetic_weather
    from dragg_amd.rl import DeviceVectorEnv, SetpointAgent, VectorEnv
    from dragg_amd.vector import VectorAggregator

    Nb, dt, W, S = args.homes, args.dt, args.warmup, args.steps
    H = args.horizon_hours * dt
    total, max_start = W + S, 7
    sim_hours = math.ceil((total + max_start + 1) / dt)
    days = math.ceil((sim_hours + args.horizon_hours + 2) / 24) + 1
    homes = synthetic_homes(Nb, seed=12, days=days, dt=dt, horizon_hours=args.horizon_hours)
    oat, ghi, tou = synthetic_weather(days, dt, sim_hours, seed=3, month=args.month)
    homes, _ = reference_completable(homes, oat, ghi, tou, seed=12)
    cfg = {"agg": {"rl": {"prev_timesteps": args.prev_timesteps}},
           "rl": {"utility": {"action_space": [-2.0, 2.0], "action_scale": 100.0}}}

    def bits(x):
        return x.contiguous().view(torch.int64) if x.dtype == torch.float64 else x

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    rows = []
    for E in args.episodes:
        seeds, starts = [12 + e for e in range(E)], [e % (max_start + 1) for e in range(E)]
        va_a, va_b, va_c = (VectorAggregator(homes, oat, ghi, tou, E, seeds, starts, total) for _ in range(3))
        env_a, env_b = VectorEnv(va_a, cfg), DeviceVectorEnv(va_b, cfg)
        ag_a, ag_b = SetpointAgent(cfg), SetpointAgent(cfg)
        ag_a.history = {"error": [], "action": []}
        fixed = torch.as_tensor(np.random.default_rng(5).uniform(-0.02, 0.02, (total, E)), dtype=torch.float64,
                                device=va_c.device)

        def loop_a(n, start=True):
            if start:
                ag_a.reset_vector()
                ag_a.history = {"error": [], "action": []}
            obs = env_a.reset() if start else env_a.observations()
            for _ in range(n):
                obs, _ = env_a.step(ag_a.act_vector(obs))
            return obs

        def loop_b(n, start=True):
            if start:
                ag_b.reset_device()
            obs = env_b.reset() if start else env_b.observations()
            for _ in range(n):
                obs, _ = env_b.step(ag_b.act_device(obs, history=False))
            return obs

        def loop_c(n):
            va_c.reset()
            for k in range(n):
                va_c.step(fixed[k])

        # ---- the same steps on both paths: bit-identical states and observations
        oa, ob = loop_a(W + 3), loop_b(W + 3)
        torch.cuda.synchronize()
        same = all(torch.equal(bits(torch.as_tensor(np.asarray(oa[k], dtype=np.float64))), bits(ob[k].cpu())) for k in oa)
        same = same and all(torch.equal(bits(x), bits(y)) for x, y in (
            (va_a.batch.vals, va_b.batch.vals), (va_a.batch.fc_store, va_b.batch.fc_store), (va_a.hist, va_b.hist),
            (va_a.status_hist, va_b.status_hist), (va_a.path_hist, va_b.path_hist), (va_a.agg_hist, va_b.agg_hist),
            (va_a.clocks, va_b.clocks)))
        if not same:
            raise SystemExit(f"env_bench.py: E = {E}: the two environments differ")

        # ---- the loops, alternated
        def timed_a():
            loop_a(W)
            return wall(lambda: loop_a(S, start=False)) / S

        def timed_b():
            loop_b(W)
            return wall(lambda: loop_b(S, start=False)) / S

        def timed_c():
            loop_c(W)
            return wall(lambda: [va_c.step(fixed[W + k]) for k in range(S)]) / S
        ta, tb, tc = [], [], []
        for r in range(args.reps):
            for which in ((timed_a, timed_b) if r % 2 == 0 else (timed_b, timed_a)):
                (ta if which is timed_a else tb).append(which())
            tc.append(timed_c())

        # ---- one staggered reset: one episode of E starts over, the others stay mid-run
        one_host = [E // 2]
        one_dev = torch.zeros(E, dtype=torch.bool, device=va_b.device)
        one_dev[E // 2] = True
        ra, rb = [], []
        for r in range(args.reps):
            for which in (("a", "b") if r % 2 == 0 else ("b", "a")):
                if which == "a":
                    ra.append(wall(lambda: env_a.reset(one_host)))
                else:
                    rb.append(wall(lambda: env_b.reset(one_dev)))
        ma, mb = statistics.median(ta), statistics.median(tb)
        rows.append({"E": E, "host_env_ms_per_step": stats(ta), "device_env_ms_per_step": stats(tb),
                     "bare_step_ms_per_step": stats(tc),
                     "host_env_episode_steps_per_s": round(E / ma * 1e3, 1),
                     "device_env_episode_steps_per_s": round(E / mb * 1e3, 1),
                     "bare_step_episode_steps_per_s": round(E / statistics.median(tc) * 1e3, 1),
                     "device_over_host": round(mb / ma, 4), "device_not_slower": bool(mb <= ma),
                     "staggered_reset_ms": {"host_env": stats(ra), "device_env": stats(rb)},
                     "states_and_observations_bit_identical": True})
        del va_a, va_b, va_c, env_a, env_b
        torch.cuda.empty_cache()

    line = {"metric": "ms per environment step (policy call + step + observations), wall clock between two "
                      "device synchronisations, medians of alternated repetitions",
            "config": {"homes": Nb, "horizon": H, "dt": dt, "month": args.month, "steps": S, "warmup": W,
                       "reps": args.reps, "prev_timesteps": args.prev_timesteps, "price": "scalar",
                       "device": torch.cuda.get_device_name(0)},
            "rows": rows,
            "note": "(a) VectorEnv + act_vector, (b) DeviceVectorEnv + act_device, order swapped every repetition; "
                    "bare: VectorAggregator.step under fixed prices; every window starts from a reset of all "
                    "episodes and the warm-up steps (untimed)"}
    s = json.dumps(line)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
