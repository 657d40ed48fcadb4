"""Diagnostic: per step, how many homes each later launch took (the lists in the workspace):
hot -> mid (deferred), mid -> big (past 384 labels), any -> step-function DP.
Usage: python tools/launch_counts.py [--rl] [--steps K] [--homes N]"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dragg_amd.aggregator import DeviceAggregator                   # noqa: E402
from dragg_amd.community import synthetic_homes, synthetic_weather  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--homes", type=int, default=10000)
ap.add_argument("--steps", type=int, default=24)
ap.add_argument("--rl", action="store_true")
a = ap.parse_args()
dt, hh = 4, 12
days = math.ceil((math.ceil(a.steps / dt) + hh + 2) / 24) + 1
homes = synthetic_homes(a.homes, seed=12, days=days, dt=dt, horizon_hours=hh)
oat, ghi, tou = synthetic_weather(days, dt, math.ceil(a.steps / dt), seed=3, month=7)
agg = DeviceAggregator(homes, oat, ghi, tou, 0, a.steps, reward_price=[0.0], seed=12, keep_history=False)
H = agg.batch.H
rng = np.random.default_rng(5)
tot = np.zeros(3, int)
for t in range(a.steps):
    if a.rl:
        agg.set_reward_price(rng.uniform(-0.02, 0.02) - 0.03 * np.cos(np.arange(H) / 3.0))
    agg.run_iteration()
    c = [agg.batch.work_list(k)[1] for k in ("deferred", "mid_list", "steps_list")]
    tot += c
    print(f"t={t}: deferred {c[0]}, to big {c[1]}, to step DP {c[2]}", flush=True)
print(f"total over {a.steps} steps: deferred {tot[0]}, to big {tot[1]}, to step DP {tot[2]}")
