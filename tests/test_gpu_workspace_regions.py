"""The lists in the workspace sit where dragg_amd._lib.workspace_regions says (the library's own map,
dragg_mpc_workspace_regions_get; tests/test_host.py pins its numbers and checks the order of the regions
against literal arithmetic).  N = 5 homes: a list's (N + 2) i32 are not a multiple of 256 bytes, so every
region after a list starts at a rounded offset."""
import os

import pytest

from dragg_amd import _lib as L
from dragg_amd.community import synthetic_homes, synthetic_weather
from dragg_amd.mpc import MPCBatch

pytestmark = pytest.mark.gpu

N, HOURS, DT = 5, 6, 4


def _batch():
    homes = synthetic_homes(N, seed=12, days=2, dt=DT, horizon_hours=HOURS)
    oat, ghi, tou = synthetic_weather(2, DT, 1, seed=3, month=7)
    b = MPCBatch(homes, oat, ghi, tou, 0, [0.0], int_mode="round", seed=12)
    assert (b.N, b.H, b.S) == (N, 24, 6)
    return b


def _step_and_lengths(b):
    """One serial step; the (deferred, step-function, mid) list lengths: the i32 after a list's N entries."""
    b.step(0)
    lengths = tuple(b.work_list(k)[1] for k in ("deferred", "steps_list", "mid_list"))
    assert b.workspace.numel() * b.workspace.element_size() >= L.workspace_regions(b.dims)["total"]
    n_opt = int((b.status == L.ST_OPTIMAL).sum())
    return n_opt, lengths


def test_lists_sit_where_workspace_regions_says(gpu):
    # every home's chains forced to the step-function DP: its list holds them, the other two stay empty
    b = _batch()
    old = os.environ.get("DRAGG_FORCE_STEP_DP")
    os.environ["DRAGG_FORCE_STEP_DP"] = "1"
    L.reload_knobs()
    try:
        n_opt, (deferred, steps, mid) = _step_and_lengths(b)
    finally:
        if old is None:
            os.environ.pop("DRAGG_FORCE_STEP_DP", None)
        else:
            os.environ["DRAGG_FORCE_STEP_DP"] = old
        L.reload_knobs()
    assert n_opt >= 4                                             # (so that no length is trivially zero)
    assert steps == int(((b.int_path & L.PATH_STEPS) != 0).sum()) and steps >= 4
    assert deferred == 0 and mid == 0
    # a reward price that changes at every stage: the hot launch defers every home it does not refuse
    b = _batch()
    b.set_reward_price([0.01 * (-1) ** k for k in range(b.H)])
    n_opt, (deferred, _, _) = _step_and_lengths(b)
    assert n_opt >= 4
    assert deferred == int(((b.int_path & L.PATH_SECOND) != 0).sum()) and deferred >= 4
