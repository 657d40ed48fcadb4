"""sub_subhourly_steps (dims.sub_steps, S) other than 6 on the GPU, against the oracle.

S is a plain config field of the reference (`mpc_calc.py:148-173, 300-309, 342, 407-431, 481-492`):
a stage has the S + 1 integer duty levels 0..S.  The direct modes take 1 <= S <= 15; every chain
with S != 6 leaves the hot launch for the bucketed DP of the mid launch and is then solved exactly
by the step-function DP (int_path bit 15).  The golden fixtures s4_dt4, s1_dt1 and s12_dt2 pin
that route against the reference's own runs (tests/test_gpu_exact.py, test_gpu_parity.py,
test_gpu_closed_loop.py); this module is a synthetic grid over S that needs no reference run:
the oracle's exact optimum (oracle/thermal.py exact_milp, thermal_optimum) and its LP
(oracle/mpc.py build_problem) are the yardsticks.

One community definition serves the grid (`_community`): 16 synthetic homes of all four types at
15-minute steps with a 3 h horizon (H = 12), July or January weather.  One home of each type has
its initial indoor temperature moved to the band edge the weather pushes it over, so that the
first stage's feasible duties are {S} alone (half a duty step of slack), none at all (half a
duty step short: no schedule, LP included), {S} with a tenth of a step of slack, and {1..S}.
With those alone every home without a schedule has an infeasible relaxation too (status
INFEASIBLE), so one more home has its comfort band narrowed to 0.3 duty steps around its initial
temperature: its relaxation is feasible, no integer schedule is, and the status is ROUND_FAIL.
"""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID_S = [1, 2, 3, 4, 5, 7, 8, 12, 15]
SEED = 31                      # chosen on the CPU with the oracle: see test_exact_over_sub_steps
N, DT, HOURS = 16, 4, 3
# the first-stage duty (in duty units, fractional) that puts T_1 exactly on the band edge, for the
# moved home -- the first -- of each type (pv_battery, pv_only, battery_only, base), relative to S.
# (The home without a schedule has no battery: a battery home that fails at t = 0 leaves no
# e_batt_opt, and the reference raises KeyError at t = 1, mpc_calc.py:285.)
MOVED = [("S", -0.5), ("S", +0.5), ("S", -0.1), ("0", +0.5)]


def _community(S, month, n=N, hours=HOURS, seed=SEED, days=2, sim_hours=2, narrow=True):
    from dragg_amd.community import synthetic_homes, synthetic_weather
    homes = synthetic_homes(n, mix=(0.25, 0.25, 0.25, 0.25), seed=seed, days=days, dt=DT, horizon_hours=hours,
                            sub_steps=S)
    oat, ghi, tou = synthetic_weather(days, DT, sim_hours, seed=seed + 1, month=month)
    winter = month == 1
    assert n % 4 == 0 and [h["type"] for h in homes[::n // 4]] == ["pv_battery", "pv_only", "battery_only", "base"]
    for j, (base, off) in enumerate(MOVED):
        hv = homes[j * (n // 4)]["hvac"]
        a = (S if base == "S" else 0) + off
        k, R = 3600.0 / (hv["c"] * 1000 * DT), hv["r"]
        # T_1 = T_0 + k ((oat_1 - T_0) / R +- a P / S) (mpc_calc.py:314-317) = the edge
        if winter:
            hv["temp_in_init"] = (hv["temp_in_min"] - k * (oat[1] / R + a * hv["p_h"] / S)) / (1 - k / R)
        else:
            hv["temp_in_init"] = (hv["temp_in_max"] - k * (oat[1] / R - a * hv["p_c"] / S)) / (1 - k / R)
    if narrow:
        # the second base home: a comfort band of 0.3 duty steps around the initial temperature.  The
        # relaxation holds it with a fractional duty, no integer schedule does (ROUND_FAIL)
        hv = homes[3 * (n // 4) + 1]["hvac"]
        unit = 3600.0 / (hv["c"] * 1000 * DT) * (hv["p_h"] if winter else hv["p_c"]) / S
        hv["temp_in_min"], hv["temp_in_max"] = hv["temp_in_init"] - 0.15 * unit, hv["temp_in_init"] + 0.15 * unit
    return homes, oat, ghi, tou


def _price(kind, tou, H):
    from oracle import mpc as M
    rp = [0.0] if kind == "tou" else [0.03 * math.cos(k / 3.0) for k in range(H)]
    return M.total_price(tou, rp, H)


@functools.lru_cache(maxsize=None)
def _cell(S, month, kind):
    """Homes, t = 0 inputs and the oracle's answers of one cell (computed once, never changed)."""
    from oracle import mpc as M
    from oracle import thermal as TH
    homes, oat, ghi, tou = _community(S, month)
    ins, ths, opts = [], [], []
    for h in homes:
        hc = M.home_const(h)
        draw, _, _ = M.water_draws(hc, 0)
        T0, Tw0, E0, _ = M.initial_conditions(hc, 0, {}, draw)
        o, g, tt = M.env_slice(oat, ghi, tou, 0, 0, hc.H)
        si = M.StepInput(t=0, T0=T0, Tw0=Tw0, E0=E0, oat=o, ghi=g, price=_price(kind, tt, hc.H), draw=draw,
                         winter=month == 1)
        th = TH.thermal_optimum(hc, si)
        ins.append(si)
        ths.append(th)
        opts.append(TH.exact_milp(hc, si, th))
    return homes, ins, ths, opts


def _explicit(ins, H):
    col = lambda k, n: np.array([np.asarray(getattr(s, k), float)[:n] for s in ins]).T  # noqa: E731
    n = len(ins)
    return dict(t=np.array([s.t for s in ins], np.int32), T0=[s.T0 for s in ins], Tw0=[s.Tw0 for s in ins],
                E0=[np.nan if s.E0 is None else s.E0 for s in ins], counter=np.zeros(n, np.int32),
                winter=np.array([int(s.winter) for s in ins], np.int32), draw=col("draw", H + 1),
                oat=col("oat", H + 1), ghi=col("ghi", H + 1), price=col("price", H))


@functools.lru_cache(maxsize=None)
def _solved(S, month, kind, mode="round"):
    import torch
    from dragg_amd.mpc import MPCBatch
    homes, ins, _, _ = _cell(S, month, kind)
    b = MPCBatch(homes, int_mode=mode)
    assert b.S == S and b.H == HOURS * DT
    b.solve_explicit(**_explicit(ins, b.H))
    torch.cuda.synchronize()
    return dict(status=b.status.cpu().numpy(), obj=b.obj.cpu().numpy(), relax=b.relax_obj.cpu().numpy(),
                path=b.int_path.cpu().numpy(), fc=b.fc.cpu().numpy(), vals=b.vals.cpu().numpy())


def _thermal_cost(hc, si, fc, i):
    """sum_k gamma^k price_k S P u_k of the duties in the hash fields (duty / S, mpc_calc.py:497-499)."""
    from dragg_amd import _lib as L
    H, S = hc.H, hc.S
    w = hc.discount ** np.arange(H) * np.asarray(si.price[:H], float)
    u = np.rint(fc[L.FC_KEYS.index("hvac_heat_on_opt" if si.winter else "hvac_cool_on_opt"), :, i] * S)
    wh = np.rint(fc[L.FC_KEYS.index("wh_heat_on_opt"), :, i] * S)
    P = hc.Ph if si.winter else hc.Pc
    return float(w @ (u * (S * P)) + w @ (wh * (S * hc.Pw))), u, wh


# ------------------------------------------------------------------ exactness over S
@pytest.mark.parametrize("kind", ["tou", "rl"])
@pytest.mark.parametrize("month", [7, 1])
@pytest.mark.parametrize("S", GRID_S)
def test_exact_over_sub_steps(S, month, kind, gpu):
    """int_mode round at every S of the grid, July and January, TOU and a cosine RL price: per home the
    status agrees with the exact MILP (an optimum or none), the objective equals it (1e-6 relative),
    the thermal cost of the returned duties equals the exact thermal optimum (1e-9 relative), and
    the answer is the step-function DP's, unflagged.  The seed is one at which the oracle alone has
    an optimum for at least half of the homes of every cell and none for at least one."""
    from dragg_amd import _lib as L
    from oracle import mpc as M
    homes, ins, ths, opts = _cell(S, month, kind)
    res = _solved(S, month, kind)
    n_opt = 0
    for i, (h, si, th, opt) in enumerate(zip(homes, ins, ths, opts)):
        st = res["status"][i]
        assert (st == L.ST_OPTIMAL) == (opt is not None), (S, month, kind, i, L.STATUS_NAMES[st], opt)
        if opt is None:
            continue
        n_opt += 1
        assert abs(res["obj"][i] - opt) <= 1e-6 * max(1.0, abs(opt)), (S, month, kind, i, res["obj"][i], opt)
        hc = M.home_const(h)
        ours, u, wh = _thermal_cost(hc, si, res["fc"], i)
        assert min(u.min(), wh.min()) >= 0 and max(u.max(), wh.max()) <= S, (i, u, wh)
        assert abs(ours - th["cost"]) <= 1e-9 * max(1.0, abs(th["cost"])), (S, month, kind, i, ours, th["cost"])
        assert res["path"][i] & L.PATH_APPROX_MASK == 0, (S, month, kind, i, hex(res["path"][i]))
        assert res["path"][i] & L.PATH_STEPS, (S, month, kind, i, hex(res["path"][i]))
    st = res["status"]
    print(f"S={S} month={month} {kind}: {len(homes)} homes compared, {n_opt} optimal and equal to the exact "
          f"optimum, {int((st == L.ST_ROUND_FAIL).sum())} round_fail, statuses {np.bincount(st, minlength=8).tolist()}")
    assert n_opt >= len(homes) // 2


def test_grid_has_round_fail(gpu):
    """Over the grid (the cells above, solved once per module) at least one home has no integer
    schedule and says so with ROUND_FAIL."""
    from dragg_amd import _lib as L
    n_fail = n_none = 0
    for S in GRID_S:
        for month in (7, 1):
            for kind in ("tou", "rl"):
                n_fail += int((_solved(S, month, kind)["status"] == L.ST_ROUND_FAIL).sum())
                n_none += sum(o is None for o in _cell(S, month, kind)[3])
    print(f"grid: {n_none} homes without a schedule, {n_fail} of them ROUND_FAIL")
    assert n_fail >= 1


# ------------------------------------------------------------------ the largest layouts
def _refused(homes, oat, ghi, tou):
    """The error code every entry point gives a community whose (H, S) the LDS layouts cannot
    take -- and the hash arrays stay as they were.  The device arrays are those of a batch of the
    same homes at H = 4 with only dims.horizon raised: every entry point runs check_dims on the dims
    before it reads a pointer or launches (dragg_mpc_step, dragg_mpc_solve_explicit), and the
    function goes on to them only after dragg_mpc_workspace_bytes has refused these dims."""
    import torch
    from dragg_amd import _lib as L
    from dragg_amd.mpc import MPCBatch, pack_homes
    lib = L.load()
    _, _, _, dm = pack_homes(homes)
    # a batch of the same homes at a horizon that fits lends its device arrays; only dims differ
    small = [dict(h, hems=dict(h["hems"], horizon=1)) for h in homes]
    b = MPCBatch(small, oat, ghi, tou, 0, [0.0], int_mode="round")
    dims = L.Dims.from_buffer_copy(b.dims)
    dims.horizon = dm["H"]
    rc = lib.dragg_mpc_workspace_bytes(ctypes.byref(dims))
    assert rc < 0
    assert lib.dragg_mpc_lds_bytes(ctypes.byref(dims)) == rc
    b.solve_explicit(t=np.zeros(b.N, np.int32), T0=[20.0] * b.N, Tw0=[46.0] * b.N, E0=[5.0] * b.N,
                     counter=np.zeros(b.N, np.int32), winter=np.zeros(b.N, np.int32),
                     draw=np.zeros((b.H + 1, b.N)), oat=np.full((b.H + 1, b.N), 25.0), ghi=np.zeros((b.H + 1, b.N)),
                     price=np.full((b.H, b.N), 0.07))
    torch.cuda.synchronize()
    before = (b.vals.clone().nan_to_num(7.5), b.fc_store.clone().nan_to_num(7.5))
    prob, hsh, out = b._problem(), b._hash(), b._out()
    ex = L.Explicit(**{k: L.ptr(v) for k, v in b._keep.items()})
    assert lib.dragg_mpc_step(ctypes.byref(dims), ctypes.byref(prob), ctypes.byref(hsh), ctypes.byref(out), 0,
                              None, L.stream_ptr(None, b.device)) == rc
    assert lib.dragg_mpc_solve_explicit(ctypes.byref(dims), ctypes.byref(prob), ctypes.byref(ex), ctypes.byref(hsh),
                                        ctypes.byref(out), L.stream_ptr(None, b.device)) == rc
    torch.cuda.synchronize()
    assert torch.equal(b.vals.nan_to_num(7.5), before[0]) and torch.equal(b.fc_store.nan_to_num(7.5), before[1])
    return int(rc)


@pytest.mark.parametrize("S", [15, 1])
def test_too_long_horizon_refused_by_every_entry_point(S, gpu):
    """H = 160 (40 h at 15-minute steps) is past the direct modes' LDS layouts at every S:
    workspace_bytes, lds_bytes, step and solve_explicit all answer DRAGG_E_HORIZON and leave the
    hash arrays untouched.  (H = 96, the longest horizon of the configs, fits at S = 15 and S = 1:
    the test below never meets a refusal.)"""
    from dragg_amd import _lib as L
    homes, oat, ghi, tou = _community(S, 7, n=8, hours=40, days=3, sim_hours=1)
    code = _refused(homes, oat, ghi, tou)
    assert code == -4 and L.load().dragg_mpc_strerror(code) == b"horizon too long for one workgroup's LDS"


@pytest.mark.parametrize("S", [15, 1])
def test_largest_layouts_satisfy_reference_model(S, gpu):
    """S = 15 (the duties fill the DP record's 4-bit field) at the longest horizon of {96, 72, 48, 24}
    the library accepts, and S = 1 at H = 96: two closed-loop steps of 8 homes.  Every optimal answer
    satisfies the reference model assembled by the oracle (violation <= 1e-5, integral duties in 0..S,
    objective = c @ x to 1e-8) and equals the exact MILP optimum (1e-6); a refused horizon is refused
    by every entry point with one code, the hash arrays untouched."""
    import torch
    from oracle import mpc as M
    from oracle import thermal as TH
    from dragg_amd import _lib as L
    from dragg_amd.aggregator import DeviceAggregator
    from tests.test_gpu_fullsize import _hash_dict
    from tests.test_gpu_parity import _expand
    n, steps = 8, 2
    agg = None
    for H in (96, 72, 48, 24):
        homes, oat, ghi, tou = _community(S, 7, n=n, hours=H // DT, days=3, sim_hours=1)
        try:
            agg = DeviceAggregator(homes, oat, ghi, tou, 0, steps, reward_price=[0.0], seed=12)
            break
        except L.DraggError:
            code = _refused(homes, oat, ghi, tou)
            print(f"S={S}: H={H} refused by every entry point with {code}")
            assert S != 1, "S = 1 fits at H = 96"
    assert agg is not None
    b = agg.batch
    assert b.H == H and b.S == S
    worst, n_opt, n_cmp = 0.0, 0, 0
    for t in range(steps):
        pv, pf = b.vals.cpu().numpy().copy(), b.fc.cpu().numpy().copy()
        noise = b.season_noise(t).cpu().numpy()
        agg.run_iteration()
        torch.cuda.synchronize()
        st, obj = b.status.cpu().numpy(), b.obj.cpu().numpy()
        vals, fc = b.vals.cpu().numpy(), b.fc.cpu().numpy()
        assert not np.isin(st, [L.ST_ERR_MISSING, L.ST_ERR_PARSE]).any()
        for i in range(n):
            hc = M.home_const(homes[i])
            draw, _, _ = M.water_draws(hc, t)
            T0, Tw0, E0, _ = M.initial_conditions(hc, t, _hash_dict(pv, pf, i) if t else {}, draw)
            o, g, tt = M.env_slice(oat, ghi, tou, 0, t, hc.H)
            si = M.StepInput(t=t, T0=T0, Tw0=Tw0, E0=E0, oat=o, ghi=g, price=M.total_price(tt, [0.0], hc.H),
                             draw=draw, winter=M.season_is_winter(o, noise[:, i]))
            opt = TH.exact_milp(hc, si)
            n_cmp += 1
            assert (st[i] == L.ST_OPTIMAL) == (opt is not None), (S, t, i, L.STATUS_NAMES[st[i]], opt)
            if opt is None:
                continue
            n_opt += 1
            P, x = _expand(hc, si, vals[:, i], fc[:, :, i], hc.S)
            ve = np.abs(P["A_eq"] @ x - P["b_eq"]).max()
            vu = (P["A_ub"] @ x - P["b_ub"]).max()
            worst = max(worst, ve, vu)
            assert ve <= 1e-5 and vu <= 1e-5, (S, t, i, ve, vu)
            duties = x[P["integrality"] == 1]
            assert np.array_equal(duties, np.round(duties)) and duties.min() >= 0 and duties.max() <= S, (t, i)
            assert abs(P["c"] @ x - obj[i]) <= 1e-8 * max(1, abs(obj[i])), (S, t, i)
            assert abs(obj[i] - opt) <= 1e-6 * max(1.0, abs(opt)), (S, t, i, obj[i], opt)
    print(f"S={S} H={H}: {n_cmp} solves compared, {n_opt} optimal and equal to the exact optimum, "
          f"worst violation {worst:.2e}")
    assert n_opt >= n_cmp // 2


# ------------------------------------------------------------------ the other int modes
@pytest.mark.parametrize("S", [4, 12])
def test_relax_matches_oracle_lp(S, gpu):
    """int_mode relax: status and objective of the LP relaxation against the oracle's LP (HiGHS), at
    tests/test_gpu_parity.py test_lp_status_and_objective's 1e-4 relative."""
    from dragg_amd import _lib as L
    n = _check_relax(S, L)
    assert n >= N // 2


def _check_relax(S, L, month=1, kind="rl"):
    from scipy.optimize import linprog
    from oracle import mpc as M
    homes, ins, _, _ = _cell(S, month, kind)
    res = _solved(S, month, kind, "relax")
    n_opt = 0
    for i, (h, si) in enumerate(zip(homes, ins)):
        P = M.build_problem(M.home_const(h), si)
        lp = linprog(P["c"], A_ub=P["A_ub"], b_ub=P["b_ub"], A_eq=P["A_eq"], b_eq=P["b_eq"],
                     bounds=[(None, None)] * len(P["c"]), method="highs")
        assert (lp.status == 0) == (res["status"][i] == L.ST_OPTIMAL), (S, i, lp.status, L.STATUS_NAMES[res["status"][i]])
        if lp.status == 0:
            n_opt += 1
            assert abs(res["relax"][i] - lp.fun) <= 1e-4 * max(1.0, abs(lp.fun)), (S, i, res["relax"][i], lp.fun)
    print(f"relax S={S}: {len(homes)} homes compared, {n_opt} LP-optimal and equal to the oracle's LP")
    return n_opt


# round_lp's binned DP measured on the MI355X over the 64 homes of each S: no chain above the exact
# optimum, worst gap 1.6e-16 (S = 4) and 2.4e-16 (S = 12), the rounding of two f64 sums of 12 terms.
# Twice a rounding residue is no bound, so the bound is the 1e-9 that every exact comparison of this
# suite allows those sums (tests/test_gpu_exact.py; the same binned DP at S = 6 is allowed 0.02 there).
ROUND_LP_BOUND = 1e-9


@pytest.mark.parametrize("S", [4, 12])
def test_round_lp_never_below_exact_and_flagged(S, gpu):
    """int_mode round_lp at S != 6 sends every chain to the binned dp_chain: the status agrees with
    the exact MILP, the thermal cost is never below the exact optimum (gap >= -1e-9) and, on this
    grid, not above it either (ROUND_LP_BOUND); the worst gap is printed.  A chain above the optimum
    would have to be flagged in int_path: no home of this grid gets there, so that assertion is
    dormant here, and round_lp is known not to flag its binned schedules (open defects:
    negprice_dt2 record 46 at S = 6 is 1.39 % above the optimum with int_path 0)."""
    from dragg_amd import _lib as L
    from oracle import mpc as M
    worst, n_cmp, n_opt, n_above = 0.0, 0, 0, 0
    for month in (7, 1):
        for kind in ("tou", "rl"):
            homes, ins, ths, opts = _cell(S, month, kind)
            res = _solved(S, month, kind, "round_lp")
            for i, (h, si, th, opt) in enumerate(zip(homes, ins, ths, opts)):
                n_cmp += 1
                st = res["status"][i]
                assert (st == L.ST_OPTIMAL) == (opt is not None), (S, month, kind, i, L.STATUS_NAMES[st], opt)
                if opt is None:
                    continue
                n_opt += 1
                ours, _, _ = _thermal_cost(M.home_const(h), si, res["fc"], i)
                gap = (ours - th["cost"]) / max(1.0, abs(th["cost"]))
                assert gap >= -1e-9, (S, month, kind, i, ours, th["cost"])
                if gap > 1e-9:
                    n_above += 1
                    assert res["path"][i] & L.PATH_APPROX_MASK, (S, month, kind, i, gap, hex(res["path"][i]))
                worst = max(worst, gap)
    print(f"round_lp S={S}: {n_cmp} homes compared, {n_opt} optimal, {n_above} above the exact optimum (all "
          f"flagged), worst gap {worst:.3e}")
    assert worst <= ROUND_LP_BOUND


# ------------------------------------------------------------------ closed loop
@pytest.mark.parametrize("S", [4, 15])
def test_step_matches_explicit_restatement(S, gpu):
    """tests/test_gpu_step.py's restatement at S = 4 and 15 over 3 steps: the hash fields written by
    dragg_mpc_step equal, bit for bit, those of solve_explicit on inputs the oracle rebuilds from the
    previous hash; p_grid_opt, forecast_p_grid_opt and p_load_opt are the reference's / S values
    (mpc_calc.py:490-492) of the duties and battery / PV powers in the same hash."""
    import torch
    from dragg_amd import _lib as L
    from dragg_amd.mpc import MPCBatch
    from oracle import mpc as M
    # (January: under the random season draws of this test every home stays in heating mode; in July a
    # "winter" draw fails a battery home at t = 0 and the reference raises KeyError at t = 1)
    homes, oat, ghi, tou = _community(S, 1)
    b = MPCBatch(homes, oat, ghi, tou, 0, [0.0], int_mode="round")
    e = MPCBatch(homes, int_mode="round")
    H, n = b.H, b.N
    rng = np.random.default_rng(5)
    n_opt = 0
    for t in range(3):
        noise = rng.standard_normal((H, n))
        ex = {k: [] for k in ("t", "T0", "Tw0", "E0", "counter", "winter", "draw", "oat", "ghi", "price")}
        hashes = [b.hash_dict(i) for i in range(n)] if t > 0 else [{}] * n
        for i, h in enumerate(homes):
            hc = M.home_const(h)
            draw, _, _ = M.water_draws(hc, t)
            T0, Tw0, E0, cnt = M.initial_conditions(hc, t, hashes[i], draw)
            o, g, tt = M.env_slice(oat, ghi, tou, 0, t, H)
            for k, v in (("t", t), ("T0", T0), ("Tw0", Tw0), ("E0", np.nan if E0 is None else E0),
                         ("counter", cnt), ("winter", int(M.season_is_winter(o, noise[:, i]))),
                         ("draw", draw), ("oat", o), ("ghi", g), ("price", M.total_price(tt, [0.0], H))):
                ex[k].append(v)
        ex = {k: (np.array(v).T if k in ("draw", "oat", "ghi", "price") else np.array(v)) for k, v in ex.items()}
        e.vals.copy_(b.vals)
        e.fc.copy_(b.fc)
        e.solve_explicit(**ex)
        b.step(t, noise=torch.tensor(noise))
        torch.cuda.synchronize()
        assert torch.equal(b.status, e.status), t
        assert torch.equal(torch.nan_to_num(b.vals, 12345.0), torch.nan_to_num(e.vals, 12345.0)), t
        assert torch.equal(torch.nan_to_num(b.fc, 12345.0), torch.nan_to_num(e.fc, 12345.0)), t
        # the / S fields against the model's rows (mpc_calc.py:342, 393-432, 490-492)
        st, fc, vals = b.status.cpu().numpy(), b.fc.cpu().numpy(), b.vals.cpu().numpy()
        f = lambda k: fc[L.FC_KEYS.index(k)]  # noqa: E731
        for i, h in enumerate(homes):
            if st[i] != L.ST_OPTIMAL:
                continue
            n_opt += 1
            hc = M.home_const(h)
            duty = lambda k: np.rint(f(k)[:, i] * S)  # noqa: E731
            p_load = S * (hc.Pc * duty("hvac_cool_on_opt") + hc.Ph * duty("hvac_heat_on_opt") + hc.Pw * duty("wh_heat_on_opt"))
            p_grid = p_load.copy()
            if hc.has_batt:
                p_grid += S * (f("p_batt_ch")[:, i] + f("p_batt_disch")[:, i])
            if hc.has_pv:
                p_grid -= S * f("p_pv_opt")[:, i]
            tol = 1e-9 * max(1.0, np.abs(p_grid).max())
            assert np.abs(f("p_load_opt")[:, i] - p_load / S).max() <= tol, (S, t, i)
            assert np.abs(f("p_grid_opt")[:, i] - p_grid / S).max() <= tol, (S, t, i)
            assert np.abs(f("forecast_p_grid_opt")[:, i] - np.r_[p_grid[1:] / S, 0.0]).max() <= tol, (S, t, i)
            assert vals[L.K["p_grid_opt"], i] == f("p_grid_opt")[0, i] and vals[L.K["p_load_opt"], i] == f("p_load_opt")[0, i]
    print(f"S={S}: 3 steps x {n} homes bit-identical to the explicit restatement; {n_opt} optimal solves' / S fields checked")
    assert n_opt >= 3 * n // 2


def _bits(t):
    import torch
    return t.cpu().contiguous().view(torch.int64).numpy()


def test_lag_mode_bit_identical_at_s4(gpu):
    """Lag mode (enable_lag, a ring of 2) at S = 4, where every home's chains are on the narrow list
    at every step: 64 homes, 6 steps, bit-identical to serial run_iteration (history, status,
    int_path, final hash), as tests/test_gpu_overlap.py asserts at S = 6."""
    import torch
    from dragg_amd import _lib as L
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.mpc import MPCBatch
    n, steps = 64, 6
    homes, oat, ghi, tou = _community(4, 1, n=n)
    a = DeviceAggregator(homes, oat, ghi, tou, 0, steps, reward_price=[0.0], seed=12)
    for _ in range(steps):
        a.run_iteration()
    torch.cuda.synchronize()
    b = MPCBatch(homes, oat, ghi, tou, 0, [0.0], int_mode="round", seed=12)
    b.enable_lag(ring=2)
    hist = torch.full((steps, L.NVAL, n), float("nan"), dtype=torch.float64, device=b.device)
    status = torch.zeros((steps, n), dtype=torch.int32, device=b.device)
    path = torch.zeros((steps, n), dtype=torch.int32, device=b.device)
    for t in range(steps):
        b.step_lagged(t, hist[t], status[t], path_row=path[t])
    b.drain()
    torch.cuda.synchronize()
    narrow = b.lag["lists"].cpu().numpy()[:, 1, n]
    sp = a.path_hist.cpu().numpy()
    st = a.status_hist.cpu().numpy()
    print(f"lag S=4: {steps} steps x {n} homes, {int((st == L.ST_OPTIMAL).sum())} optimal solves, "
          f"{int(((sp & L.PATH_STEPS) != 0).sum())} by the step-function DP, narrow-list lengths of the last ring "
          f"slots {narrow.tolist()}")
    assert ((sp & L.PATH_STEPS) != 0)[st == L.ST_OPTIMAL].all()     # every solved home went through the narrow list
    assert (st == L.ST_OPTIMAL).sum() >= steps * n // 2
    assert np.array_equal(_bits(a.hist), _bits(hist))
    assert np.array_equal(st, status.cpu().numpy())
    assert np.array_equal(sp, path.cpu().numpy())
    assert np.array_equal(_bits(a.batch.vals), _bits(b.vals))
    assert np.array_equal(_bits(a.batch.fc_store), _bits(b.fc_store))


def test_sweep_equals_forecast_at_s4(gpu):
    """The grouped price sweep at S = 4 (the narrow-list entries carry replica home indices):
    sweep(prices, 2) with G = 3 equals three forecast calls bit for bit, on tests/test_gpu_sweep.py's
    community rebuilt with sub_steps = 4, 16 homes."""
    import torch
    from dragg_amd.aggregator import DeviceAggregator
    from dragg_amd.community import synthetic_homes, synthetic_weather
    from tests.test_gpu_sweep import _prices
    homes = synthetic_homes(64, seed=5, days=2, dt=4, horizon_hours=6, sub_steps=4)[:16]
    oat, ghi, tou = synthetic_weather(2, 4, 24, seed=5, month=7)

    def agg():
        a = DeviceAggregator(homes, oat, ghi, tou, 0, 8, reward_price=[0.0] * 24, seed=5)
        for _ in range(2):
            a.run_iteration()
            a.collect_data()
        return a
    a = agg()
    fc = []
    for p in _prices():
        a.set_reward_price(p)
        fc.append(a.forecast(2).clone())
    sw = agg().sweep(_prices(), 2)
    assert tuple(sw.shape) == (3, 2, 3) and not torch.isnan(sw).any()
    for g in range(3):
        assert torch.equal(sw[g], fc[g]), g
    assert not torch.equal(sw[0], sw[1]) and not torch.equal(sw[1], sw[2])
    print(f"sweep S=4: 3 candidates x 2 steps x 16 homes equal to forecast, sums {sw[:, -1, 0].tolist()}")


# ------------------------------------------------------------------ argument edges
@pytest.mark.parametrize("S", [0, 16])
def test_sub_steps_out_of_range_is_refused(S, gpu):
    """S = 0 and S = 16 in int_mode round: DRAGG_E_ARG from workspace_bytes, step and solve_explicit,
    and the hash arrays keep their bits."""
    import torch
    from dragg_amd import _lib as L
    from dragg_amd.mpc import MPCBatch
    lib = L.load()
    homes, ins, _, _ = _cell(4, 1, "tou")
    _, oat, ghi, tou = _community(4, 1)
    b = MPCBatch(homes, oat, ghi, tou, 0, [0.0], int_mode="round")
    b.solve_explicit(**_explicit(ins, b.H))
    torch.cuda.synchronize()
    before = (_bits(b.vals).copy(), _bits(b.fc_store).copy())
    dims = L.Dims.from_buffer_copy(b.dims)
    dims.sub_steps = S
    E_ARG = -1
    assert lib.dragg_mpc_strerror(E_ARG) == b"invalid argument"
    assert lib.dragg_mpc_workspace_bytes(ctypes.byref(dims)) == E_ARG
    prob, hsh, out = b._problem(), b._hash(), b._out()
    ex = L.Explicit(**{k: L.ptr(v) for k, v in b._keep.items()})
    assert lib.dragg_mpc_step(ctypes.byref(dims), ctypes.byref(prob), ctypes.byref(hsh), ctypes.byref(out), 0, None,
                              L.stream_ptr(None, b.device)) == E_ARG
    assert lib.dragg_mpc_solve_explicit(ctypes.byref(dims), ctypes.byref(prob), ctypes.byref(ex), ctypes.byref(hsh),
                                        ctypes.byref(out), L.stream_ptr(None, b.device)) == E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(_bits(b.vals), before[0]) and np.array_equal(_bits(b.fc_store), before[1])


def test_relax_takes_sixteen_sub_steps(gpu):
    """The 4-bit duty field binds the direct modes only: int_mode relax accepts S = 16, and then it
    solves: status and objective equal the oracle's LP."""
    from dragg_amd import _lib as L
    assert _check_relax(16, L) >= N // 2
