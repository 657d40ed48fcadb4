"""CPU tests of the host side: C ABI library/exports/struct layout, packing, keyed RNG,
synthetic inputs.  No GPU compute here."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dragg_mi355x.h")


@pytest.fixture(scope="module")
def lib_path():
    from dragg_amd import build
    return build.build()


def test_library_exports_every_header_symbol(lib_path):
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_mpc_\w+)\s*\(", open(HEADER).read(), re.M)
    assert len(names) >= 7
    lib = ctypes.CDLL(lib_path)
    for n in names:
        assert hasattr(lib, n), n
    from dragg_amd import _lib
    assert set(names) == set(_lib.EXPORTS)
    assert lib.dragg_mpc_abi_version() == _lib.ABI_VERSION


def test_results_library_exports_its_header():
    """libdragg_results.so (the host-side results.json formatter) exports include/dragg_results.h."""
    from dragg_amd import build as B
    path = B.build_results()
    names = re.findall(r"^\w[\w\s\*]*?\b(dragg_\w+)\s*\(", open(os.path.join(ROOT, "include", "dragg_results.h")).read(), re.M)
    assert set(names) == {"dragg_results_abi_version", "dragg_fmt_double", "dragg_fmt_series"}
    lib = ctypes.CDLL(path)
    for n in names:
        assert hasattr(lib, n), n
    assert not B.results_needs_build()


def test_ctypes_structs_match_c_layout(tmp_path):
    """sizeof/offsetof of every ABI struct, from gcc, against the ctypes mirrors."""
    from dragg_amd import _lib as L
    structs = {"dragg_mpc_dims": L.Dims, "dragg_mpc_problem": L.Problem, "dragg_mpc_hash": L.Hash,
               "dragg_mpc_out": L.Out, "dragg_mpc_explicit": L.Explicit,
               "dragg_mpc_workspace_regions": L.WorkspaceRegions}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(line.split() for line in out if line)
    for cname, cls in structs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)


def test_enums_match_header():
    from dragg_amd import _lib as L
    h = open(HEADER).read()
    assert "DRAGG_NFC" in h and len(L.FC_KEYS) == 15 and len(L.VAL_KEYS) == 19
    # order of the fc keys in the header enum
    body = h[h.index("enum dragg_fc_key"):h.index("DRAGG_NFC\n")]
    keys = re.findall(r"DRAGG_K_(\w+)", body)
    want = ["P_GRID", "FORECAST_P_GRID", "P_LOAD", "TEMP_IN_EV", "TEMP_WH_EV", "HVAC_COOL", "HVAC_HEAT",
            "WH_HEAT", "COST", "WATERDRAWS", "P_PV", "U_PV_CURT", "P_BATT_CH", "P_BATT_DISCH", "E_BATT"]
    assert keys == want
    pbody = h[h.index("enum dragg_param"):h.index("DRAGG_NPARAM\n")]
    assert re.findall(r"DRAGG_P_(\w+)", pbody) == L.PARAMS


def test_pack_homes_matches_reference_constants():
    """pack_homes reproduces setup_base/battery/pv_problem's derived constants exactly."""
    from dragg_amd import _lib as L
    from dragg_amd.mpc import pack_homes
    from oracle import mpc as M
    from tests import fixtures as F
    d = F.load("c1_h24")
    P, types, draws, dm = pack_homes(d["homes"])
    assert (dm["S"], dm["dt"], dm["H"]) == (6, 4, 24)
    for i, h in enumerate(d["homes"]):
        hc = M.home_const(h)
        assert P[L.P["R"], i] == hc.R and P[L.P["C"], i] == hc.C and P[L.P["PC"], i] == hc.Pc
        assert P[L.P["PH"], i] == hc.Ph and P[L.P["RW"], i] == hc.Rw and P[L.P["PW"], i] == hc.Pw
        assert P[L.P["CW"], i] == hc.Cw and P[L.P["V"], i] == hc.V
        assert P[L.P["TMIN"], i] == hc.Tmin and P[L.P["TWMAX"], i] == hc.Twmax
        if hc.has_batt:
            assert P[L.P["EMIN"], i] == hc.batt["Emin"] and P[L.P["EINIT"], i] == hc.batt["E_init"]
        assert types[i] == L.TYPE_CODE[h["type"]]
        assert np.array_equal(draws[:len(hc.draw_sizes), i], hc.draw_sizes)


def test_pack_homes_divides_by_sub_steps():
    """sub_subhourly_steps = 4 (mpc_calc.py:159-162): the per-duty-unit powers are p / 4, bit for bit,
    and a community whose homes disagree on S is refused (one batch has one dims.sub_steps; the
    reference's responsive_hems share one hems table, aggregator.py:381-387, 446)."""
    from dragg_amd import _lib as L
    from dragg_amd.community import synthetic_homes
    from dragg_amd.mpc import hems_dims, pack_homes
    homes = synthetic_homes(8, seed=3, dt=4, horizon_hours=3, sub_steps=4)
    homes[2]["hvac"]["p_c"], homes[2]["hvac"]["p_h"], homes[2]["wh"]["p"] = 3.7, 4.1, 2.3   # (not all 3.5 / 2.5)
    P, _, _, dm = pack_homes(homes)
    assert (dm["S"], dm["dt"], dm["H"]) == (4, 4, 12) and hems_dims(homes[0])[0] == 4
    for i, h in enumerate(homes):
        assert P[L.P["PC"], i] == float(h["hvac"]["p_c"]) / 4
        assert P[L.P["PH"], i] == float(h["hvac"]["p_h"]) / 4
        assert P[L.P["PW"], i] == float(h["wh"]["p"]) / 4
    assert P[L.P["PC"], 2] == 0.925 and P[L.P["PH"], 2] == 1.025 and P[L.P["PW"], 2] == 0.575
    homes[5]["hems"]["sub_subhourly_steps"] = 6
    with pytest.raises(ValueError, match="share the hems settings"):
        pack_homes(homes)


def philox_np(ctr, key):
    """Philox4x32-10 in numpy (uint64 arithmetic), the generator of the device season noise."""
    c = [np.uint64(x) for x in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return [int(x) for x in c]


def test_philox_known_answers():
    """Random123 Philox4x32-10 known-answer vectors (kat_vectors)."""
    assert philox_np([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox_np([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert philox_np([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_synthetic_weather_shapes():
    from dragg_amd.community import synthetic_weather, upsample, tou_hourly
    assert upsample([1, 2, 3, 4], 4).tolist() == [1, 1, 2, 2, 3, 3, 4, 4]      # aggregator.py:140-145
    assert upsample([1, 2], 1).tolist() == [1]
    assert upsample([1, 2], 3).tolist() == [1, 1, 2]
    t = tou_hourly(24)
    assert t[8] == 0.07 and t[9] == 0.09 and t[20] == 0.09 and t[21] == 0.07   # peak overwritten
    oat, ghi, tou = synthetic_weather(3, 4, 30, seed=1)
    assert len(oat) == len(ghi) == len(tou) == 3 * 24 * 4
    assert np.all(oat == np.trunc(oat)) and ghi.min() >= 0
    assert tou[-1] == tou[29 * 4]                                              # forward fill


def test_synthetic_homes_schema():
    from dragg_amd.community import synthetic_homes
    from dragg_amd.mpc import pack_homes
    homes = synthetic_homes(50, seed=3, days=2)
    types = [h["type"] for h in homes]
    assert types.count("base") == 20 and types.count("pv_battery") == 10
    P, ty, dr, dm = pack_homes(homes)
    assert dr.shape == (48, 50) and dm["H"] == 24
    for h in homes:
        assert h["hvac"]["temp_in_min"] < h["hvac"]["temp_in_init"] < h["hvac"]["temp_in_max"]
        assert max(h["wh"]["draw_sizes"]) <= h["wh"]["tank_size"]


def test_reward_price_length_rule():
    """mpc_calc.py:353 raises unless len(rp) is 1 or >= H; the host mirrors that."""
    from dragg_amd.mpc import MPCBatch
    with pytest.raises(ValueError):
        MPCBatch.set_reward_price(type("B", (), {"H": 24, "device": "cpu", "dims": type("D", (), {})()})(),
                                  [0.0] * 4)


def test_size_queries_without_gpu(lib_path):
    """dragg_mpc_lds_bytes / dragg_mpc_workspace_bytes are host-only queries (no GPU needed)."""
    from dragg_amd import _lib as L
    lib = L.load()
    d = L.Dims(n_homes=100, horizon=24, sub_steps=6, dt=4, n_draw_hours=48, n_env=0, n_rp=1,
               int_mode=L.INT_ROUND, max_iter=0, check_every=0, discount=0.92)
    ws = lib.dragg_mpc_workspace_bytes(ctypes.byref(d))
    # u16 back-pointer per front label and stage (NB_CAP = 336), rounded to 256 B, then the
    # [N][8H] f64 stage-slot solutions and the [N] i32 list (+ its length) of the homes deferred to
    # the second launch, then (256-aligned) the second launch's back-pointer rows [512 blocks][H][NF_BIG =
    # 2048] u16, then (256-aligned) the [N] i32 list (+ length) of homes for the step-function DP launch and
    # (256-aligned) its storage: min(N, 16) block slots of ([2][2^20] f64 breakpoints / values,
    # [2][8 x 32768] i32 merge ids, [2][256][64] (x, v) LP rows)
    par = (100 * 24 * 336 * 2 + 255) // 256 * 256
    defer = par + 100 * 8 * 24 * 8
    big_off = (defer + 102 * 4 + 255) // 256 * 256
    nl_off = (big_off + 512 * 24 * 2048 * 2 + 255) // 256 * 256
    nr_off = (nl_off + 102 * 4 + 255) // 256 * 256
    # then (256-aligned) the [N] i32 list (+ length) the mid launch hands to the big one and
    # (256-aligned) the mid launch's back-pointer rows [2048 blocks][H][NF_MID = 384] u16
    slot = 2 * 2 ** 20 * 8 + 2 * 8 * 32768 * 4 + 2 * 256 * 64 * 16
    ml_off = (nr_off + 16 * slot + 255) // 256 * 256
    mr_off = (ml_off + 102 * 4 + 255) // 256 * 256
    # then (256-aligned) the front DP's LP cost-to-go rows [N][H + 1][64] (x, v)
    w_off = (mr_off + 2048 * 24 * 384 * 2 + 255) // 256 * 256
    assert ws == (w_off + 100 * 25 * 64 * 16 + 255) // 256 * 256
    # every intermediate above against the library's own map: this proves the order of the regions
    r = L.workspace_regions(d)
    assert (r["back_pointers"], r["solutions"], r["deferred"], r["big_rows"], r["steps_list"], r["steps_pools"],
            r["mid_list"], r["mid_rows"], r["w_rows"], r["cell_rows"], r["total"]) == \
        (0, par, defer, big_off, nl_off, nr_off, ml_off, mr_off, w_off, ws, ws)
    # the lag mode's side workspace: the lists and per-block scratch only, [defer, w_off)
    lib.dragg_mpc_side_workspace_bytes.restype = ctypes.c_int64
    assert lib.dragg_mpc_side_workspace_bytes(ctypes.byref(d)) == w_off - defer
    lds_direct = lib.dragg_mpc_lds_bytes(ctypes.byref(d))
    assert 0 < lds_direct <= 13 * 1024                 # the hot launch: >= 12 homes per CU at H = 24
    d.horizon = 48
    assert 0 < lib.dragg_mpc_lds_bytes(ctypes.byref(d)) <= 13 * 1024   # and at H = 48
    d.horizon = 24
    d.int_mode = L.INT_RELAX
    assert lib.dragg_mpc_workspace_bytes(ctypes.byref(d)) == 0
    assert set(L.workspace_regions(d).values()) == {0}
    assert lib.dragg_mpc_lds_bytes(ctypes.byref(d)) > lds_direct
    # round_lp: the back-pointers of its front DP alone, every other region starts at the total
    d.int_mode = L.INT_ROUND_LP
    assert lib.dragg_mpc_workspace_bytes(ctypes.byref(d)) == par
    r = L.workspace_regions(d)
    assert r.pop("back_pointers") == 0 and set(r.values()) == {par}
    # the map is refused where the size is
    regions = L.WorkspaceRegions()
    d.int_mode = 9
    assert lib.dragg_mpc_workspace_bytes(ctypes.byref(d)) < 0
    assert lib.dragg_mpc_workspace_regions_get(ctypes.byref(d), ctypes.byref(regions)) == \
        lib.dragg_mpc_workspace_bytes(ctypes.byref(d)) == -1
    d.int_mode = L.INT_ROUND
    assert lib.dragg_mpc_workspace_regions_get(ctypes.byref(d), None) == -1
    d.horizon = 160
    assert lib.dragg_mpc_workspace_regions_get(ctypes.byref(d), ctypes.byref(regions)) == \
        lib.dragg_mpc_workspace_bytes(ctypes.byref(d)) == -4
    with pytest.raises(L.DraggError):
        L.workspace_regions(d)
    # a list entry's home field holds every home index the library accepts, and no more
    d.horizon, d.n_homes = 24, L.LIST_HOME_MASK
    assert lib.dragg_mpc_workspace_bytes(ctypes.byref(d)) > 0
    d.n_homes = L.LIST_HOME_MASK + 1
    assert lib.dragg_mpc_workspace_bytes(ctypes.byref(d)) == -1
    d.n_homes = 100
    d.horizon = 400                                    # LP kernel's LDS is the binding limit
    d.int_mode = L.INT_RELAX
    assert lib.dragg_mpc_lds_bytes(ctypes.byref(d)) == -4


def _round_dims(L, N, H, S=6, n_rp=1, int_mode=None):
    return L.Dims(n_homes=N, horizon=H, sub_steps=S, dt=4, n_draw_hours=48, n_env=0, n_rp=n_rp,
                  int_mode=L.INT_ROUND if int_mode is None else int_mode, max_iter=0, check_every=0, discount=0.92)


# H -> hot launch LDS, workspace, workspace with a reward-price list (cell rows), side workspace; N = 100, S = 6,
# round mode: the values of the build before the LDS layouts were written once
PINNED_SIZES = {1: (9712, 314328576, 314328576, 314050048),
                17: (10736, 375864832, 379551232, 372770304),
                48: (12720, 495091200, 505126400, 486540800),
                96: (16928, 679699968, 699565568, 662701568),
                143: (23120, 860462848, 889954048, 835192320)}


# (N, H, cells) -> the workspace's region map (dragg_amd._lib.workspace_regions' values in order): the values
# of the Python mirror of the kernel's offset chain, before the library answered the query itself
PINNED_REGIONS = {
    (5, 24, False): (0, 80640, 88320, 88576, 50420224, 50420480, 147413760, 147414016, 185162752, 185290752,
                     185290752),
    (5, 24, True): (0, 80640, 88320, 88576, 50420224, 50420480, 147413760, 147414016, 185162752, 185290752,
                    185546752),
    (100, 48, False): (0, 3225600, 3532800, 3533312, 104196608, 104197120, 414575616, 414576128, 490073600,
                       495091200, 495091200),
    (100, 48, True): (0, 3225600, 3532800, 3533312, 104196608, 104197120, 414575616, 414576128, 490073600,
                      495091200, 505126400),
    (1000, 96, False): (0, 64512000, 70656000, 70660096, 271986688, 271990784, 582369280, 582373376, 733368320,
                        832696320, 832696320),
    (1000, 96, True): (0, 64512000, 70656000, 70660096, 271986688, 271990784, 582369280, 582373376, 733368320,
                       832696320, 1031352320)}


@pytest.mark.parametrize("H", sorted(PINNED_SIZES))
def test_pinned_size_queries(lib_path, H):
    from dragg_amd import _lib as L
    lib = L.load()
    d, dc = _round_dims(L, 100, H), _round_dims(L, 100, H, n_rp=H)
    got = (lib.dragg_mpc_lds_bytes(ctypes.byref(d)), lib.dragg_mpc_workspace_bytes(ctypes.byref(d)),
           lib.dragg_mpc_workspace_bytes(ctypes.byref(dc)), lib.dragg_mpc_side_workspace_bytes(ctypes.byref(d)))
    assert got == PINNED_SIZES[H]


def _largest_horizon(L, S, int_mode):
    lib = L.load()
    ok = [H for H in range(1, 200) if lib.dragg_mpc_lds_bytes(ctypes.byref(_round_dims(L, 100, H, S=S, int_mode=int_mode))) > 0]
    assert ok == list(range(1, len(ok) + 1))             # accepted up to a largest horizon, none past it
    return ok[-1]


def test_largest_accepted_horizons(lib_path):
    from dragg_amd import _lib as L
    lib = L.load()
    for S in (1, 4, 6, 7, 8, 12, 15):
        assert _largest_horizon(L, S, L.INT_ROUND) == 159
        assert lib.dragg_mpc_lds_bytes(ctypes.byref(_round_dims(L, 100, 160, S=S))) == -4
    assert _largest_horizon(L, 6, L.INT_RELAX) == 69
    assert _largest_horizon(L, 6, L.INT_ROUND_LP) == 69


@pytest.mark.parametrize("N,H", [(5, 24), (100, 48), (1000, 96)])
@pytest.mark.parametrize("cells", [False, True])
def test_workspace_regions_match_the_library(lib_path, N, H, cells):
    """The library's region map (dragg_amd._lib.workspace_regions) against its pinned numbers and the library's
    two size queries (test_size_queries_without_gpu proves the order of the regions from literal arithmetic,
    tests/test_gpu_workspace_regions.py reads the lists)."""
    from dragg_amd import _lib as L
    lib = L.load()
    d = _round_dims(L, N, H, n_rp=H if cells else 1)
    r = L.workspace_regions(d)
    assert tuple(r.values()) == PINNED_REGIONS[N, H, cells]
    assert r["total"] == lib.dragg_mpc_workspace_bytes(ctypes.byref(d))
    assert r["w_rows"] - r["deferred"] == lib.dragg_mpc_side_workspace_bytes(ctypes.byref(d))
    keys = list(r)
    assert keys == ["back_pointers", "solutions", "deferred", "big_rows", "steps_list", "steps_pools", "mid_list",
                    "mid_rows", "w_rows", "cell_rows", "total"]
    assert all(r[a] <= r[b] for a, b in zip(keys, keys[1:]))
    assert all(r[k] % 256 == 0 for k in keys[keys.index("deferred") + 1:-1])
    assert r["solutions"] % 256 == 0


def test_side_grid_clamped_to_scratch_slots(lib_path, monkeypatch):
    """DRAGG_SIDE_GRID entries are clamped to each side launch's per-block scratch: the
    step-function launch's narrow_slots(N) = min(N, 16) pools, the big launch's 512 and the mid launch's
    2,048 rows, and to one block per home."""
    from dragg_amd import _lib as L
    d = L.Dims(n_homes=1000, horizon=48, sub_steps=6, dt=4, n_draw_hours=48, n_env=0, n_rp=1,
               int_mode=L.INT_ROUND, max_iter=0, check_every=0, discount=0.92)
    try:
        monkeypatch.delenv("DRAGG_SIDE_GRID", raising=False)
        L.reload_knobs()
        assert L.side_grid(d) == [16, 16, 16, 2]
        monkeypatch.setenv("DRAGG_SIDE_GRID", "5000,4096,9999,32")
        L.reload_knobs()
        assert L.side_grid(d) == [1000, 1000, 512, 16]
        d.n_homes = 3000
        assert L.side_grid(d) == [3000, 2048, 512, 16]
        d.n_homes = 5
        assert L.side_grid(d) == [5, 5, 5, 5]
        monkeypatch.setenv("DRAGG_SIDE_GRID", "0,-3,1,1")
        L.reload_knobs()
        assert L.side_grid(d) == [5, 5, 1, 1]
    finally:
        monkeypatch.delenv("DRAGG_SIDE_GRID", raising=False)
        L.reload_knobs()


def test_entry_points_refuse_bad_arguments(lib_path):
    """The refusal table of the solve entry points: every call below is refused (or is a zero-home
    no-op) before any HIP call, so it runs without a GPU on dummy pointers.  One thing is knocked out
    of a valid call per case.  (Only refused calls and no-ops: a call the library accepts would launch
    kernels on these addresses.)"""
    from dragg_amd import _lib as L
    lib = L.load()
    E_ARG, E_HORIZON, DUMMY = -1, -4, 0x1000

    def ptrs(cls):
        return {f: DUMMY for f, ty in cls._fields_ if ty is L.c_dp}

    def call(entry, dims={}, prob={}, hsh={}, out={}, ex={}, lag={}, t=0):
        d = L.Dims(**{**dict(n_homes=4, horizon=24, sub_steps=6, dt=4, n_draw_hours=48, n_env=200, n_rp=1,
                             int_mode=L.INT_ROUND), **dims})
        p, h, o = L.Problem(**{**ptrs(L.Problem), **prob}), L.Hash(**{**ptrs(L.Hash), **hsh}), L.Out(**{**ptrs(L.Out), **out})
        e, lg = L.Explicit(**{**ptrs(L.Explicit), **ex}), L.Lag(**{**ptrs(L.Lag), **lag})
        r = ctypes.byref
        if entry == "step":
            return lib.dragg_mpc_step(r(d), r(p), r(h), r(o), t, None, None)
        if entry in ("step_main", "step_side"):
            return getattr(lib, "dragg_mpc_" + entry)(r(d), r(p), r(h), r(o), t, r(lg), None)
        if entry == "solve_explicit":
            return lib.dragg_mpc_solve_explicit(r(d), r(p), r(e), r(h), r(o), None)
        assert entry == "lag_reset"
        return lib.dragg_mpc_lag_reset(r(d), r(lg), t, None)

    table = []          # (entry, what is knocked out, expected code)
    for f in ("params", "home_type", "draw_hourly", "oat", "ghi", "tou", "reward_price", "workspace"):
        table.append(("step", dict(prob={f: None}), E_ARG))
    for f in ("vals", "fc"):
        table.append(("step", dict(hsh={f: None}), E_ARG))
    for f in ("status", "iters", "obj", "relax_obj"):
        table.append(("step", dict(out={f: None}), E_ARG))
    table += [("step", dict(t=-1), E_ARG), ("step", dict(dims=dict(n_rp=5)), E_ARG),
              ("step", dict(dims=dict(n_env=24)), E_ARG), ("step", dict(dims=dict(sub_steps=16)), E_ARG),
              ("step", dict(dims=dict(horizon=160)), E_HORIZON), ("step", dict(dims=dict(n_homes=0)), 0)]
    for entry in ("step_main", "step_side"):
        for f in ("clock", "skipped", "narrow"):
            table.append((entry, dict(lag={f: None}), E_ARG))
        table += [(entry, dict(dims=dict(n_groups=2)), E_ARG), (entry, dict(dims=dict(int_mode=L.INT_RELAX)), E_ARG),
                  (entry, dict(t=2 ** 30 - 1), E_ARG), (entry, dict(prob=dict(workspace=None)), E_ARG),
                  (entry, dict(dims=dict(n_homes=0)), 0)]
    table.append(("step_side", dict(lag=dict(side_workspace=None)), E_ARG))
    for f, _ in L.Explicit._fields_:
        table.append(("solve_explicit", dict(ex={f: None}), E_ARG))
    table += [("solve_explicit", dict(dims=dict(n_groups=2)), E_ARG), ("solve_explicit", dict(dims=dict(n_homes=0)), 0)]
    table += [("lag_reset", dict(lag=dict(clock=None)), E_ARG), ("lag_reset", dict(dims=dict(n_groups=2)), E_ARG),
              ("lag_reset", dict(t=2 ** 30 - 1), E_ARG)]
    assert len(table) == 20 + 2 * 8 + 1 + 12 + 3
    got = [(entry, knock, call(entry, **knock)) for entry, knock, _ in table]
    assert got == table


def test_stale_library_refused(tmp_path, monkeypatch, lib_path):
    """The library carries its sources' sha-256 (dragg_amd/build.py); the loader refuses one whose stamp
    is not the sources' beside it."""
    from dragg_amd import _lib as L, build as B
    assert B.stamp_of(lib_path) == B.source_hash()
    assert not B.needs_build()
    L.check_stamp(lib_path)                           # the fresh build passes
    assert ctypes.CDLL(lib_path).dragg_mpc_source_hash  # exported
    stale = tmp_path / "stale.so"
    data = open(lib_path, "rb").read().replace(B.STAMP_PREFIX + B.source_hash().encode(),
                                               B.STAMP_PREFIX + b"0" * 64)
    stale.write_bytes(data)
    monkeypatch.setattr(B, "OUT", str(stale))
    monkeypatch.delenv("DRAGG_LIB", raising=False)
    assert B.needs_build()
    with pytest.raises(L.DraggError, match="stale"):
        L.check_stamp(str(stale))


def test_solver_name_plug_point():
    """home['hems']['solver'] (mpc_calc.py:141-145): the MILP backends -- and an unknown name,
    which the reference replaces by GLPK_MI -- select the exact MILP path; ECOS, which cvxpy
    refuses on an integer problem (every solve falls back, mpc_calc.py:450-454), selects the
    always-fallback mode; the build's own int_mode names select themselves."""
    from dragg_amd.calc import int_mode_for
    for name, mode in (("GLPK_MI", "round"), ("GUROBI", "round"), ("ECOS", "fail"), ("nonsense", "round"),
                       ("relax", "relax"), ("round_lp", "round_lp"), ("fail", "fail")):
        assert int_mode_for({"hems": {"solver": name}}) == mode
    assert int_mode_for({"hems": {}}) == "round"


def test_mpccalc_needs_a_community():
    """MPCCalc(home) without a community attaches to the default one; with none it raises."""
    from dragg_amd.calc import Community, MPCCalc
    Community._default = None
    with pytest.raises(RuntimeError):
        MPCCalc({"name": "h", "type": "base", "hems": {"solver": "GLPK_MI"}})
