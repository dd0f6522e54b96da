"""The stream kernel's LDS layout and the pass plan of the Sinkhorn grid call (pilot_amd/csrc/sinkhorn_layout.hpp), checked on
the host alone: tests/sinkhorn_layout_dump.cpp includes only that header, is built with the host C++ compiler and prints one line
per case.  The kernels address LDS by the same function, so an offset that leaves the block shows here, not on a device.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _num(v):
    try:
        return int(v)
    except ValueError:
        try:
            return float(v)
        except ValueError:
            return v


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = tmp_path_factory.mktemp("layout") / "sinkhorn_layout_dump"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "sinkhorn_layout_dump.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = {"C": [], "L": [], "P": []}
    for line in out.splitlines():
        kind, _, rest = line.partition(" ")
        rows[kind].append({k: _num(v) for k, v in (f.split("=", 1) for f in rest.split())})
    assert len(rows["C"]) == 1 and len(rows["L"]) > 500 and len(rows["P"]) > 20000
    return rows["C"][0], rows["L"], rows["P"]


def _check_regions(c, r, pre, ts):
    """offsets ascend (so the regions, each as long as the gap to the next, do not overlap), the last one ends at the byte count, and
    what a lane reads 16 bytes at a time starts on a 16-byte boundary"""
    off = [r[pre + k] for k in ("table", "tail", "rings", "park", "hb", "end")]
    assert off[0] > 0 and all(a <= b for a, b in zip(off, off[1:])), r
    assert r[pre + "end"] * ts == r[pre + "lbytes"], r
    assert (r[pre + "rings"] * ts) % 16 == 0 and (r[pre + "park"] * ts) % 16 == 0 and (r[pre + "slot"] * ts) % 16 == 0, r
    assert r[pre + "slot"] == 2 * r[pre + "panel"] + 4, r
    # the solo workgroups' lines (one value per lane for each wave, at the start of the block) lie inside it
    assert c["waves"] * c["wave"] <= r[pre + "end"], r


def test_layout_regions_ascend_and_end_at_the_byte_count(dump):
    c, layouts, _ = dump
    for r in layouts:
        ts = 4 * r["w"]
        _check_regions(c, r, "", ts)
        KP = 16 * r["RT"]
        assert r["tail"] - r["table"] == KP, r
        # the rings are `ring` slots for each wave; the hand-over buffers exist in the fast kernels only
        assert r["park"] - r["rings"] == c["waves"] * r["ring"] * r["slot"], r
        assert (r["end"] - r["hb"]) * ts == (0 if r["track"] else c["waves"] * c["handover"] * 4), r
        split = r["cfg"] in (c["cfg_s32"], c["cfg_h32"])
        assert (r["hb"] > r["park"]) == (split and not r["track"] and r["RT"] <= 4), r
        assert (r["rings"] > r["tail"]) == (r["tv"] > 0 and not split), r


def _parent_host_bytes(c, r):
    """What the host reserved per pass before the layout had one statement (fixed part and bytes of one slot in every wave's ring),
    restated from its formulas: the values that decide ring and resident workgroups and must not move."""
    cfg, RT, K, sym = r["cfg"], r["RT"], r["K"], r["sym"]
    half, split, f64 = cfg == c["cfg_h32"], cfg in (c["cfg_s32"], c["cfg_h32"]), cfg == c["cfg_f64"]
    ts, KP, W, nf = (8 if f64 else 4), 16 * RT, c["waves"], (1 if sym else 2)
    kb = (RT + 1) // 2
    form = lambda np_: np_ * kb * RT * 64 * 4
    form_cfg = form(2) if half else (form(3) if split else KP * KP)
    hb = W * c["handover"] * 4
    tv = r["f_tv"]
    fixed = nf * form_cfg * ts + KP * ts + hb + nf * tv * ((RT - 1) * 4 + 1) * 64 * 2 * ts
    slot = (2 * KP + 4) * ts
    park = split and RT <= 4
    slot_fast = (2 * (2 * kb * 16) + 4) * ts if half else slot
    park_bytes = W * (2 * kb * 4 if half else RT * 4) * 64 * ts if park else 0
    fixed_t = fixed
    if half:
        fixed_t = nf * form(3) * ts + KP * ts + hb
    if r["mixed"]:
        fixed_t = nf * form_cfg * ts * 2 + KP * ts + hb
    fixed64 = nf * KP * KP * 8 + KP * 8
    return {"f_": (fixed + park_bytes, W * slot_fast), "t_": (fixed_t, W * slot), "d_": (fixed64, W * (2 * KP + 4) * 8)}


def _parent_stream_lds(c, fixed, slots, want):
    while True:
        budget = c["lds_bytes"] // want
        ring = (budget - fixed) // slots if budget > fixed else 0
        if ring >= 4 or want == 1:
            ring = min(ring, c["ring_max"])
            return fixed + slots * ring, ring, want
        want -= 1


def test_plans_fit_lds_and_keep_the_reserved_bytes(dump):
    c, _, plans = dump
    LDS = c["lds_bytes"]
    n_enotsup = 0
    for r in plans:
        stream = [pre for pre in ("f_", "t_", "d_") if r[pre + "run"] and not r[pre + "quad"] and not r[pre + "solo64"]]
        parent = _parent_host_bytes(c, r)
        for pre in stream:
            assert (r[pre + "fixed"], r[pre + "slots"]) == parent[pre], (pre, r)
        too_big = any(r[pre + "fixed"] + r[pre + "slots"] > LDS for pre in stream)
        assert (r["rc"] == c["enotsup"]) == too_big and r["rc"] in (0, c["enotsup"]), r
        assert (r["msg"] == "set") == too_big, r
        if too_big:
            n_enotsup += 1
            continue
        for pre in stream:
            ts = 4 * r[pre + "w"]
            _check_regions(c, r, pre, ts)
            assert r[pre + "lbytes"] + r[pre + "inherited"] == r[pre + "bytes"] <= LDS, (pre, r)
            assert 1 <= r[pre + "ring"] <= c["ring_max"] and (r[pre + "ring"] >= 4 or r[pre + "wpc"] == 1), (pre, r)
            assert r[pre + "wpc"] >= 1 and r[pre + "wpc"] * r[pre + "bytes"] <= LDS, (pre, r)
        for pre in ("f_", "t_", "d_"):
            if r[pre + "run"]:
                assert r[pre + "wgs"] >= 1, (pre, r)
        # every launch's ring and resident workgroups are what the parent's search gave for the parent's bytes and occupancy: the fast
        # kernel's as instantiated (two workgroups at K <= 4 in the fp16-split configuration), the bf16-split or plain tracking
        # kernel's with live1 / the tracking tail rows, the f64 tracking kernel's
        want = {"f_": 2 if r["cfg"] == c["cfg_h32"] and r["K"] <= 4 and r["mw"] > 2 else r["mw"], "t_": r["mw_t"], "d_": r["mw_d"]}
        for pre in stream:
            assert (r[pre + "bytes"], r[pre + "ring"], r[pre + "wpc"]) == _parent_stream_lds(c, *parent[pre], want[pre]), (pre, r)
    assert 0 < n_enotsup < len(plans) // 4


def test_plan_variant_rules(dump):
    c, _, plans = dump
    F32, F64, S32, H32 = c["cfg_f32"], c["cfg_f64"], c["cfg_s32"], c["cfg_h32"]
    seen = set()
    for r in plans:
        RT, K, split = r["RT"], r["K"], r["cfg"] in (S32, H32)
        n_last = K - 16 * (RT - 1)
        for pre in ("f_", "t_", "d_"):
            if r[pre + "tv"] > 0:
                assert r[pre + "cfg"] in (F32, F64) and 2 <= RT <= 7 and n_last <= 4 and not r["debug"] & c["no_tail"], (pre, r)
                assert r[pre + "tv"] == (1 if n_last <= 2 else 2), (pre, r)
            if r[pre + "live1"]:
                assert r[pre + "cfg"] in (S32, H32) and 2 <= RT <= 4 and n_last <= 4, (pre, r)
        assert r["t_tv"] in (0, r["f_tv"]) and r["d_tv"] == 0 and r["d_cfg"] == F64, r
        assert r["f_cfg"] == r["cfg"] and r["t_cfg"] == (S32 if split else r["cfg"]), r
        assert not r["f_track"] and r["t_track"] and r["d_track"], r
        assert r["t_bands"] == (2 if r["mixed"] else 1) and r["f_bands"] == 1 and r["d_bands"] == 1, r
        if r["rc"]:
            continue
        assert r["t_run"] == 1, r
        # every pair goes through the tracking kernel at once: small reg under AUTO, and the bf16-split configuration from max(M)/reg = 24
        track_all = bool(r["mixed"]) or (r["cfg"] == S32 and r["mcr"] > 24 and not r["debug"] & c["no_track_all"])
        assert r["f_run"] == (not track_all) and (r["t_len"] == -1) == track_all, r
        assert r["d_run"] == (bool(r["mixed"]) or (split and r["mcr"] > 12)), r
        assert r["f_quad"] == (r["cfg"] == H32 and bool(r["sym"]) and 113 <= K <= 128 and not r["no_quad"]), r
        if r["d_run"]:
            assert r["d_solo64"] == (bool(r["sym"]) and K <= 64), r
        solo = r["f_solo_blocks"] > 0
        assert solo == bool(r["mode"] & 2), r
        if solo:
            full_tiles, wave_slots = (r["N"] * r["N"] + 15) // 16, r["n_cu"] * r["mw"] * c["waves"]
            assert r["sym"] and RT <= 4 and full_tiles < 3 * wave_slots and r["solo_rule"] and r["f_run"] and not r["debug"] & c["no_solo"], r
            assert r["f_solo_blocks"] == min(r["n_cu"], (r["n_rows"] + c["waves"] - 1) // c["waves"]), r
        seen.add((solo, r["f_tv"] > 0, bool(r["f_live1"]), bool(r["f_quad"]), bool(r["d_solo64"] and r["d_run"]), track_all))
    # the grid of cases reaches every kind of variant
    for i in range(6):
        assert {s[i] for s in seen} == {False, True}, (i, seen)
