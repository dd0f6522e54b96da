"""The workspace guard's bookkeeping, without a device: the slot list the library exports (one list for the enum and the names,
abi_common.hpp) and the coverage of tests/test_gpu_ws_guard.py -- every slot is declared by a case there, or excluded here by name
with its reason."""
import ctypes

from pilot_amd import _lib, engine
from test_gpu_ws_guard import CASES

# slots no single-device engine call on the calling thread can reach: name -> reason
EXCLUDED = {}


def test_slot_names():
    L = _lib.load()
    n = L.pilot_ot_ws_slot_count()
    names = engine.ws_slot_names()
    assert n > 100 and len(names) == n and len(set(names)) == n
    assert all(name.startswith("WS_") and name == name.upper() for name in names)
    assert "WS_GS_PART" in names and "WS_SLOTS" not in names
    for bad in (-1, n, n + 1, 2 ** 31 - 1, -2 ** 31):
        assert L.pilot_ot_ws_slot_name(bad) is None


def test_report_without_a_device_or_a_guarded_hand_out():
    """nothing was handed out under guard: the report makes no HIP call and reads clean, with and without the outputs"""
    assert engine.ws_guard_report() == (set(), None)
    assert engine.ws_guard_report(reset=True) == (set(), None)
    assert _lib.load().pilot_ot_ws_guard_report(None, None, None, None, 0) == _lib.OK


def test_every_slot_is_declared_by_a_case_or_excluded():
    names = set(engine.ws_slot_names())
    declared = set()
    for case, (run, slots) in CASES.items():
        assert callable(run) and slots and len(set(slots)) == len(slots), case
        stale = set(slots) - names
        assert not stale, "%s declares slots the library does not have: %s" % (case, sorted(stale))
        declared |= set(slots)
    assert set(EXCLUDED) <= names, "EXCLUDED names slots the library does not have: %s" % sorted(set(EXCLUDED) - names)
    assert all(isinstance(r, str) and r for r in EXCLUDED.values())
    assert not declared & set(EXCLUDED), "excluded and declared: %s" % sorted(declared & set(EXCLUDED))
    gap = names - declared - set(EXCLUDED)
    assert not gap, "slots no case of tests/test_gpu_ws_guard.py declares: %s" % sorted(gap)
