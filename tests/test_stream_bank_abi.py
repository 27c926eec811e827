"""The stream bank's additions to the C ABI (CPU): the event flag macros of include/ewk.h and
their Python mirrors, the best-template helper, and the unchanged ABI version."""
import os
import re

import numpy as np

from easywakeword_amd import _lib

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "ewk.h")


def _define(name):
    src = open(HEADER).read()
    m = re.search(r"^#define\s+%s\s+\(?(-?\d+)\)?" % re.escape(name), src, flags=re.M)
    assert m, name
    return int(m.group(1))


def test_flag_macros_equal_the_headers():
    for name in ("EWK_EV_SKIPPED", "EWK_EV_RESCORED", "EWK_EV_BANK", "EWK_EV_BEST_SHIFT"):
        assert getattr(_lib, name) == _define(name), name
    assert _lib.EWK_EV_BANK == 4 and _lib.EWK_EV_BEST_SHIFT == 8
    # the three flag bits and the best-template field do not overlap
    field = 63 << _lib.EWK_EV_BEST_SHIFT
    assert field & (_lib.EWK_EV_SKIPPED | _lib.EWK_EV_RESCORED | _lib.EWK_EV_BANK) == 0
    # EWK_EV_BEST(flags) is ((flags) >> EWK_EV_BEST_SHIFT) & 63
    src = open(HEADER).read()
    assert re.search(r"#define\s+EWK_EV_BEST\(flags\)\s+\(\(\(flags\)\s*>>\s*EWK_EV_BEST_SHIFT\)\s*&\s*63\)", src)


def test_event_best_template_round_trips():
    low = _lib.EWK_EV_BANK | _lib.EWK_EV_RESCORED
    for best in range(64):
        flags = low | (best << _lib.EWK_EV_BEST_SHIFT)
        assert _lib.event_best_template(flags) == best
        assert flags & 0xFF == low
    arr = (np.arange(64, dtype=np.int32) << _lib.EWK_EV_BEST_SHIFT) | _lib.EWK_EV_BANK
    assert np.array_equal(_lib.event_best_template(arr), np.arange(64))


def test_abi_version_is_still_4_and_the_calls_are_declared():
    assert _define("EWK_ABI_VERSION") == 4
    assert {"ewk_stream_bank_enable", "ewk_stream_bank_disable"} <= set(_lib.EXPORTS)
    src = open(HEADER).read()
    assert re.search(r"int\s+ewk_stream_bank_enable\(ewk_engine\*\s*e,\s*const int32_t\*\s*stream_word\);", src)
    assert re.search(r"int\s+ewk_stream_bank_disable\(ewk_engine\*\s*e\);", src)
