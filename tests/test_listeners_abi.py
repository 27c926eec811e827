"""Stream listeners in the C ABI: the header declares them, the ctypes binding matches, the
library exports them (CPU; no device is touched)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ewk_stream_listeners_set", "ewk_stream_listeners", "ewk_get_listener_state"]


def _code():
    src = open(os.path.join(ROOT, "include", "ewk.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_listener_abi():
    code = _code()
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
    assert re.search(r"#define\s+EWK_LISTENERS_MAX\s+16\b", code)
    assert re.search(r"#define\s+EWK_EV_LISTENER_SHIFT\s+16\b", code)
    assert re.search(r"#define\s+EWK_EV_LISTENER\(flags\)\s+\(\(\(flags\)\s*>>\s*EWK_EV_LISTENER_SHIFT\)\s*&\s*15\)", code)
    assert re.search(r"#define\s+EWK_ABI_VERSION\s+4\b", code)      # additive: the version stays
    m = re.search(r"typedef struct ewk_listener\s*\{(.*?)\}\s*ewk_listener;", code, flags=re.S)
    assert m, "struct ewk_listener"
    assert re.findall(r"int32_t\s+([a-z_]+)\s*;", m.group(1)) == ["profile", "word"]
    # ewk_event keeps its layout
    ev = re.search(r"typedef struct ewk_event\s*\{(.*?)\}\s*ewk_event;", code, flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*;", ev) == ["stream", "length", "tick", "ring_start", "time", "score", "match",
                                                   "flags"]


def test_binding_matches_the_header():
    from easywakeword_amd import _lib
    assert ctypes.sizeof(_lib.EwkListener) == 8
    assert _lib.EwkListener._fields_ == [("profile", ctypes.c_int32), ("word", ctypes.c_int32)]
    assert ctypes.sizeof(_lib.EwkEvent) == 48
    assert (_lib.EWK_LISTENERS_MAX, _lib.EWK_EV_LISTENER_SHIFT) == (16, 16)
    lib = _lib.load()
    for name in CALLS:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)          # exported
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, name
    assert len(lib.ewk_stream_listeners_set.argtypes) == 6
    assert len(lib.ewk_stream_listeners.argtypes) == 5
    assert len(lib.ewk_get_listener_state.argtypes) == 4
    assert lib.ewk_abi_version() == 4


def test_listener_bits_of_the_flags():
    import numpy as np
    from easywakeword_amd import _lib
    flags = (5 << 16) | _lib.EWK_EV_BANK | (7 << 8) | 1
    assert _lib.event_listener(flags) == 5
    assert _lib.event_best_template(flags) == 7
    arr = np.array([flags, 1, 15 << 16], np.int32)
    assert _lib.event_listener(arr).tolist() == [5, 0, 15]
    assert _lib.event_best_template(arr).tolist() == [7, 0, 0]


def test_null_engine_is_refused_without_a_device():
    from easywakeword_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int32(0)
    assert lib.ewk_stream_listeners_set(None, None, 0, None, None, 0) == _lib.EWK_EINVAL
    assert b"engine is NULL" in lib.ewk_last_error()
    assert lib.ewk_stream_listeners(None, 0, None, 0, ctypes.byref(n)) == _lib.EWK_EINVAL
