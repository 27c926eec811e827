"""Detector profiles in the C ABI: the header declares them, the ctypes binding matches, the
library exports them (CPU; no device is touched)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ewk_default_detector_profile", "ewk_detector_profiles_set", "ewk_detector_profiles_info",
         "ewk_detector_profile_get", "ewk_stream_profile_assign", "ewk_stream_profiles"]
FIELDS = ["pre_speech_silence", "speech_duration_min", "speech_duration_max", "post_speech_silence", "padding",
          "max_segment_seconds", "reentry_timeout"]


def _header():
    return open(os.path.join(ROOT, "include", "ewk.h")).read()


def test_header_declares_the_profile_abi():
    src = _header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in CALLS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
    assert re.search(r"#define\s+EWK_PROFILE_MAX\s+65536\b", code)
    assert re.search(r"#define\s+EWK_ABI_VERSION\s+4\b", code)
    m = re.search(r"typedef struct ewk_detector_profile\s*\{(.*?)\}\s*ewk_detector_profile;", code, flags=re.S)
    assert m, "struct ewk_detector_profile"
    body = m.group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == FIELDS     # seven doubles, in ewk_config's order
    assert "int" not in body and "float" not in body


def test_binding_matches_the_header():
    from easywakeword_amd import _lib
    assert ctypes.sizeof(_lib.EwkDetectorProfile) == 56
    assert [f for f, _ in _lib.EwkDetectorProfile._fields_] == FIELDS
    assert all(t is ctypes.c_double for _, t in _lib.EwkDetectorProfile._fields_)
    assert _lib.EWK_PROFILE_MAX == 65536
    lib = _lib.load()
    for name in CALLS:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)          # exported
        assert fn.argtypes is not None and len(fn.argtypes) >= 2, name
    assert lib.ewk_default_detector_profile.restype is None
    assert all(getattr(lib, n).restype is ctypes.c_int for n in CALLS[1:])
    assert lib.ewk_abi_version() == 4


def test_reference_defaults_without_an_engine():
    from easywakeword_amd import _lib
    p = _lib.EwkDetectorProfile()
    _lib.load().ewk_default_detector_profile(None, ctypes.byref(p))
    assert [getattr(p, f) for f in FIELDS] == [0.8, 0.3, 2.0, 0.4, 0.05, 3.0, 0.0]
    c = _lib.default_config()
    assert [getattr(p, f) for f in FIELDS] == [getattr(c, f) for f in FIELDS]
