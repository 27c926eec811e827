"""Stream lifecycle calls (CPU): the five prototypes of include/ewk.h, their names in
_lib.EXPORTS, and the ABI version they were added under (no struct changed: still 4)."""
import os
import re

from easywakeword_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "ewk_push_streams":
        "int ewk_push_streams(ewk_engine* e, const int32_t* streams, int32_t n, const float* pcm, "
        "int64_t stride, int64_t tick_stride, int32_t n_ticks, int32_t flags);",
    "ewk_push_streams_pcm16":
        "int ewk_push_streams_pcm16(ewk_engine* e, const int32_t* streams, int32_t n, const int16_t* pcm, "
        "int64_t stride, int64_t tick_stride, int32_t n_ticks, int32_t flags);",
    "ewk_reset_stream_list":
        "int ewk_reset_stream_list(ewk_engine* e, const int32_t* streams, int32_t n);",
    "ewk_stream_ticks":
        "int ewk_stream_ticks(ewk_engine* e, const int32_t* streams, int32_t n, int64_t* out);",
    "ewk_stream_bank_assign":
        "int ewk_stream_bank_assign(ewk_engine* e, const int32_t* streams, int32_t n, const int32_t* words);",
}


def _header():
    src = open(os.path.join(ROOT, "include", "ewk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"\s+", " ", src)


def test_prototypes_in_header():
    h = _header()
    for name, proto in PROTOTYPES.items():
        assert proto in h, name


def test_names_exported():
    for name in PROTOTYPES:
        assert name in _lib.EXPORTS, name


def test_abi_version_still_4():
    m = re.search(r"#define\s+EWK_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "ewk.h")).read())
    assert m and int(m.group(1)) == 4
