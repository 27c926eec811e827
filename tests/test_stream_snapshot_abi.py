"""Stream snapshots in the C ABI: the new names are in the header, the binding and the library,
the ABI version is unchanged, and the two structs have the header's layout (CPU)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ewk_snapshot_plan", "ewk_snapshot_info", "ewk_export_streams", "ewk_import_streams"]


def header():
    return open(os.path.join(ROOT, "include", "ewk.h")).read()


def test_names_in_header_binding_and_library():
    from easywakeword_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)


def test_abi_version_stays_4():
    from easywakeword_amd import _lib
    assert re.search(r"#define\s+EWK_ABI_VERSION\s+4\b", header())
    assert _lib.load().ewk_abi_version() == 4


def header_define(name):
    m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, header())
    assert m, name
    return int(m.group(1), 0)


def test_struct_layouts_match_header():
    from easywakeword_amd import _lib
    n_sec = header_define("EWK_SNAP_SECTIONS")
    n_lsn = header_define("EWK_LISTENERS_MAX")
    assert (n_sec, n_lsn) == (_lib.EWK_SNAP_SECTIONS, _lib.EWK_LISTENERS_MAX)
    assert len(_lib.SNAP_SECTION_NAMES) == n_sec
    # ewk_snapshot_layout: magic, version, 8 int32, 2 int64, a double, the sections, 2 x 8 bytes
    assert ctypes.sizeof(_lib.EwkSnapshotSection) == 16
    assert ctypes.sizeof(_lib.EwkSnapshotLayout) == 2 * 4 + 8 * 4 + 2 * 8 + 8 + n_sec * 16 + 2 * 8 == 208
    # ewk_stream_meta: magic, version, tick, record_bytes, fingerprint, 4 int32, the listener rows
    assert ctypes.sizeof(_lib.EwkStreamMeta) == 2 * 4 + 3 * 8 + 4 * 4 + n_lsn * 8 == 176
    assert _lib.STREAM_META_DTYPE.itemsize == ctypes.sizeof(_lib.EwkStreamMeta)
    for name, _ in _lib.EwkStreamMeta._fields_:
        assert _lib.STREAM_META_DTYPE.fields[name][1] == getattr(_lib.EwkStreamMeta, name).offset, name
    assert re.search(r"ewk_snapshot_layout\s*\{\s*/\*\s*208 bytes", header())
    assert re.search(r"ewk_stream_meta\s*\{\s*/\*\s*176 bytes", header())
    assert header_define("EWK_SNAPSHOT_MAGIC") == _lib.EWK_SNAPSHOT_MAGIC
    assert header_define("EWK_SNAPSHOT_VERSION") == _lib.EWK_SNAPSHOT_VERSION
    assert np.zeros(1, _lib.STREAM_META_DTYPE)["listeners"].shape == (1, n_lsn, 2)
