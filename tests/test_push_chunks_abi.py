"""Packet ingest in the C ABI: the header declares the four calls, the ctypes binding matches, the
library exports them (CPU; no device is touched)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ewk_push_chunks", "ewk_push_chunks_pcm16", "ewk_stream_pending", "ewk_chunk_plan"]


def _code():
    src = open(os.path.join(ROOT, "include", "ewk.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_chunk_abi():
    code = _code()
    push = (r"\(ewk_engine\* e, const int32_t\* streams, int32_t n, const {}\* pcm, int64_t n_pcm, "
            r"const int64_t\* offsets, const int32_t\* counts, int32_t flags\);")
    assert re.search(r"\bint ewk_push_chunks" + push.format("float"), code)
    assert re.search(r"\bint ewk_push_chunks_pcm16" + push.format("int16_t"), code)
    assert re.search(r"\bint ewk_stream_pending\(ewk_engine\* e, const int32_t\* streams, int32_t n, int32_t\* out\);",
                     code)
    assert re.search(r"\bint ewk_chunk_plan\(int32_t in_block, int32_t n, const int32_t\* pending, "
                     r"const int32_t\* counts, int32_t\* ticks, int32_t\* new_pending, int32_t\* order, "
                     r"int32_t\* n_ticking, int32_t\* group_ticks, int32_t\* group_first, int32_t group_cap, "
                     r"int32_t\* n_groups\);", code)
    assert re.search(r"#define EWK_CHUNK_MAX_TICKS 64\b", code)
    assert re.search(r"#define EWK_ABI_VERSION 4\b", code)      # additive: the version stays


def test_binding_matches_the_header():
    from easywakeword_amd import _lib
    assert _lib.EWK_CHUNK_MAX_TICKS == 64
    lib = _lib.load()
    for name in CALLS:
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)          # exported
        assert fn.restype is ctypes.c_int and fn.argtypes is not None, name
    assert len(lib.ewk_push_chunks.argtypes) == 8
    assert len(lib.ewk_push_chunks_pcm16.argtypes) == 8
    assert len(lib.ewk_stream_pending.argtypes) == 4
    assert len(lib.ewk_chunk_plan.argtypes) == 12
    assert lib.ewk_abi_version() == 4


def test_null_engine_is_refused_without_a_device():
    from easywakeword_amd import _lib
    lib = _lib.load()
    assert lib.ewk_push_chunks(None, None, 0, None, 0, None, None, 0) == _lib.EWK_EINVAL
    assert b"engine is NULL" in lib.ewk_last_error()
    assert lib.ewk_push_chunks_pcm16(None, None, 0, None, 0, None, None, 0) == _lib.EWK_EINVAL
    assert lib.ewk_stream_pending(None, None, 0, None) == _lib.EWK_EINVAL


def test_the_facade_has_the_chunk_calls():
    from easywakeword_amd import StreamEngine
    for name in ("push_chunks", "push_chunks_pcm16", "push_chunks_device", "stream_pending"):
        assert callable(getattr(StreamEngine, name))


def test_array_source_read_sizes():
    import numpy as np
    import pytest
    from easywakeword_amd.audio import ArraySource
    audio = np.arange(1, 5001, dtype=np.float32)
    src = ArraySource(audio, read_sizes=[320, 1000, 37])
    got = [src.read() for _ in range(7)]
    assert [len(g) for g in got] == [320, 1000, 37, 320, 1000, 37, 320]
    np.testing.assert_array_equal(np.concatenate(got), audio[:3034])
    assert len(ArraySource(audio, read_sizes=480).read()) == 480
    tail = ArraySource(audio[:100], read_sizes=[64])
    np.testing.assert_array_equal(np.concatenate([tail.read(), tail.read()]), np.r_[audio[:100], np.zeros(28, np.float32)])
    assert tail.exhausted
    assert len(ArraySource(audio).read()) == 1600                # the default: a tick
    for bad in ([], [0], [-1, 5]):
        with pytest.raises(ValueError):
            ArraySource(audio, read_sizes=bad)


def test_mic_source_blocksize(monkeypatch):
    """MicSource(blocksize=): None keeps a tick per callback, 0 lets PortAudio choose (a stubbed
    sounddevice: construction only)."""
    import sys
    import types
    from easywakeword_amd.audio import MicSource
    seen = []
    stub = types.ModuleType("sounddevice")
    stub.InputStream = lambda **kw: seen.append(kw) or object()
    monkeypatch.setitem(sys.modules, "sounddevice", stub)
    assert MicSource().blocksize == 1600
    assert MicSource(samplerate=48000).blocksize == 4800
    assert MicSource(blocksize=0).blocksize == 0
    assert MicSource(blocksize=320, samplerate=48000).read_block == 4800
    assert [kw["blocksize"] for kw in seen] == [1600, 4800, 0, 320]
