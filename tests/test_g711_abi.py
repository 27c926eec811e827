"""G.711 ingest in the C ABI: the header declares the calls and the two law defines, the ctypes
binding matches, the library exports them (CPU; no device is touched)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"ewk_g711_table": 2, "ewk_decode_g711": 6, "ewk_push_g711": 7, "ewk_push_streams_g711": 9,
         "ewk_push_chunks_g711": 10}


def _code():
    src = open(os.path.join(ROOT, "include", "ewk.h")).read()
    return " ".join(re.sub(r"/\*.*?\*/", "", src, flags=re.S).split())


def test_header_declares_the_g711_abi():
    code = _code()
    assert re.search(r"#define EWK_G711_ULAW 0\b", code)
    assert re.search(r"#define EWK_G711_ALAW 1\b", code)
    assert re.search(r"\bint ewk_g711_table\(int32_t law, int16_t\* out256\);", code)
    assert re.search(r"\bint ewk_decode_g711\(ewk_engine\* e, const uint8_t\* in, int64_t n, float\* out, int32_t law, "
                     r"int32_t flags\);", code)
    assert re.search(r"\bint ewk_push_g711\(ewk_engine\* e, const uint8_t\* pcm, int64_t stride, int64_t tick_stride, "
                     r"int32_t n_ticks, int32_t law, int32_t flags\);", code)
    assert re.search(r"\bint ewk_push_streams_g711\(ewk_engine\* e, const int32_t\* streams, int32_t n, "
                     r"const uint8_t\* pcm, int64_t stride, int64_t tick_stride, int32_t n_ticks, int32_t law, "
                     r"int32_t flags\);", code)
    assert re.search(r"\bint ewk_push_chunks_g711\(ewk_engine\* e, const int32_t\* streams, int32_t n, "
                     r"const uint8_t\* pcm, int64_t n_pcm, const int64_t\* offsets, const int32_t\* counts, int32_t law, "
                     r"const uint8_t\* laws, int32_t flags\);", code)
    assert re.search(r"#define EWK_ABI_VERSION 4\b", code)      # additive: the version stays


def test_binding_matches_the_header():
    from easywakeword_amd import _lib
    assert (_lib.G711_ULAW, _lib.G711_ALAW) == (0, 1)
    assert _lib.G711_LAWS == {"ulaw": 0, "alaw": 1}
    lib = _lib.load()
    for name, n_args in CALLS.items():
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)          # exported
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, name
    assert lib.ewk_abi_version() == 4


def test_null_engine_is_refused_without_a_device():
    from easywakeword_amd import _lib
    lib = _lib.load()
    assert lib.ewk_push_g711(None, None, 0, 0, 1, 0, 0) == _lib.EWK_EINVAL
    assert b"engine is NULL" in lib.ewk_last_error()
    assert lib.ewk_push_streams_g711(None, None, 0, None, 0, 0, 1, 0, 0) == _lib.EWK_EINVAL
    assert lib.ewk_push_chunks_g711(None, None, 0, None, 0, None, None, 0, None, 0) == _lib.EWK_EINVAL
    assert lib.ewk_decode_g711(None, None, 0, None, 0, 0) == _lib.EWK_EINVAL


def test_the_facade_has_the_g711_calls():
    from easywakeword_amd import Engine, StreamEngine, audio
    for name in ("push_g711", "push_streams_g711", "push_device_g711", "push_chunks_g711", "decode_g711"):
        assert callable(getattr(StreamEngine, name))
    assert callable(Engine.decode_g711) and callable(audio.g711_decode) and callable(audio.g711_encode)
    import inspect
    assert "g711" in inspect.signature(StreamEngine.push_streams_device).parameters
    assert "g711" in inspect.signature(StreamEngine.push_chunks_device).parameters
