"""G.711 on the host (CPU; no device is touched): the library's table (csrc/ewk_g711.h through
ewk_g711_table) against the formulas of the issue restated in numpy and, where the interpreter
still has it, against audioop; the numpy codec of easywakeword_amd.audio; WAVE_FORMAT_ALAW /
WAVE_FORMAT_MULAW files; and ArraySource(codec=)."""
import ctypes as C
import struct

import numpy as np
import pytest

LAWS = ("ulaw", "alaw")

try:
    import audioop
except ImportError:   # (removed from the standard library in Python 3.13)
    audioop = None


def _formula(law):
    """The decode as the header states it, code by code in plain Python integers."""
    out = []
    for b in range(256):
        if law == "ulaw":
            u = ~b & 0xFF
            t = (((u & 0xF) << 3) + 0x84) << ((u >> 4) & 7)
            out.append(0x84 - t if u & 0x80 else t - 0x84)
        else:
            a = b ^ 0x55
            e, m = (a >> 4) & 7, a & 0xF
            t = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
            out.append(t if a & 0x80 else -t)
    return np.array(out, np.int64)


def _table(law):
    from easywakeword_amd import _lib
    t = np.zeros(256, np.int16)
    _lib.check(_lib.load().ewk_g711_table(_lib.G711_LAWS[law], t.ctypes.data_as(C.c_void_p)))
    return t


@pytest.mark.parametrize("law", LAWS)
def test_table_equals_the_formulas_and_audioop(law):
    t = _table(law)
    want = _formula(law)
    np.testing.assert_array_equal(t.astype(np.int64), want)
    lo, hi, distinct = (-32124, 32124, 255) if law == "ulaw" else (-32256, 32256, 256)
    assert (t.min(), t.max(), len(set(t.tolist()))) == (lo, hi, distinct)
    if law == "ulaw":
        assert t[0x7F] == 0 and t[0xFF] == 0
    else:
        assert np.abs(t.astype(np.int64)).min() == 8
    # v / 32768 is exact in float32
    f = t.astype(np.float32) * np.float32(1.0 / 32768.0)
    np.testing.assert_array_equal(f.astype(np.float64) * 32768.0, want.astype(np.float64))
    if audioop is not None:
        fn = audioop.ulaw2lin if law == "ulaw" else audioop.alaw2lin
        np.testing.assert_array_equal(t, np.frombuffer(fn(bytes(range(256)), 2), np.int16))


def test_table_refuses_another_law():
    from easywakeword_amd import _lib
    lib = _lib.load()
    t = np.full(256, 77, np.int16)
    assert lib.ewk_g711_table(2, t.ctypes.data_as(C.c_void_p)) == _lib.EWK_EINVAL
    assert b"law = 2" in lib.ewk_last_error()
    assert lib.ewk_g711_table(0, None) == _lib.EWK_EINVAL
    assert (t == 77).all()


@pytest.mark.parametrize("law", LAWS)
def test_numpy_codec(law):
    from easywakeword_amd import audio
    codes = np.arange(256, dtype=np.uint8)
    dec = audio.g711_decode(codes, law)
    assert dec.dtype == np.int16
    np.testing.assert_array_equal(dec, _table(law))
    np.testing.assert_array_equal(audio.g711_decode(codes.reshape(16, 16), law), dec.reshape(16, 16))
    # decode(encode(decode(c))) == decode(c) for all 256 codes
    enc = audio.g711_encode(dec, law)
    assert enc.dtype == np.uint8
    np.testing.assert_array_equal(audio.g711_decode(enc, law), dec)
    # the encoder is monotone: a larger sample never decodes to a smaller value
    x = np.arange(-32768, 32768).astype(np.int16)
    e = audio.g711_encode(x, law)
    assert (np.diff(audio.g711_decode(e, law).astype(np.int64)) >= 0).all()
    if law == "ulaw":   # the two zeros: both decode to 0, and 0 encodes to the positive one
        assert audio.g711_decode([0x7F, 0xFF], law).tolist() == [0, 0]
        assert audio.g711_encode([0], law)[0] == 0xFF
    if audioop is not None:
        fn = audioop.lin2ulaw if law == "ulaw" else audioop.lin2alaw
        np.testing.assert_array_equal(e, np.frombuffer(fn(x.tobytes(), 2), np.uint8))
    with pytest.raises(ValueError):
        audio.g711_decode(codes, "g722")
    with pytest.raises(ValueError):
        audio.g711_encode(x, "g722")


def _riff(fmt_tag, rate, channels, codes, extra=b""):
    """A WAV with a hand-made header: an 18-byte fmt chunk (cbSize 0), a chunk to skip, then data."""
    fmt = struct.pack("<HHIIHHH", fmt_tag, channels, rate, rate * channels, channels, 8, 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra
    body += b"data" + struct.pack("<I", len(codes)) + codes + (b"\0" if len(codes) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


@pytest.mark.parametrize("law,tag", [("ulaw", 7), ("alaw", 6)])
def test_load_wav_reads_g711_files(tmp_path, law, tag):
    from easywakeword_amd import audio
    codes = np.random.default_rng(tag).integers(0, 256, 1235, dtype=np.uint8)   # (odd: the data chunk is padded)
    want = audio.g711_decode(codes, law).astype(np.float32) / np.float32(32768.0)
    path = tmp_path / f"{law}.wav"
    fact = b"fact" + struct.pack("<II", 4, len(codes))
    path.write_bytes(_riff(tag, 8000, 1, codes.tobytes(), extra=fact))
    got = audio.load_wav(str(path), sr=8000)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(audio.load_wav(str(path)), audio.resample(want, 8000, 16000))
    # two channels: the channel mean, as for PCM files
    st = tmp_path / f"{law}_stereo.wav"
    st.write_bytes(_riff(tag, 8000, 2, codes[:1234].tobytes()))
    two = audio.g711_decode(codes[:1234], law).astype(np.float32) / np.float32(32768.0)
    np.testing.assert_array_equal(audio.load_wav(str(st), sr=8000), np.mean(two.reshape(-1, 2).T, axis=0).astype(np.float32))
    # a source at the file's own rate
    src = audio.WavSource(str(path), native_rate=True)
    assert src.rate == 8000 and src.read_block == 800
    np.testing.assert_array_equal(src.read(), want[:800])
    # PCM16 files still go through the wave module
    pcm = tmp_path / "pcm.wav"
    audio.write_wav(str(pcm), want, sr=8000)
    assert len(audio.load_wav(str(pcm), sr=8000)) == len(want)


@pytest.mark.parametrize("law,pad", [("ulaw", 0xFF), ("alaw", 0xD5)])
def test_array_source_with_a_codec(law, pad):
    from easywakeword_amd import ArraySource, audio
    codes = np.random.default_rng(pad).integers(0, 256, 2000, dtype=np.uint8)
    src = ArraySource(codes, rate=8000, codec=law)
    assert src.codec == law and src.rate == 8000 and src.read_block == 800
    blocks = [src.read() for _ in range(4)]
    assert all(b.dtype == np.uint8 and b.shape == (800,) for b in blocks)
    np.testing.assert_array_equal(np.concatenate(blocks[:2]), codes[:1600])
    np.testing.assert_array_equal(blocks[2][:400], codes[1600:])
    assert (blocks[2][400:] == pad).all() and (blocks[3] == pad).all() and src.exhausted
    # the padding is the law's code for zero (A-law has none: its smallest magnitude)
    assert abs(int(audio.g711_decode([pad], law)[0])) == (0 if law == "ulaw" else 8)
    pk = ArraySource(codes, rate=8000, codec=law, read_sizes=[160, 37])
    got = [pk.read() for _ in range(3)]
    assert [len(g) for g in got] == [160, 37, 160] and all(g.dtype == np.uint8 for g in got)
    np.testing.assert_array_equal(np.concatenate(got), codes[:357])
    # without a codec nothing changes: float32 blocks, zeros after the end
    f = ArraySource(np.ones(10, np.float32))
    b = f.read()
    assert f.codec is None and b.dtype == np.float32 and b[:10].all() and not b[10:].any()
    with pytest.raises(ValueError):
        ArraySource(codes, rate=8000, codec="g722")


MAIN = r"""
#include <stdio.h>
#include "%s"
// stdin: 512 integers, the expected values of mu-law codes 0..255 then A-law codes 0..255
int main() {
    int bad = 0;
    for (int law = 0; law < 2; ++law)
        for (unsigned b = 0; b < 256; ++b) {
            int want = 0;
            if (scanf("%%d", &want) != 1) return 2;
            const int got = ewk::g711_decode(b, law);
            const float f = ewk::g711_sample(b, law);
            if (got != want || (double)f * 32768.0 != (double)want) {
                printf("law %%d code %%u: %%d, expected %%d\n", law, b, got, want);
                bad += 1;
            }
        }
    printf("checked 512\n");
    return bad ? 1 : 0;
}
"""


def test_header_under_sanitizers(tmp_path):
    """csrc/ewk_g711.h is HIP-free for a host compiler: a stand-alone program built with g++
    -fsanitize=address,undefined decodes all 256 codes of both laws (no shift or conversion is
    undefined) and compares them with the formulas' table.  Nothing of it is loaded into Python."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "easywakeword_amd", "csrc",
                       "ewk_g711.h")
    src = tmp_path / "g711_main.cpp"
    src.write_text(MAIN % hdr)
    exe = tmp_path / "g711_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(src), "-o", str(exe)], check=True)
    want = np.concatenate([_formula("ulaw"), _formula("alaw")])
    r = subprocess.run([str(exe)], input=" ".join(map(str, want.tolist())) + "\n", capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stderr == "" and r.stdout.strip() == "checked 512"
