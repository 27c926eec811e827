"""Audio I/O for the drop-in facade: WAV decode and block sources.

``load_wav`` replaces ``librosa.load(path, sr=16000)`` (reference wakeword.py:588,
866-870): PCM16 -> float32 int16/32768 (libsndfile scaling), PCM32 -> /2**31,
8-bit unsigned -> (x-128)/128, channel mean for multi-channel files
(librosa.to_mono).  16 kHz files are bit-exact with librosa.  Other rates are
resampled to 16 kHz on the host with a polyphase Kaiser FIR
(scipy.signal.resample_poly); librosa's default there is soxr 'HQ' (soxr is absent
from this image), so resampled audio is close to, not bit-identical with, the
reference's -- parity unpinned for non-16 kHz files.

Sources replace the PortAudio input stream of SoundBuffer (wakeword.py:438-444):
each yields float32 blocks of ``block`` samples, one per 0.1 s tick -- or, for a source kept at
its own sample rate (``rate=`` / ``native_rate=True`` / ``samplerate=``), the tick's samples at
that rate, which the engine resamples on the device (StreamEngine.set_input_rate).

G.711 (``g711_decode`` / ``g711_encode``, WAVE_FORMAT_ALAW / WAVE_FORMAT_MULAW files, and sources
with ``codec="ulaw"`` / ``"alaw"``): PCMU and PCMA code bytes.  A source with a codec yields uint8
blocks and the engine decodes them on the device (StreamEngine.push_g711 / push_chunks_g711).
"""
from __future__ import annotations

import struct
import wave
from typing import Iterator, Optional

import numpy as np

FREQUENCY = 16000


G711_PAD = {"ulaw": 0xFF, "alaw": 0xD5}   # the code of a zero sample (A-law: of +8, its smallest magnitude)
_WAVE_FORMAT_G711 = {6: "alaw", 7: "ulaw"}   # WAVE_FORMAT_ALAW, WAVE_FORMAT_MULAW


def _g711_law(law: str) -> str:
    if law not in G711_PAD:
        raise ValueError(f'law must be "ulaw" or "alaw", got {law!r}')
    return law


def g711_decode(codes, law: str) -> np.ndarray:
    """G.711 code bytes -> int16 (ITU-T G.711; equal to audioop.ulaw2lin / alaw2lin at width 2,
    and to the device decode, csrc/ewk_g711.h).  The float sample is the value / 32768."""
    b = np.asarray(codes, dtype=np.uint8).astype(np.int32)
    if _g711_law(law) == "ulaw":
        u = ~b & 0xFF
        t = (((u & 0xF) << 3) + 0x84) << ((u >> 4) & 7)
        v = np.where(u & 0x80, 0x84 - t, t - 0x84)
    else:
        a = b ^ 0x55
        e, m = (a >> 4) & 7, a & 0xF
        t = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
        v = np.where(a & 0x80, t, -t)
    return v.astype(np.int16)


_SEG_UEND = np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF])
_SEG_AEND = np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF])


def g711_encode(pcm16, law: str) -> np.ndarray:
    """int16 PCM -> G.711 code bytes: the ITU / Sun g711.c encoder on the sample's upper 14
    (mu-law) or 13 (A-law) bits, equal to audioop.lin2ulaw / lin2alaw at width 2 on every value."""
    x = np.asarray(pcm16, dtype=np.int16).astype(np.int32)
    if _g711_law(law) == "ulaw":
        v = x >> 2
        mask = np.where(v < 0, 0x7F, 0xFF)
        v = np.minimum(np.abs(v), 8159) + (0x84 >> 2)
        seg = np.searchsorted(_SEG_UEND, v, side="left")
        code = np.where(seg >= 8, 0x7F, (seg << 4) | ((v >> (seg + 1)) & 0xF))
    else:
        v = x >> 3
        mask = np.where(v >= 0, 0xD5, 0x55)
        v = np.where(v >= 0, v, -v - 1)
        seg = np.searchsorted(_SEG_AEND, v, side="left")
        code = np.where(seg >= 8, 0x7F, (seg << 4) | ((v >> np.maximum(seg, 1)) & 0xF))
    return (code ^ mask).astype(np.uint8)


def _read_g711_wav(path: str):
    """(law, channels, rate, code bytes) of a WAVE_FORMAT_ALAW / WAVE_FORMAT_MULAW file, which the
    stdlib wave module refuses; None for every other format.  RIFF chunks parsed by hand."""
    with open(str(path), "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        return None
    at, fmt, data = 12, None, None
    while at + 8 <= len(raw):
        cid, size = raw[at:at + 4], struct.unpack_from("<I", raw, at + 4)[0]
        body = raw[at + 8:at + 8 + size]
        if cid == b"fmt " and len(body) >= 16:
            fmt = struct.unpack_from("<HHIIHH", body, 0)
        elif cid == b"data":
            data = body
        at += 8 + size + (size & 1)   # chunks are word-aligned
    if fmt is None or fmt[0] not in _WAVE_FORMAT_G711:
        return None
    if data is None or fmt[5] != 8 or fmt[1] < 1:
        raise ValueError(f"{path}: a G.711 WAV needs 8 bits per sample and a data chunk")
    return _WAVE_FORMAT_G711[fmt[0]], int(fmt[1]), int(fmt[2]), np.frombuffer(data, dtype=np.uint8)


def load_wav(path: str, sr: int = FREQUENCY) -> np.ndarray:
    g711 = _read_g711_wav(path)
    if g711 is not None:   # decoded on the host: int16 / 32768, as PCM16
        law, nch, rate, codes = g711
        codes = codes[:len(codes) - len(codes) % nch]
        x = g711_decode(codes, law).astype(np.float32) / np.float32(32768.0)
        if nch > 1:
            x = np.mean(x.reshape(-1, nch).T, axis=0).astype(np.float32)
        if rate != sr:
            x = resample(x, rate, sr)
        return np.ascontiguousarray(x, dtype=np.float32)
    with wave.open(str(path), "rb") as w:
        nch, sw, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if sw == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768.0)
    elif sw == 4:
        x = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif sw == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    else:
        raise ValueError(f"{path}: unsupported sample width {sw}")
    if nch > 1:
        x = np.mean(x.reshape(-1, nch).T, axis=0).astype(np.float32)
    if rate != sr:
        x = resample(x, rate, sr)
    return np.ascontiguousarray(x, dtype=np.float32)


def resample(x: np.ndarray, orig_sr: int, target_sr: int) -> np.ndarray:
    """Band-limited resampling orig_sr -> target_sr (polyphase FIR, Kaiser beta 5.0),
    float64 internally, float32 out, length ceil(n * target / orig) like librosa."""
    from math import gcd
    from scipy.signal import resample_poly
    if orig_sr <= 0 or target_sr <= 0:
        raise ValueError("sample rates must be positive")
    g = gcd(int(orig_sr), int(target_sr))
    up, down = int(target_sr) // g, int(orig_sr) // g
    y = resample_poly(np.asarray(x, np.float64), up, down, window=("kaiser", 5.0))
    n = int(np.ceil(len(x) * target_sr / orig_sr))
    return y[:n].astype(np.float32)


def write_wav(path: str, audio, sr: int = FREQUENCY) -> None:
    """PCM16 writer with libsndfile's float scaling (x * 32767)."""
    q = np.clip(np.round(np.asarray(audio, np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(q.tobytes())


def input_block(block: int, rate: int) -> int:
    """Samples per tick at `rate` Hz for a tick of `block` samples at 16 kHz (StreamEngine.input_block)."""
    n = int(block) * int(rate)
    if int(rate) <= 0 or n % FREQUENCY:
        raise ValueError(f"a tick of {block} samples at {FREQUENCY} Hz is not a whole number of samples at {rate} Hz")
    return n // FREQUENCY


class ArraySource:
    """Blocks from an in-memory float32 signal; zeros after the end (a silent mic).
    ``rate``: the signal's sample rate.  At another rate than 16 kHz every read yields the
    tick's samples at that rate (``block * rate / 16000``; ``block`` stays the 16 kHz tick the
    engine is built with) and the engine resamples them on the device.
    ``read_sizes``: an int, or a sequence that is cycled -- every read yields that many input
    samples instead of a tick's (a network source's packets; the engine re-blocks them on the
    device, StreamEngine.push_chunks).
    ``codec``: "ulaw" or "alaw" -- `audio` holds G.711 code bytes (normally with ``rate=8000``),
    every read yields a uint8 block for the engine to decode on the device, and the padding after
    the end is the law's code for zero (0xFF for mu-law, 0xD5 for A-law)."""

    realtime = False

    def __init__(self, audio, block: int = 1600, loop: bool = False, rate: int = FREQUENCY, read_sizes=None,
                 codec: Optional[str] = None):
        self.codec = None if codec is None else _g711_law(codec)
        self.dtype, self.pad = (np.float32, 0.0) if codec is None else (np.uint8, G711_PAD[codec])
        self.audio = np.ascontiguousarray(np.asarray(audio, dtype=self.dtype).reshape(-1))
        self.block = int(block)
        self.rate = int(rate)
        self.read_block = input_block(self.block, self.rate)
        if read_sizes is not None:
            read_sizes = [int(read_sizes)] if np.isscalar(read_sizes) else [int(n) for n in read_sizes]
            if not read_sizes or min(read_sizes) < 0 or max(read_sizes) == 0:
                raise ValueError("read_sizes must hold sample counts >= 0, one of them positive")
        self.read_sizes = read_sizes
        self.reads = 0
        self.loop = loop
        self.pos = 0

    def blocks(self) -> Iterator[np.ndarray]:
        while True:
            b = self.read()
            yield b

    def read(self) -> np.ndarray:
        n = self.read_block if self.read_sizes is None else self.read_sizes[self.reads % len(self.read_sizes)]
        self.reads += 1
        a = self.audio
        if self.loop and len(a):
            idx = (self.pos + np.arange(n)) % len(a)
            out = a[idx]
        else:
            out = np.full(n, self.pad, self.dtype)
            if self.pos < len(a):
                chunk = a[self.pos:self.pos + n]
                out[:len(chunk)] = chunk
        self.pos += n
        return out

    @property
    def exhausted(self) -> bool:
        return not self.loop and self.pos >= len(self.audio)

    def start(self):
        pass

    def stop(self):
        pass


class WavSource(ArraySource):
    """A WAV file: resampled to 16 kHz on the host when it is loaded, or, with
    ``native_rate=True``, left at its own rate (``.rate``) and resampled on the device."""

    def __init__(self, path: str, block: int = 1600, loop: bool = False, native_rate: bool = False):
        if native_rate:
            g711 = _read_g711_wav(path)
            if g711 is not None:
                rate = g711[2]
            else:
                with wave.open(str(path), "rb") as w:
                    rate = w.getframerate()
            super().__init__(load_wav(path, sr=rate), block=block, loop=loop, rate=rate)
        else:
            super().__init__(load_wav(path), block=block, loop=loop)


class MicSource:
    """PortAudio microphone through ``sounddevice`` (only when installed); `device` is a
    PortAudio index -- easywakeword_amd.devices.AudioDeviceManager resolves names and
    the reference's magic words.  ``samplerate``: open the device at its own rate (no
    conversion inside PortAudio); the engine resamples the blocks on the device.
    ``blocksize``: frames per callback -- None: a tick's (``read_block``), 0: PortAudio chooses, as
    the reference opens its stream; reads of any other length than a tick are re-blocked on the
    device (StreamEngine.push_chunks)."""

    realtime = True

    def __init__(self, device: Optional[int] = None, block: int = 1600, samplerate: int = FREQUENCY,
                 blocksize: Optional[int] = None):
        import queue

        import sounddevice as sd  # noqa: F401  (raises ImportError/OSError when absent)
        self._sd = sd
        self.block = int(block)
        self.rate = int(samplerate)
        self.read_block = input_block(self.block, self.rate)
        self.q: "queue.Queue[np.ndarray]" = queue.Queue()
        self.blocksize = self.read_block if blocksize is None else int(blocksize)
        self.stream = sd.InputStream(samplerate=self.rate, channels=1, blocksize=self.blocksize, device=device,
                                     callback=lambda indata, frames, t, status: self.q.put(
                                         np.array(indata, dtype=np.float32).reshape(-1).copy()))

    def start(self):
        self.stream.start()

    def stop(self):
        self.stream.stop()

    def read(self) -> np.ndarray:
        return self.q.get()

    exhausted = False
