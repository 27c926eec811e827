"""StreamSnapshot off the device: built from numpy arrays it round-trips through bytes, files and
indexing, and refuses what is not a snapshot (CPU, no library call)."""
import struct

import numpy as np
import pytest

from easywakeword_amd import StreamSnapshot, _lib

RB = 256   # record_bytes of the toy records (a multiple of 128)


def make(n=5, seed=3):
    rng = np.random.default_rng(seed)
    meta = np.zeros(n, _lib.STREAM_META_DTYPE)
    meta["magic"] = _lib.EWK_SNAPSHOT_MAGIC
    meta["version"] = _lib.EWK_SNAPSHOT_VERSION
    meta["tick"] = rng.integers(0, 1 << 40, n)
    meta["record_bytes"] = RB
    meta["fingerprint"] = 0xFEDCBA9876543210
    meta["pending"] = rng.integers(0, 1600, n)
    meta["profile"] = rng.integers(-1, 3, n)
    meta["word"] = rng.integers(0, 3, n)
    meta["n_listeners"] = rng.integers(1, 17, n)
    meta["listeners"] = rng.integers(-1, 5, (n, _lib.EWK_LISTENERS_MAX, 2))
    return StreamSnapshot(meta, rng.integers(0, 256, (n, RB), dtype=np.uint8))


def same(a, b):
    assert len(a) == len(b)
    assert a.meta.tobytes() == b.meta.tobytes()
    assert a.payload.shape == b.payload.shape and a.payload.tobytes() == b.payload.tobytes()


def test_bytes_round_trip_and_form():
    s = make()
    blob = s.tobytes()
    assert len(blob) == 24 + 5 * 176 + 5 * RB
    assert struct.unpack_from("<Iiqq", blob) == (_lib.EWK_SNAPSHOT_MAGIC, _lib.EWK_SNAPSHOT_VERSION, 5, RB)
    assert blob[24:24 + 5 * 176] == s.meta.tobytes() and blob[24 + 5 * 176:] == s.payload.tobytes()
    same(StreamSnapshot.frombytes(blob), s)
    same(StreamSnapshot.frombytes(bytearray(blob)), s)
    empty = make(0)
    same(StreamSnapshot.frombytes(empty.tobytes()), empty)
    assert StreamSnapshot.frombytes(blob).layout["record_bytes"] == RB


def test_save_and_load(tmp_path):
    s = make(7, seed=11)
    s.save(tmp_path / "streams.ewksnap")
    assert (tmp_path / "streams.ewksnap").read_bytes() == s.tobytes()
    same(StreamSnapshot.load(tmp_path / "streams.ewksnap"), s)


def test_indexing_gives_sub_snapshots():
    s = make(6)
    one = s[2]
    assert len(one) == 1 and one.meta[0] == s.meta[2] and (one.payload[0] == s.payload[2]).all()
    pick = s[[4, 0, 5]]
    assert len(pick) == 3
    assert (pick.meta == s.meta[[4, 0, 5]]).all() and (pick.payload == s.payload[[4, 0, 5]]).all()
    same(s[1:4], s[[1, 2, 3]])
    same(s[-1], s[5])
    pick.payload[:] = 0                      # a copy: the parent is untouched
    assert s.payload[[4, 0, 5]].any()
    same(StreamSnapshot.frombytes(s[[3, 1]].tobytes()), s[[3, 1]])
    with pytest.raises(IndexError):
        s[6]


def test_constructor_checks_shapes():
    s = make(3)
    with pytest.raises(ValueError, match="payload must be"):
        StreamSnapshot(s.meta, s.payload[:2])
    with pytest.raises(ValueError, match="records of"):
        StreamSnapshot(s.meta, np.zeros((3, 128), np.uint8))


def test_truncated_and_foreign_blobs_are_refused():
    blob = make().tobytes()
    for cut in (0, 10, 23, 24, 24 + 176, len(blob) - 1):
        with pytest.raises(ValueError, match="truncated|header"):
            StreamSnapshot.frombytes(blob[:cut])
    with pytest.raises(ValueError, match="bytes, got"):
        StreamSnapshot.frombytes(blob + b"\0")
    bad = bytearray(blob)
    bad[0] ^= 0xFF
    with pytest.raises(ValueError, match="magic"):
        StreamSnapshot.frombytes(bytes(bad))
    with pytest.raises(ValueError, match="magic"):
        StreamSnapshot.frombytes(b"RIFF" + blob[4:])
    bad = bytearray(blob)
    struct.pack_into("<i", bad, 4, _lib.EWK_SNAPSHOT_VERSION + 1)
    with pytest.raises(ValueError, match="version"):
        StreamSnapshot.frombytes(bytes(bad))
    bad = bytearray(blob)
    struct.pack_into("<q", bad, 16, RB + 1)
    with pytest.raises(ValueError, match="corrupt"):
        StreamSnapshot.frombytes(bytes(bad))
    bad = bytearray(blob)
    struct.pack_into("<I", bad, 24 + 176, 0)          # the second record's meta
    with pytest.raises(ValueError, match="corrupt"):
        StreamSnapshot.frombytes(bytes(bad))
