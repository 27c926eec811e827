"""Stream snapshots off the device: the container StreamEngine.export_streams returns and
StreamEngine.import_streams takes (include/ewk.h, "stream snapshots").

Pure numpy: a snapshot is built, cut, written and read without a GPU and without libewk.so.
"""
from __future__ import annotations

import struct

import numpy as np

from ._lib import (EWK_SNAPSHOT_MAGIC, EWK_SNAPSHOT_VERSION, SNAP_SECTION_NAMES, STREAM_META_DTYPE,
                   EwkSnapshotLayout)

# byte form: this header, then the meta array, then the payload; everything little-endian
_HEADER = struct.Struct("<Iiqq")   # magic, version, n, record_bytes


def layout_dict(l: EwkSnapshotLayout) -> dict:
    """An ewk_snapshot_layout as a dict: its scalar fields, and "sections": name -> (offset, bytes)."""
    d = {f: getattr(l, f) for f, _ in l._fields_ if f != "section"}
    d["sections"] = {name: (int(l.section[k].offset), int(l.section[k].bytes))
                     for k, name in enumerate(SNAP_SECTION_NAMES)}
    return d


class StreamSnapshot:
    """n exported streams: `meta`, a structured array [n] (_lib.STREAM_META_DTYPE: tick, pending,
    profile, word, listeners and the format fields an importer checks), and `payload`, uint8
    [n, record_bytes], one record of device state per stream.  `layout` is the exporting engine's
    layout (layout_dict) when the snapshot came from an engine, else the format fields alone.
    Indexing with a position, a slice or a list gives a sub-snapshot (a copy)."""

    def __init__(self, meta, payload, layout=None):
        m = np.ascontiguousarray(meta, dtype=STREAM_META_DTYPE).reshape(-1)
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        if p.ndim != 2 or p.shape[0] != m.size:
            raise ValueError(f"payload must be uint8 [{m.size}, record_bytes], got shape {p.shape}")
        if m.size and not (m["record_bytes"] == p.shape[1]).all():
            raise ValueError(f"meta says records of {sorted(set(m['record_bytes'].tolist()))} bytes, "
                             f"the payload's are {p.shape[1]}")
        self.meta, self.payload = m, p
        self._layout = dict(layout) if layout is not None else None

    @property
    def record_bytes(self) -> int:
        return int(self.payload.shape[1])

    @property
    def layout(self) -> dict:
        if self._layout is not None:
            return self._layout
        out = {"magic": EWK_SNAPSHOT_MAGIC, "version": EWK_SNAPSHOT_VERSION, "record_bytes": self.record_bytes}
        if len(self):
            out["fingerprint"] = int(self.meta["fingerprint"][0])
        return out

    def __len__(self) -> int:
        return int(self.meta.size)

    def __getitem__(self, key) -> "StreamSnapshot":
        if isinstance(key, (int, np.integer)):
            key = [int(key)]
        elif not isinstance(key, slice):
            key = np.asarray(key, dtype=np.int64).reshape(-1)
        return StreamSnapshot(self.meta[key].copy(), self.payload[key].copy(), self._layout)

    def section(self, name: str) -> np.ndarray:
        """The bytes of one section of every record, uint8 [n, bytes] (needs the engine's layout)."""
        if self._layout is None or "sections" not in self._layout:
            raise ValueError("this snapshot carries no layout (it was read from bytes): use StreamEngine.snapshot_layout()")
        off, nbytes = self._layout["sections"][name]
        return self.payload[:, off:off + nbytes]

    # -- bytes and files ---------------------------------------------------------
    def tobytes(self) -> bytes:
        return _HEADER.pack(EWK_SNAPSHOT_MAGIC, EWK_SNAPSHOT_VERSION, len(self), self.record_bytes) + \
            self.meta.tobytes() + self.payload.tobytes()

    @classmethod
    def frombytes(cls, blob) -> "StreamSnapshot":
        """The snapshot tobytes() wrote.  ValueError for anything else: a foreign or truncated
        blob, another format version, trailing bytes."""
        buf = memoryview(blob).cast("B")
        if len(buf) < _HEADER.size:
            raise ValueError(f"not a stream snapshot: {len(buf)} bytes, the header alone has {_HEADER.size}")
        magic, version, n, record_bytes = _HEADER.unpack_from(buf, 0)
        if magic != EWK_SNAPSHOT_MAGIC:
            raise ValueError(f"not a stream snapshot: magic {magic:#010x}, expected {EWK_SNAPSHOT_MAGIC:#010x}")
        if version != EWK_SNAPSHOT_VERSION:
            raise ValueError(f"stream snapshot version {version}; this library reads version {EWK_SNAPSHOT_VERSION}")
        if n < 0 or record_bytes <= 0 or record_bytes % 128:
            raise ValueError(f"corrupt stream snapshot header: n = {n}, record_bytes = {record_bytes}")
        meta_bytes = n * STREAM_META_DTYPE.itemsize
        want = _HEADER.size + meta_bytes + n * record_bytes
        if len(buf) != want:
            raise ValueError(f"stream snapshot of {n} records of {record_bytes} bytes is {want} bytes, got {len(buf)}"
                             + (" (truncated)" if len(buf) < want else ""))
        meta = np.frombuffer(buf, dtype=STREAM_META_DTYPE, count=n, offset=_HEADER.size).copy()
        payload = np.frombuffer(buf, dtype=np.uint8, count=n * record_bytes,
                                offset=_HEADER.size + meta_bytes).reshape(n, record_bytes).copy()
        if n and not ((meta["magic"] == EWK_SNAPSHOT_MAGIC).all() and (meta["version"] == EWK_SNAPSHOT_VERSION).all()):
            raise ValueError("corrupt stream snapshot: a record's meta has another magic or version")
        return cls(meta, payload)

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(_HEADER.pack(EWK_SNAPSHOT_MAGIC, EWK_SNAPSHOT_VERSION, len(self), self.record_bytes))
            f.write(self.meta.tobytes())
            f.write(self.payload.data)

    @classmethod
    def load(cls, path) -> "StreamSnapshot":
        with open(path, "rb") as f:
            return cls.frombytes(f.read())
