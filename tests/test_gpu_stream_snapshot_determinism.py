"""Stream snapshots are reproducible and safe: two exports of an untouched engine are
byte-identical, an export straight after an import equals the imported records, every byte the
format declares dead is zero, a refused import changes nothing, the launches are counted under
profile kind 5, and the facade restores a full buffer at once."""
import numpy as np
import pytest

import lifecycle_util as lu
import snapshot_util as su

pytestmark = pytest.mark.gpu


def same(x, y):
    assert x.meta.tobytes() == y.meta.tobytes()
    assert x.payload.shape == y.payload.shape and np.array_equal(x.payload, y.payload)


def _import_raw(eng, slots, meta, payload):
    """ewk_import_streams with arrays that StreamSnapshot itself would refuse to hold."""
    import ctypes as C
    from easywakeword_amd import _lib
    s = np.array(slots, np.int32)
    m = np.ascontiguousarray(meta, _lib.STREAM_META_DTYPE)
    _lib.check(_lib.load().ewk_import_streams(eng.handle, _lib.i32ptr(s), s.size, m.ctypes.data_as(C.c_void_p),
                                              payload.ctypes.data_as(C.c_void_p), payload.nbytes, 0))


def pushed(case, n, k, desync=False):
    eng = su.engine(case, n)
    if desync:
        su.push_listed(eng, case, list(range(su.N)), case["src"], 0, k)
    else:
        su.push_lockstep(eng, case, case["src"] if n == su.N else case["other"], 0, k)
    return eng


@pytest.mark.parametrize("ring", ["f32_full", "i16_odd_rows"])
def test_exports_repeat_and_survive_an_import(ring):
    """Also with int16 rows that are not a multiple of 16 bytes (snapshot_util.odd_rows_case)."""
    case = su.make_case("f32_full") if ring == "f32_full" else su.odd_rows_case()
    k = 120 if ring == "f32_full" else 400
    b = pushed(case, su.N, k)
    c = pushed(case, su.NC, su.C_PRE)
    try:
        s1 = b.export_streams(list(range(su.N)))
        s2 = b.export_streams(list(range(su.N)))
        same(s1, s2)
        same(s1[[4, 2]], b.export_streams([4, 2]))                  # a record does not depend on its neighbours
        assert s1.meta["tick"].tolist() == [k] * su.N
        c.import_streams(su.SLOTS, s1)
        same(c.export_streams(su.SLOTS), s1)
        # ... through device memory too
        import torch
        buf = torch.empty(s1.payload.nbytes, dtype=torch.uint8, device="cuda:0")
        meta = b.export_streams_device(list(range(su.N)), buf.data_ptr(), buf.numel())
        b.sync()
        assert meta.tobytes() == s1.meta.tobytes()
        assert np.array_equal(buf.cpu().numpy().reshape(su.N, -1), s1.payload)
        # the ring of a moved stream reads back as the source's
        for i, s in enumerate(su.SLOTS):
            np.testing.assert_array_equal(c.read_last(s, 4 * 1600), b.read_last(i, 4 * 1600))
    finally:
        b.close()
        c.close()


def test_dead_bytes_are_zero():
    """Before the ring is full the RMS and sorted rows are not valid, no listener rows exist and
    nothing is pending: those sections, and all padding, are zero whatever the slot held before."""
    case = su.make_case("f32_full")
    c = pushed(case, su.N, 120)                # a full ring, valid rows: then reset and refilled a little
    try:
        c.reset_streams([3, 5])
        c.push_streams([3, 5], case["src"][:2, :40 * 1600])
        s = c.export_streams([3, 5])
        lay = s.layout
        for name in ("block_rms", "sorted", "listeners", "carry"):
            assert not s.section(name).any(), name
        assert s.section("ring")[:, :4 * 40 * 1600].any() and not s.section("ring")[:, 4 * 40 * 1600:].any()
        covered = np.zeros(lay["record_bytes"], bool)
        for off, nbytes in lay["sections"].values():
            covered[off:off + nbytes] = True
        assert not s.payload[:, ~covered].any()
        assert (~covered).sum() == lay["record_bytes"] - sum(b for _, b in lay["sections"].values()) > 0
        full = c.export_streams([0])
        assert full.section("block_rms").any() and full.section("sorted").any()
        srt = full.section("sorted").copy().view(np.float64)[0]
        rms = full.section("block_rms").copy().view(np.float64)[0]
        assert (np.diff(srt) >= 0).all() and np.array_equal(np.sort(rms), srt)
    finally:
        c.close()


def test_refused_imports_change_nothing():
    case = su.make_case("f32_full")
    other_geometry = su.make_case("f32_compact", cfg=dict(ring_samples=lu.min_ring(1600)))
    b = pushed(case, su.N, 30)
    c = pushed(case, su.NC, su.C_PRE)
    d = pushed(other_geometry, su.N, 5)
    try:
        snap = b.export_streams(list(range(su.N)))
        before = c.export_streams(list(range(su.NC)))
        foreign = d.export_streams(list(range(su.N)))
        with pytest.raises(ValueError, match="records of 648704 bytes"):      # (the size is checked first)
            c.import_streams(su.SLOTS, foreign)
        padded = np.zeros((su.N, snap.record_bytes), np.uint8)                 # the right size, the wrong geometry
        with pytest.raises(ValueError, match="another geometry"):
            _import_raw(c, su.SLOTS, foreign.meta, padded)
        with pytest.raises(ValueError, match="listed twice"):
            c.import_streams([7, 2, 5, 0, 8, 7], snap)
        with pytest.raises(ValueError, match="outside"):
            c.import_streams([7, 2, 5, 0, 8, 9], snap)
        with pytest.raises(ValueError, match="records for"):
            c.import_streams(su.SLOTS[:5], snap)
        for field, value, msg in (("magic", 7, "magic"), ("version", 2, "version"), ("fingerprint", 1, "geometry"),
                                  ("pending", 1600, "pending"), ("n_listeners", 17, "listeners"), ("profile", 0, "profile"),
                                  ("word", 1, "word")):
            bad = snap[list(range(su.N))]
            bad.meta[field][4] = value
            with pytest.raises(ValueError, match=msg):
                c.import_streams(su.SLOTS, bad)
        from easywakeword_amd import _lib
        import ctypes as C
        s = np.array(su.SLOTS, np.int32)
        rc = _lib.load().ewk_import_streams(c.handle, _lib.i32ptr(s), su.N, snap.meta.ctypes.data_as(C.c_void_p),
                                            snap.payload.ctypes.data_as(C.c_void_p), snap.payload.nbytes - 128, 0)
        assert rc == _lib.EWK_EINVAL
        meta = np.zeros(su.N, _lib.STREAM_META_DTYPE)
        small = np.full(snap.payload.nbytes - 1, 0xA5, np.uint8)
        rc = _lib.load().ewk_export_streams(b.handle, _lib.i32ptr(np.arange(su.N, dtype=np.int32)), su.N,
                                            meta.ctypes.data_as(C.c_void_p), small.ctypes.data_as(C.c_void_p), small.nbytes, 0)
        assert rc == _lib.EWK_EINVAL and (small == 0xA5).all() and not meta.view(np.uint8).any()
        same(c.export_streams(list(range(su.NC))), before)
        assert c.stream_ticks().tolist() == [su.C_PRE] * su.NC
    finally:
        for e in (b, c, d):
            e.close()


def test_profile_kind_5_counts_the_launches():
    case = su.make_case("f32_full")
    b = pushed(case, su.N, 10)
    c = pushed(case, su.NC, 3)
    try:
        for e in (b, c):
            e.profile(True)
        snap = b.export_streams([0, 3])
        c.import_streams([8, 1], snap)
        b.move_streams(c, [5], [0])
        for e in (b, c):
            ms, n = e.profile_read(5)
            assert n == 2 and ms > 0.0
            assert e.profile_read(5) == (0.0, 0)
        assert c.profile_read(2)[1] == 0 and b.profile_read(2)[1] == 0   # no gate launch among them
    finally:
        b.close()
        c.close()


def test_restored_wakeword_detects_without_refilling(tmp_path):
    """WakeWord.snapshot() / restore(): a new WakeWord pumps 100 ticks in _wait_for_buffer before
    it can detect; a restored one finds is_buffer_full() true before its first pump, and its
    waitforit() returns the word having pumped only the ticks up to the word."""
    import os
    import synth
    from golden_io import GOLD
    from easywakeword_amd import ArraySource, WakeWord
    wav = os.path.join(GOLD, "reference_word.wav")
    gate = dict(pre_speech_silence=0.8, speech_duration_min=0.3, speech_duration_max=2.0, post_speech_silence=0.4)
    pcm, _ = synth.make_stream(seed=7105, n_words=3, kinds=["tone880", "noise", "word"])
    pcm = np.asarray(pcm, np.float32)
    cut = 105
    old = WakeWord("hello", wav, timeout=60, similarity_threshold=90.0, source=ArraySource(pcm), **gate)
    new = WakeWord("hello", wav, timeout=60, similarity_threshold=90.0, source=ArraySource(pcm[cut * 1600:]), **gate)
    try:
        old._initialize_audio()
        for _ in range(cut):
            old._sound_buffer.pump()
        old._sound_buffer.engine.poll()
        snap = old.snapshot()
        assert len(snap) == 1 and int(snap.meta["tick"][0]) == cut
        new.restore(snap)
        assert new._sound_buffer.is_buffer_full()                 # before any pump of its own
        assert new._sound_buffer.source.reads == 0
        assert new.waitforit() == "hello"
        eng = new._sound_buffer.engine
        ticks = int(eng.stream_ticks()[0])
        print(f"restored WakeWord: detected at tick {ticks} after {new._sound_buffer.source.reads} reads")
        assert new._sound_buffer.source.reads == ticks - cut      # every read was a tick of new audio: no refill
    finally:
        old.stop()
        new.stop()


def test_restored_sound_buffer_is_full_at_once():
    """The facade: a new SoundBuffer pumps 100 ticks before is_buffer_full(); a restored one is
    full from its first tick, with the threshold and the last seconds of the one it continues."""
    import synth
    from easywakeword_amd import ArraySource, SoundBuffer, StreamSnapshot
    pcm, _ = synth.make_stream(seed=7105, n_words=4)
    pcm = np.asarray(pcm, np.float32)
    one = SoundBuffer(source=ArraySource(pcm))
    two = SoundBuffer(source=ArraySource(pcm[130 * 1600:]))
    try:
        for _ in range(130):
            one.pump()
        assert one.is_buffer_full() and not two.is_buffer_full()
        one.engine.poll()                        # (queued events are not part of a snapshot: they stay with `one`)
        two.restore(StreamSnapshot.frombytes(one.snapshot().tobytes()))
        assert two.is_buffer_full()
        assert two.silence_threshold == one.silence_threshold and two.is_silent() == one.is_silent()
        np.testing.assert_array_equal(two.return_last_n_seconds(3.0), one.return_last_n_seconds(3.0))
        for _ in range(20):
            one.pump()
            two.pump()
        assert two.engine.state(0) == one.engine.state(0)
        lu.assert_events_equal(one.engine.poll(), two.engine.poll(), 1)
    finally:
        one.engine.close()
        two.engine.close()
