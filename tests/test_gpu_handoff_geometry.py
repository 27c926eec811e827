"""The hand-off kernels past their first pass (GPU): sizes at which the loops the launch geometry
creates run a second time.

* k_compact_scan scans 1,024 block counts an iteration and carries the running total: more than
  1,024 blocks of 4,096 segments (n > 4,194,304) reach the carry; ids from first_id = 2**40, NaN
  scores with their payloads, an append on top and an append of nothing.
* k_decode_pcm16 and k_decode_g711 are grid-stride on a grid capped at 16,384 blocks of 256: above
  4,194,304 samples (16 x that many G.711 codes) a thread takes a second stride.

Every bar is equality of bits against numpy or a table lookup.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER_BLOCK = 4096            # segments a compaction block counts
SCAN = 1024                 # block counts a scan iteration takes
PASS = 16384 * 256          # threads of the capped decode grid
FIRST_ID = 2 ** 40
NAN_BITS = 0x7FF8000000000000


@pytest.fixture(scope="module")
def eng():
    from easywakeword_amd import Engine
    e = Engine()
    yield e
    e.close()


def _batch(n, seed):
    """(score, match) on the device: about 1 % matches, block 0 all matches, block 1 none, the last
    partial block all matches; every seventh score a NaN with its own payload (block 0 and the 1 %
    match some of them)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    score = torch.rand(n, generator=g, device="cuda", dtype=torch.float64) * 100.0
    bits = score.view(torch.int64)
    k = torch.arange(0, n, 7, device="cuda", dtype=torch.int64)
    bits[::7] = NAN_BITS + 1 + k
    match = (torch.rand(n, generator=g, device="cuda") < 0.01).to(torch.uint8)
    match[:PER_BLOCK] = 1
    match[PER_BLOCK:2 * PER_BLOCK] = 0
    assert n % PER_BLOCK
    match[n // PER_BLOCK * PER_BLOCK:] = 1
    return score, match


def _records(score, match, step):
    """numpy on host copies: rows (first_id + index, score bits, step) of the matched segments."""
    idx = np.flatnonzero(match.cpu().numpy())
    sc = score.cpu().numpy().view(np.int64)[idx]
    return np.stack([FIRST_ID + idx, sc, np.full(len(idx), step, np.int64)], axis=1)


@pytest.mark.parametrize("n", [PER_BLOCK * SCAN + 1, 2 * PER_BLOCK * SCAN + PER_BLOCK + 1])
def test_compaction_past_one_scan_pass(eng, n):
    import torch
    assert -(-n // PER_BLOCK) in (SCAN + 1, 2 * SCAN + 2)       # two and three scan iterations
    s1, m1 = _batch(n, 41 + n % 97)
    s2, m2 = _batch(n, 43 + n % 97)
    r1, r2 = _records(s1, m1, 3), _records(s2, m2, 9)
    k1, k2 = len(r1), len(r2)
    assert 0.009 * n < k1 - PER_BLOCK < 0.011 * n               # about 1 % besides block 0
    nan_matched = np.isnan(r1[:, 1].copy().view(np.float64))
    assert nan_matched.sum() > PER_BLOCK // 7 + 50 and len(np.unique(r1[nan_matched, 1])) == nan_matched.sum()
    GUARD = -77
    out = torch.full((k1 + k2 + 1, 3), GUARD, dtype=torch.int64, device="cuda")   # what the counts need + a guard row
    cnt = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()         # (the compaction runs on the engine's stream, torch filled these on its own)
    eng.compact_positives_device(s1.data_ptr(), m1.data_ptr(), n, FIRST_ID, out.data_ptr(), cnt.data_ptr(), step=3)
    torch.cuda.synchronize()
    assert int(cnt.item()) == k1
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:k1], r1)
    assert (got[k1:] == GUARD).all()
    # an append of the same size, another step tag: behind the first call's records
    eng.compact_positives_device(s2.data_ptr(), m2.data_ptr(), n, FIRST_ID, out.data_ptr(), cnt.data_ptr(), step=9,
                                 append=True)
    torch.cuda.synchronize()
    assert int(cnt.item()) == k1 + k2
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:k1], r1)
    np.testing.assert_array_equal(got[k1:k1 + k2], r2)
    assert (got[k1 + k2:] == GUARD).all()
    # an append of nothing
    eng.compact_positives_device(s2.data_ptr(), m2.data_ptr(), 0, FIRST_ID, out.data_ptr(), cnt.data_ptr(), step=11,
                                 append=True)
    torch.cuda.synchronize()
    assert int(cnt.item()) == k1 + k2
    np.testing.assert_array_equal(out.cpu().numpy(), got)


def _pcm16(n):
    """All 65,536 int16 values, cycling."""
    return ((np.arange(n, dtype=np.int64) * 4099 + 12345) % 65536 - 32768).astype(np.int16)


def test_decode_pcm16_past_one_stride_pass_host(eng):
    n = PASS + 257
    x = _pcm16(n)
    assert len(np.unique(x)) == 65536
    want = x.astype(np.float32) / np.float32(32768.0)
    got = eng.decode_pcm16(x)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def test_decode_pcm16_device_form(eng):
    """Device pointers, the input at an odd int16 offset, guards either side of the output."""
    import torch
    from easywakeword_amd import _lib
    G, SENT = 8, np.float32(7.5)
    dev = torch.device("cuda", eng.gpu)
    for n in (1, 255, 256, 257, PASS + 257):
        x = _pcm16(n + 1)
        want = x[1:].astype(np.float32) / np.float32(32768.0)
        d_in = torch.from_numpy(x).to(dev)
        d_out = torch.full((G + n + G,), float(SENT), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()     # (the decode runs on the engine's stream, torch filled these on its own)
        _lib.check(eng._lib.ewk_decode_pcm16(eng.handle, C.c_void_p(d_in.data_ptr() + 2), n,
                                             C.c_void_p(d_out.data_ptr() + 4 * G), _lib.EWK_PCM_DEVICE))
        eng.sync()
        out = d_out.cpu().numpy()
        np.testing.assert_array_equal(out[G:G + n].view(np.int32), want.view(np.int32), err_msg=f"n {n}")
        assert (out[:G] == SENT).all() and (out[G + n:] == SENT).all(), n


@pytest.mark.parametrize("law", ["ulaw", "alaw"])
def test_decode_g711_past_one_stride_pass(eng, law):
    """16 x 4,194,304 + 16 x 300 + 5 codes in device memory, the input 3 bytes and the output one
    float off the 16-byte grid; compared on the device with a gather from the table."""
    import torch
    from easywakeword_amd import _lib
    n = 16 * PASS + 16 * 300 + 5
    G, SENT, IN_OFF, OUT_OFF = 8, 7.5, 3, 1
    dev = torch.device("cuda", eng.gpu)
    law_id = _lib.G711_LAWS[law]
    t16 = np.zeros(256, np.int16)
    _lib.check(eng._lib.ewk_g711_table(law_id, t16.ctypes.data_as(C.c_void_p)))
    table = torch.from_numpy(t16.astype(np.float32) / np.float32(32768.0)).to(dev)
    g = torch.Generator(device=dev).manual_seed(51 + law_id)
    codes = torch.randint(0, 256, (IN_OFF + n + 5,), generator=g, device=dev, dtype=torch.uint8)
    assert int(torch.bincount(codes[:1 << 20].to(torch.int64), minlength=256).min()) > 0    # every code
    d_out = torch.full((G + OUT_OFF + n + G,), SENT, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()         # (the decode runs on the engine's stream, torch filled these on its own)
    assert (codes.data_ptr() + IN_OFF) % 16 == IN_OFF and (d_out.data_ptr() + 4 * (G + OUT_OFF)) % 16 == 4 * OUT_OFF
    _lib.check(eng._lib.ewk_decode_g711(eng.handle, C.c_void_p(codes.data_ptr() + IN_OFF), n,
                                        C.c_void_p(d_out.data_ptr() + 4 * (G + OUT_OFF)), law_id, _lib.EWK_PCM_DEVICE))
    eng.sync()
    lo = G + OUT_OFF
    assert bool((d_out[:lo] == SENT).all()) and bool((d_out[lo + n:] == SENT).all())
    STEP = 1 << 23
    for a in range(0, n, STEP):
        b = min(n, a + STEP)
        want = table[codes[IN_OFF + a:IN_OFF + b].to(torch.int32)]
        got = d_out[lo + a:lo + b]
        if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
            bad = torch.nonzero(got.view(torch.int32) != want.view(torch.int32)).reshape(-1)
            pytest.fail(f"{law}: {len(bad)} samples differ in [{a}, {b}), first at {a + int(bad[0])}: "
                        f"got {got[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}")
