"""G.711 subset pushes (ewk_push_streams_g711): engine A is pushed the decoded PCM16 and engine B
the code bytes by the same seeded subset schedule, with a list reset of one stream in the middle --
events, rings and thresholds are equal.  And a stream may change its sample type tick by tick:
stream 0 alternates float32, PCM16 and G.711 ticks of the same decoded audio and equals the
lockstep PCM16 engine."""
import numpy as np
import pytest

import g711_util as gu
import lifecycle_util as lu

pytestmark = pytest.mark.gpu

IB, N = gu.IB, gu.N


@pytest.mark.parametrize("law", gu.LAWS)
def test_subset_schedule_with_a_list_reset(law):
    d, n_ticks = gu.data()
    codes, dec16 = d[law]
    half = n_ticks // 2
    # every stream gets its first half; stream 2 is reset and hears everything from the start again,
    # the others go on -- so each stream still hears its whole input once without a break
    sched = [("push", x) for x in lu.schedule(N, half, 31, max_ticks=3)]
    sched.append(("reset", [2]))
    sched += [("push", x) for x in lu.schedule(N, n_ticks, 32, max_ticks=3, done=[half, half, 0, half])]
    out = []
    for name, src, law_arg in (("a", dec16, None), ("b", codes, law)):
        e = gu.engine()
        done = np.zeros(N, np.int64)
        got = []
        for what, x in sched:
            if what == "reset":
                got.append(e.poll())
                e.reset_streams(x)
                done[x] = 0
                continue
            sub, nt, first = x
            rows = lu.rows_of(src, sub, first, nt, IB)
            if law_arg is None:
                e.push_streams_pcm16(sub, rows)
            else:
                e.push_streams_g711(sub, rows, law_arg)
            done[sub] += nt
            np.testing.assert_array_equal(e.stream_ticks(), done)
            got.append(e.poll())
        out.append((np.concatenate(got), gu.results(e)))
        e.close()
    (ev_a, res_a), (ev_b, _) = out
    assert len(ev_a) >= gu.MIN_EVENTS, len(ev_a)
    # (the same check as against a lockstep reference: events, rings' bits, thresholds)
    assert lu.assert_events_equal(ev_a, ev_b, N) >= gu.MIN_EVENTS
    for s in range(N):
        np.testing.assert_array_equal(out[1][1][0][s].view(np.int32), res_a[0][s].view(np.int32), err_msg=f"ring {s}")
        assert out[1][1][1][s] == res_a[1][s]


@pytest.mark.parametrize("law", gu.LAWS)
def test_a_stream_changes_its_sample_type_tick_by_tick(law):
    import torch
    d, n_ticks = gu.data()
    codes, dec16 = d[law]
    f32 = dec16.astype(np.float32) / np.float32(32768.0)
    ref = gu.reference(law)
    e = gu.engine()
    got, keep = [], []
    for c in range(0, n_ticks, 3):
        nt = min(3, n_ticks - c)
        for t in range(c, c + nt):
            sl = slice(t * IB, (t + 1) * IB)
            if t % 3 == 0:
                e.push_streams([0], f32[:1, sl])
            elif t % 3 == 1:
                e.push_streams_pcm16([0], dec16[:1, sl])
            else:
                e.push_streams_g711([0], codes[:1, sl], law)
        if (c // 3) % 2 == 0:
            e.push_streams_g711([3, 1, 2], codes[[3, 1, 2], c * IB:(c + nt) * IB], law)
        else:   # the same from device memory, at an odd address
            buf, _, stride, tick_stride = gu.strided(codes[[3, 1, 2]], c, nt, gu.GAP[law], lead=5)
            dev = torch.from_numpy(buf).to(torch.device("cuda", 0))
            e.push_streams_device([3, 1, 2], dev.data_ptr() + 5, stride, tick_stride, nt, g711=law)
            keep.append(dev)
        got.append(e.poll())
    e.sync()
    gu.assert_same(e, np.concatenate(got), ref, law)
    e.close()
