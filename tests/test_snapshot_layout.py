"""The record layout of a stream snapshot (ewk_snapshot_plan, csrc/ewk_snapshot_plan.h), without a
device: alignment, size, the fingerprint's dependence on the geometry and on nothing else, the
configurations it refuses -- through the library, and again by a stand-alone program that holds
the header alone, built by the host compiler with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import lifecycle_util as lu
from easywakeword_amd import _lib
from easywakeword_amd.snapshot import layout_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "easywakeword_amd", "csrc", "ewk_snapshot_plan.h")

# (name, configuration, input rate)
CONFIGS = [
    ("default", {}, 0),
    ("compact", dict(ring_samples=lu.min_ring(1600)), 0),
    ("compact_i16", dict(ring_samples=lu.min_ring(1600), ring_format=_lib.EWK_RING_I16), 0),
    ("block512", dict(block=512), 0),
    ("block512_i16", dict(block=512, ring_format=_lib.EWK_RING_I16), 0),
    ("rate48k", {}, 48000),
    ("rate8k", {}, 8000),
]


def plan(cfg, rate):
    out = _lib.EwkSnapshotLayout()
    rc = _lib.load().ewk_snapshot_plan(C.byref(_lib.default_config(**cfg)), int(rate), C.byref(out))
    _lib.check(rc)
    return layout_dict(out)


def expected_sections(l):
    """The sizes the format implies (include/ewk.h), in section order."""
    es = 2 if l["ring_format"] == _lib.EWK_RING_I16 else 4
    return [96, (_lib.EWK_LISTENERS_MAX - 1) * 40, 8 * l["n_blocks"], 8 * l["n_blocks"], es * l["sring_len"],
            4 * l["hist_len"], 16 if l["hist_len"] else 0, es * l["in_block"]]


@pytest.mark.parametrize("name, cfg, rate", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_sections_are_aligned_disjoint_and_sum_up(name, cfg, rate):
    l = plan(cfg, rate)
    assert (l["magic"], l["version"]) == (_lib.EWK_SNAPSHOT_MAGIC, _lib.EWK_SNAPSHOT_VERSION)
    secs = [l["sections"][n] for n in _lib.SNAP_SECTION_NAMES]
    assert [b for _, b in secs] == expected_sections(l)
    at = 0
    for off, nbytes in secs:
        assert off % 16 == 0 and off == at          # in order, each right behind the last one's padding
        at = off + -(-nbytes // 16) * 16
    assert l["record_bytes"] % 128 == 0
    assert l["record_bytes"] == -(-sum(-(-b // 16) * 16 for _, b in secs) // 128) * 128
    assert 0 <= l["record_bytes"] - at < 128


def test_geometry_of_the_covered_configurations():
    d = plan({}, 0)
    assert (d["n_blocks"], d["sring_len"], d["ring_len"], d["in_rate"], d["in_block"], d["hist_len"]) == \
        (100, 160000, 160000, 16000, 1600, 0)
    # 96 + 608 (600 padded) + 800 + 800 + 640000 + 6400 = 648704 = 5068 * 128
    assert d["sections"]["ring"][1] == 640000 and d["record_bytes"] == 648704
    c = plan(dict(ring_samples=lu.min_ring(1600), ring_format=_lib.EWK_RING_I16), 0)
    assert c["sring_len"] == lu.min_ring(1600) and c["sections"]["ring"][1] == 2 * lu.min_ring(1600)
    b = plan(dict(block=512), 0)
    assert b["n_blocks"] == 312
    r = plan({}, 48000)
    assert (r["in_rate"], r["in_block"], r["hist_len"]) == (48000, 4800, 62)   # J = 2 * 30 / 1 + 1 taps, J + 1 kept
    assert r["sections"]["fresh"][1] == 16
    assert plan({}, 16000) == d                    # the engine's own rate: no resampler
    i16 = plan(dict(ring_samples=48000, ring_format=_lib.EWK_RING_I16), 0)
    assert i16["sections"]["ring"][1] == 96000


def test_null_config_is_the_default():
    out = _lib.EwkSnapshotLayout()
    _lib.check(_lib.load().ewk_snapshot_plan(None, 0, C.byref(out)))
    assert layout_dict(out) == plan({}, 0)


GEOMETRY_CHANGES = [
    (dict(block=800), 0), (dict(buffer_seconds=5), 0), (dict(ring_samples=lu.min_ring(1600)), 0),
    (dict(ring_samples=lu.min_ring(1600) + 1600), 0), (dict(ring_format=_lib.EWK_RING_I16), 0),
    (dict(tick_seconds=0.05), 0), ({}, 48000), ({}, 8000), ({}, 32000),
]
NOT_GEOMETRY = [
    dict(pre_speech_silence=0.5), dict(speech_duration_min=0.2, speech_duration_max=1.5), dict(post_speech_silence=0.3),
    dict(padding=0.1), dict(max_segment_seconds=2.0), dict(similarity_threshold=60.0), dict(reentry_timeout=5.0),
    dict(min_threshold=0.01), dict(initial_threshold=0.02), dict(rescore_margin=1e-2),
]


def test_fingerprint_follows_the_geometry_and_nothing_else():
    base = plan({}, 0)
    prints = {base["fingerprint"]}
    for cfg, rate in GEOMETRY_CHANGES:
        fp = plan(cfg, rate)["fingerprint"]
        assert fp not in prints, (cfg, rate)
        prints.add(fp)
    for cfg in NOT_GEOMETRY:
        assert plan(cfg, 0) == base, cfg
    # the same with a rate set and a compact ring
    assert plan(dict(ring_samples=lu.min_ring(1600), padding=0.0), 0) == plan(dict(ring_samples=lu.min_ring(1600)), 0)
    assert plan(dict(post_speech_silence=0.3), 48000) == plan({}, 48000)


INVALID = [
    (dict(sample_rate=8000), 0, "sample_rate must be 16000"),
    (dict(buffer_seconds=0), 0, "buffer_seconds must be positive"),
    (dict(block=0), 0, "block must be in"),
    (dict(block=8193), 0, "block must be in"),
    (dict(tick_seconds=0.0), 0, "tick_seconds must be positive"),
    (dict(speech_duration_min=2.0, speech_duration_max=1.0), 0, "speech_duration_min must be <="),
    (dict(post_speech_silence=0.0), 0, "post_speech_silence must be positive"),
    (dict(ring_format=2), 0, "ring_format must be"),
    (dict(ring_samples=19200), 0, "longest segment request"),
    (dict(ring_samples=48000, block=512), 0, "block to divide"),
    (dict(ring_samples=-1), 0, "ring_samples must be in"),
    (dict(ring_samples=170000), 0, "ring_samples must be in"),
    ({}, -1, "in_rate must be"),
    ({}, 11025, "whole number of samples"),
    (dict(ring_format=_lib.EWK_RING_I16), 48000, "int16 ring"),
]


@pytest.mark.parametrize("cfg, rate, msg", INVALID)
def test_invalid_configurations_are_refused_and_nothing_is_written(cfg, rate, msg):
    out = _lib.EwkSnapshotLayout()
    C.memset(C.byref(out), 0xA5, C.sizeof(out))
    rc = _lib.load().ewk_snapshot_plan(C.byref(_lib.default_config(**cfg)), int(rate), C.byref(out))
    assert rc == _lib.EWK_EINVAL
    with pytest.raises(ValueError, match=msg):
        _lib.check(rc)
    assert bytes(out) == b"\xa5" * C.sizeof(out)


MAIN = r'''
#include <stdio.h>
#include <string.h>
#include "%s"
// stdin: per case "block ring_samples ring_format buffer_seconds tick_seconds in_rate".  stdout: the
// return code and, when 0, record_bytes, the fingerprint, n_blocks, in_block, hist_len and every
// section's offset and size.
int main() {
    int block, ring_samples, ring_format, buffer_seconds, in_rate;
    double tick;
    while (scanf("%%d %%d %%d %%d %%lf %%d", &block, &ring_samples, &ring_format, &buffer_seconds, &tick, &in_rate) == 6) {
        ewk_config c;
        memset(&c, 0, sizeof(c));
        c.sample_rate = 16000; c.buffer_seconds = buffer_seconds; c.block = block; c.ring_samples = ring_samples;
        c.tick_seconds = tick; c.pre_speech_silence = 0.8; c.speech_duration_min = 0.3; c.speech_duration_max = 2.0;
        c.post_speech_silence = 0.4; c.padding = 0.05; c.max_segment_seconds = 3.0; c.similarity_threshold = 75.0;
        c.min_threshold = 0.005; c.initial_threshold = 0.01; c.rescore_margin = 1e-3; c.ring_format = ring_format;
        ewk_snapshot_layout* l = new ewk_snapshot_layout;   // exact size on the heap: the sanitizer sees a write past it
        memset(l, 0x5a, sizeof(*l));
        const int rc = (int)ewk::snapshot_plan(&c, in_rate, l);
        printf("%%d", rc);
        if (rc == 0) {
            printf(" %%lld %%llu %%d %%d %%d", (long long)l->record_bytes, (unsigned long long)l->fingerprint, l->n_blocks,
                   l->in_block, l->hist_len);
            for (int k = 0; k < EWK_SNAP_SECTIONS; ++k)
                printf(" %%lld %%lld", (long long)l->section[k].offset, (long long)l->section[k].bytes);
        } else {
            const unsigned char* b = reinterpret_cast<const unsigned char*>(l);
            for (size_t i = 0; i < sizeof(*l); ++i) if (b[i] != 0x5a) return 3;   // a failure writes nothing
            if (!ewk::snapshot_plan_message((ewk::SnapshotPlanError)rc)[0]) return 4;
        }
        printf("\n");
        delete l;
    }
    return ewk::snapshot_plan(nullptr, 0, nullptr) == ewk::kSnapPlanArgs ? 0 : 5;
}
'''


def test_header_alone_under_sanitizers(tmp_path):
    """ewk_snapshot_plan.h needs no HIP: the host compiler builds it into a program of its own,
    which gives the library's answers for every covered and every refused configuration."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = tmp_path / "snap_main.cpp"
    src.write_text(MAIN % HDR)
    exe = tmp_path / "snap_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(src), "-o", str(exe)], check=True)
    todo = [(cfg, rate) for _, cfg, rate in CONFIGS] + GEOMETRY_CHANGES + \
        [(cfg, rate) for cfg, rate, _ in INVALID if set(cfg) <= {"block", "ring_samples", "ring_format", "buffer_seconds",
                                                                  "tick_seconds"}]
    lines = []
    for cfg, rate in todo:
        c = _lib.default_config(**cfg)
        lines.append(f"{c.block} {c.ring_samples} {c.ring_format} {c.buffer_seconds} {c.tick_seconds!r} {rate}")
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""
    out = r.stdout.strip().split("\n")
    assert len(out) == len(todo)
    for (cfg, rate), line in zip(todo, out):
        got = line.split()
        lay = _lib.EwkSnapshotLayout()
        rc = _lib.load().ewk_snapshot_plan(C.byref(_lib.default_config(**cfg)), int(rate), C.byref(lay))
        assert (int(got[0]) == 0) == (rc == 0), (cfg, rate, line)
        if rc:
            continue
        l = layout_dict(lay)
        want = [l["record_bytes"], l["fingerprint"], l["n_blocks"], l["in_block"], l["hist_len"]]
        for n in _lib.SNAP_SECTION_NAMES:
            want += list(l["sections"][n])
        assert [int(x) for x in got[1:]] == want, (cfg, rate)
