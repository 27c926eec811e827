"""Level-3 front end on the CPU: the yardstick the GPU tests hold the kernels to.

* tests/whisper_frontend.py restates the semantics of ewk_whisper_features_* in float64 numpy.
  At 3000 frames it must equal transformers' float64 ``_np_extract_fbank_features`` within
  2e-7 -- that extractor's float32 output rounding -- on every case of the matrix.
* The matrix must exercise the front end (tones above the floor) and tell the restatement from
  nine mutants by at least ten times the bar.
* The bar is min(4 E, 2^-10), E the worst error of the parent's float32 torch front end over the
  same matrix (computed here, never hard-coded; 6.7e-5 was seen, so the bar is about 2.7e-4).
* The C ABI declares both calls and EWK_FEAT_BF16 without a version change.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import whisper_frontend as wf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = wf.matrix()


def _family(fam):
    return [i for i, c in enumerate(CASES) if c.family == fam]


def test_matrix_is_the_one_the_bar_is_stated_on():
    assert [c.name for c in CASES if c.family == "A"] == [f"tone{k}" for k in range(201)]
    assert [c.name for c in CASES if c.family == "B"] == [f"noise{n}" for n in wf.NOISE_LENGTHS] + ["quiet_then_loud"]
    assert [c.name for c in CASES if c.family == "C"] == ["len1", "len6400", "len48800", "zeros", "nan"]
    assert all(c.n_frames == (3000 if c.family == "C" else 8) for c in CASES)
    # live-frame counts on both sides of (L + 200) / 160
    assert [wf.n_live_frames(n, 8) for n in (2, 120, 121, 159, 160, 161, 1079, 1080, 1081, 1280, 2000)] == \
        [2, 2, 3, 3, 3, 3, 8, 8, 8, 8, 8]
    assert wf.n_live_frames(0, 8) == 0 and wf.n_live_frames(48800, 3000) == 307


@pytest.mark.parametrize("fam", ["A", "B", "C"])
def test_restatement_equals_transformers_yardstick(fam):
    refs = wf.references()
    worst, above = 0.0, 1.0
    for i in _family(fam):
        c = CASES[i]
        want = wf.yardstick(c.y)
        got = refs[i] if c.n_frames == 3000 else wf.features_ref(c.y, 3000)
        worst = max(worst, wf.max_err(got, want))
        if c.n_frames == 8 and len(c.raw) <= 1080:
            # nothing of these segments is cut and frame 7 reflects only zeros: the 8-frame
            # features are the first 8 columns of the 3000-frame ones
            assert wf.max_err(refs[i], got[:, :8]) <= 1e-12, c
        if fam == "A":   # the tones must not be compared as constants
            # (L + 4) / 4 puts the max - 8 floor at the output's maximum - 2
            above = min(above, float((want[:, :6] > want.max() - 2.0 + 1e-9).mean()))
    print(f"family {fam}: restatement vs yardstick {worst:.3g}; least share above the floor {above:.4f}")
    assert worst <= wf.YARDSTICK_BOUND
    if fam == "A":
        assert above >= 0.95


def test_special_cases_of_the_semantics():
    refs = wf.references()
    by_name = {c.name: r for c, r in zip(CASES, refs)}
    assert np.all(by_name["zeros"] == -1.5)
    assert np.isnan(by_name["nan"]).all()
    assert np.all(wf.features_ref(np.zeros(0), 8) == -1.5)
    r = by_name["len6400"]                      # 6400 samples: frames 0..41 live, the rest the floor constant
    top = (r.max() * 4.0 - 4.0)
    assert np.all(r[:, 42:] == (max(-10.0, top - 8.0) + 4.0) / 4.0)
    q = by_name["quiet_then_loud"]
    assert np.unravel_index(q.argmax(), q.shape)[1] == wf.n_live_frames(920, 8) - 1 == 6


def test_parent_error_sets_a_bar_and_mutants_exceed_it_tenfold():
    per = wf.parent_error()
    bar = wf.bar()
    print("parent float32 front end, worst error per family:", {k: f"{v:.3g}" for k, v in per.items()}, f"bar {bar:.3g}")
    assert 0.0 < per["all"] < wf.BAR_CAP and bar == min(4.0 * per["all"], wf.BAR_CAP)
    refs = wf.references()
    moved = {}
    for mut in wf.MUTANTS:
        worst = 0.0
        for c, r in zip(CASES, refs):
            if c.name == "nan":
                continue
            worst = max(worst, wf.max_err(wf.features_ref(c.y, c.n_frames, mutant=mut), r))
        moved[mut] = worst
    print("mutants move the matrix by:", {k: f"{v:.3g}" for k, v in moved.items()})
    weak = {k: v for k, v in moved.items() if not v >= 10.0 * bar}
    assert not weak, weak


def test_bf16_rounding_model_is_torch_rounding():
    import torch
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32),
                        np.array([0.0, -1.5, 1.0, 0.50390625, 0.501953125, 0.505859375, np.nan, -0.0], np.float32)])
    t = torch.from_numpy(a).to(torch.bfloat16)
    want = t.view(torch.int16).numpy().view(np.uint16)
    got = wf.bf16_round(a)
    finite = ~np.isnan(a)
    np.testing.assert_array_equal(got[finite], want[finite])
    # torch's NaN payload differs between its conversion paths; the kernel writes the quiet NaN 0x7FC0
    assert torch.isnan(t[torch.from_numpy(~finite)]).all() and np.all(got[~finite] == 0x7FC0)


def test_abi_declares_the_front_end():
    from easywakeword_amd import _lib
    src = open(os.path.join(ROOT, "include", "ewk.h")).read()
    assert re.search(r"#define\s+EWK_ABI_VERSION\s+4\b", src)
    m = re.search(r"#define\s+EWK_FEAT_BF16\s+(\d+)", src)
    assert m and int(m.group(1)) == _lib.EWK_FEAT_BF16
    assert _lib.EWK_FEAT_BF16 & (_lib.EWK_PCM_DEVICE | _lib.EWK_OUT_DEVICE) == 0
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+ewk_whisper_features_events\s*\(\s*ewk_engine\s*\*\s*e,\s*const\s+ewk_event\s*\*\s*events,"
                     r"\s*int32_t\s+n,\s*void\s*\*\s*out,\s*int32_t\s+n_frames,\s*int32_t\s+flags\s*\)", code)
    assert re.search(r"int\s+ewk_whisper_features_segments\s*\(\s*ewk_engine\s*\*\s*e,\s*const\s+float\s*\*\s*pcm,"
                     r"\s*int64_t\s+n_pcm,\s*const\s+int64_t\s*\*\s*offsets,\s*const\s+int32_t\s*\*\s*lengths,"
                     r"\s*int32_t\s+n_seg,\s*void\s*\*\s*out,\s*int32_t\s+n_frames,\s*int32_t\s+flags\s*\)", code)
    lib = _lib.load()
    assert lib.ewk_abi_version() == 4
    for name, n_args in (("ewk_whisper_features_events", 6), ("ewk_whisper_features_segments", 9)):
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args
    # refusals that need no device: a NULL engine
    buf = np.zeros(80 * 8, np.float32)
    rc = lib.ewk_whisper_features_events(None, None, 1, buf.ctypes.data_as(ctypes.c_void_p), 8, 0)
    assert rc == _lib.EWK_EINVAL and b"engine is NULL" in lib.ewk_last_error()
    rc = lib.ewk_whisper_features_segments(None, None, 0, None, None, 1, buf.ctypes.data_as(ctypes.c_void_p), 8, 0)
    assert rc == _lib.EWK_EINVAL and np.all(buf == 0)
