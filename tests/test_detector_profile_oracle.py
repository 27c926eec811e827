"""tests/profile_cases.py on the CPU: the memoised ring buffer equals the plain oracle, and the
recipe of the GPU tests has the properties those tests lean on."""
import profile_cases as pc
from oracle.gate_ref import run_stream


def test_memo_buffer_equals_the_plain_oracle():
    case = pc.main_case()
    for i in (1, 2, 3):   # a short-window profile, the skipping one, the re-entering one
        cfg = pc.gate_config(int(case["assign"][i]))
        plain = run_stream(case["data"][i], cfg, keep_audio=False)
        memo = case["ref"][i]
        assert pc.key(memo) == pc.key(plain.events)
        assert [(e.time, e.n_request, e.end_trim) for e in memo] == [(e.time, e.n_request, e.end_trim) for e in plain.events]


def test_recipe_tells_profiles_from_the_configuration():
    case = pc.main_case()
    pc.assert_recipe_tells(case)
    assert sum(len(r) for r in case["ref"]) == 27
    assert [i for i in range(pc.N) if any(e.skipped for e in case["ref"][i])] == [2, 7]   # profile 1's streams
