"""The Tsit45 checker computes what its three programs computed before they became one: every case of tests/golden/make_erk_checker_parity.py run again, the
sha256 of every array the fixture names (tests/golden/erk_checker_parity.json, recorded once before the merge and not regenerated) compared with the one
recorded, and `failed`, the first member's statistics or the counters in clear.  The fixture was recorded with the portable pow on models of + - * / alone, so
it holds on any x86-64 host.  A module may return more than the fixture names (erk_sens_ref's ncols); what it names must be there, bit for bit."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_erk_checker_parity as G  # noqa: E402

with open(G.FIXTURE) as _f:
    RECORDED = {r["name"]: r for r in json.load(_f)}


def test_the_fixture_and_the_case_list_name_the_same_cases():
    assert [c["name"] for c in G.CASES] == list(RECORDED)


@pytest.mark.parametrize("case", G.CASES, ids=[c["name"] for c in G.CASES])
def test_the_checker_computes_what_was_recorded(case):
    want, got = RECORDED[case["name"]], G.run_case(case)
    for key in want:
        if key == "arrays":
            for name, h in want["arrays"].items():
                assert name in got["arrays"], (case["name"], name, "not returned")
                assert got["arrays"][name] == h, (case["name"], name)
        else:
            assert got[key] == want[key], (case["name"], key, got[key], want[key])
