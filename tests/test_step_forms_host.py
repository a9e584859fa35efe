"""Completeness of tests/step_form_cases.py against the option table (csrc/engine_options.hpp), on the host: every name that
ma_engine_set_option / ma_engine_get_option knows is either the switch of a case of tests/test_gpu_step_forms.py or listed in EXEMPT with the
reason.  A switch that is added to the table without a numbers test fails here."""
import os
import re

import step_form_cases as S

TABLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "meshanything_amd", "csrc", "engine_options.hpp")


def option_names():
    with open(TABLE) as f:
        return re.findall(r'\.name = "(\w+)"', f.read())


def test_every_option_is_a_case_or_exempt():
    names = option_names()
    assert len(names) > 40 and len(set(names)) == len(names), names
    missing = S.uncovered(names)
    assert not missing, f"options without a row in step_form_cases.CASES and without a reason in EXEMPT: {missing}"
    # nothing stale, nothing claimed twice
    assert sorted(S.covered() - set(names)) == [] and sorted(set(S.EXEMPT) - set(names)) == []
    assert sorted(S.covered() & set(S.EXEMPT)) == []
    assert all(isinstance(r, str) and r.strip() for r in S.EXEMPT.values())


def test_a_deleted_row_is_named():
    """The check sees what it is for: without the rows of one switch, that switch is reported."""
    names = option_names()
    for gone in ("mfma_ln_waves", "gemv_k8_ksplit", "attn_impl"):
        rest = [c for c in S.CASES if gone not in dict(c.switch)]
        assert len(rest) < len(S.CASES)
        assert S.uncovered(names, cases=rest) == [gone]
    assert S.uncovered(names, exempt={k: v for k, v in S.EXEMPT.items() if k != "use_graph"}) == ["use_graph"]


def test_table_is_well_formed():
    ids = [c.id for c in S.CASES]
    assert len(set(ids)) == len(ids), ids
    names = set(option_names())
    for c in S.CASES:
        assert c.relation in (S.IDENTICAL, S.REORDERED) and c.reason.strip(), c.id
        assert c.switch and 1 <= c.B <= 64 and set(c.policies) <= {"bf16", "fp16", "fp32"}, c.id
        assert {k for k, _ in c.prereq + c.switch} <= names, c.id
        assert not set(dict(c.prereq)) & set(dict(c.switch)), c.id
    # a placement-only switch has nothing to show but bit-equal logits; its gates are option names
    for name, gates in S.PLACEMENT_ONLY.items():
        assert all(c.relation == S.IDENTICAL for c in S.CASES if name in dict(c.switch)), name
        assert name in S.covered() and {k for k, _ in gates} <= names, name
    for (policy, name, value), why in S.NOTHING_MOVES.items():
        assert any(policy in c.policies and dict(c.switch).get(name) == value for c in S.CASES) and why.strip(), (policy, name, value)
