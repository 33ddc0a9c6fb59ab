"""GPU (-m gpu): `mlp_adam_apply_kernel` and the two slab reductions request everything they read in one go and keep what they compute
bit for bit -- held against the commit before that reordering.

tests/golden/adam_round_trips.json holds a SHA-256 of every buffer a launch may write (P, PF, PT, PB, PTB, PH, PTH, exp_avg,
exp_avg_sq, the step words, the norm, h2_scales; for the gradient launches G, the norm partials, the step words, h2_overflow,
h2_scales) after every launch of the sequences in tests/adam_round_trips_seq.py, written by that module from a build of the
reference commit.  The digests are those of the code one compiler generates: the file records `hipcc --version`, and under another
compiler the comparison is skipped (the sequences' own assertions -- a refused step stores nothing, a due rescale happens -- are
part of running them and are not).  The sequences run twice in one process from the same start and must agree: state a launch
leaves behind for the next one (a cache keyed too loosely) would show there."""
import json
import os

import pytest

from tests import adam_round_trips_seq as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_round_trips.json")


@pytest.fixture(scope="module")
def reference():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("planes,steps,seed", S.SEQUENCES, ids=[s[0] for s in S.SEQUENCES])
def test_sequence_matches_the_reference_build_bit_for_bit(planes, steps, seed, reference):
    first = S.run_sequence(planes, steps, seed)
    S.check_facts(planes, first["facts"])
    second = S.run_sequence(planes, steps, seed)
    assert first == second, "two runs of the sequence in one process disagree"
    have = S.compiler_string()
    if have != reference["compiler"]:
        pytest.skip("the golden digests were recorded under another compiler (%r, here %r): nothing to compare bit for bit"
                    % (reference["compiler"].splitlines()[0], have.splitlines()[0]))
    want = reference["sequences"][planes]
    assert first["facts"] == want["facts"]
    assert [r[0] for r in first["records"]] == [r[0] for r in want["records"]]
    for (label, got), (_, ref) in zip(first["records"], want["records"]):
        assert set(got) == set(ref), label
        diff = sorted(k for k in got if got[k] != ref[k])
        assert not diff, (label, "buffers that differ from the reference build", diff)


def test_the_golden_file_covers_what_it_should(reference):
    for planes, steps, _ in S.SEQUENCES:
        recs = reference["sequences"][planes]["records"]
        S.check_facts(planes, reference["sequences"][planes]["facts"])
        step_recs = [r for r in recs if set(r[1]) == set(S.STEP_BUFFERS)]
        grad_recs = [r for r in recs if set(r[1]) == set(S.GRAD_BUFFERS)]
        assert len(step_recs) + len(grad_recs) == len(recs) and len(step_recs) >= steps
        assert any("/grad33" in r[0] for r in grad_recs) and any("/grad64" in r[0] for r in grad_recs)
    labels = [r[0] for r in reference["sequences"]["f16x2"]["records"]]
    for part in ("refused-mark", "refused-invalid-self_norm", "refused-invalid-norm_ready", "refused-before-rescale", "sticky-overflow"):
        assert any(part in lb for lb in labels), part
    assert any("tile-error" in r[0] for r in reference["sequences"]["f32"]["records"])
