"""GPU (-m gpu): the head of `mlp_fused_step_h2_kernel` requests everything it reads before its first wait (layer 1's first weight
fragments, the loss constants, scales and biases with the first x DMA) and reads a share of the weight planes to warm its XCD's L2;
the tile loop skips its own request of those fragments for a workgroup's first tile.  That is scheduling only: everything one
`mlp_fused_grad_h2` call (fused launch + slab reduction) leaves behind is held bit for bit against the commit before the change.

tests/golden/fused_h2_heads.json holds the SHA-256 digests, written by tests/fused_h2_heads_cases.py from a build of the parent commit
(the file names it).  The shapes are the smallest at which the changed code can go wrong: 1 row (one workgroup, one ragged tile), 33
rows (a whole and a ragged tile), 32 * 256 + 1 rows (exactly one workgroup walks a second, ragged tile: the first-tile flag must
clear), 32 * 257 rows with x one float off 16-byte alignment (the plain-load fetch path), and 8193 rows on 7 workgroups (many tiles
per workgroup); each under a frozen and a live scale table.  The inputs hold no NaN and overflow nothing (run_case asserts it)."""
import json
import os

import pytest

from tests import fused_h2_heads_cases as H

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_h2_heads.json")


@pytest.fixture(scope="module")
def reference():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def policy():
    return H.make_policy()


@pytest.mark.parametrize("case", H.CASES, ids=[c[0] for c in H.CASES])
def test_one_call_leaves_what_the_parent_build_leaves(case, policy, reference):
    pol, sd = policy
    got = H.run_case(pol, sd, case)
    want = reference["cases"][case[0]]
    assert set(got) == set(H.TABLES) == set(want)
    for table in H.TABLES:
        assert set(got[table]) == set(H.BUFFERS) == set(want[table]), table
        diff = sorted(k for k in H.BUFFERS if got[table][k] != want[table][k])
        assert not diff, (case[0], table, "buffers that differ from the parent build", diff)


def test_the_golden_file_names_its_parent_and_covers_every_case(reference):
    assert len(reference["parent"]) == 40 and int(reference["parent"], 16) >= 0
    assert set(reference["cases"]) == {c[0] for c in H.CASES}
    live = [reference["cases"][c[0]]["live"]["h2_scales"] != reference["cases"][c[0]]["frozen"]["h2_scales"] for c in H.CASES]
    assert all(live), "a live table records the launch's maxima (fsc[32 ..]) at least: its digest differs from the frozen one"
