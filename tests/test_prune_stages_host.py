"""CPU: the stages of a pruned fill and what is queued in front of each, through the hook
swg_debug_prune_stages -> swg_prune_stages, the one list the launch walks.

The rules, restated below in a few lines of Python: the stages are the segments, except that a lone segment is split at
head_pairs when the head is shorter than the segment.  Every stage but the first is cut, and under a caller's threshold
the first is cut too.  A cut stage gets the threshold kernel in front of it unless the threshold is the caller's; then
the prefix cut alone, or -- pair by pair -- the refine pass where there is a second level and the list.  The gate runs
only in front of the first of several stages, under a caller's threshold, with a second level."""
import pytest

ONE = [(0, 10)]
TWO = [(0, 6), (6, 10)]
THREE = [(0, 5), (5, 9), (9, 10)]


def _expected(segments, head_pairs=0, fixed=False, refine=0, prefix_cut=False):
    stages = []
    for i, (b, e) in enumerate(segments):
        mid = min(e, b + head_pairs) if len(segments) == 1 and head_pairs > 0 else e
        stages.append((b, mid, i))
        if mid < e:
            stages.append((mid, e, i))
    out = []
    for si, (b, e, i) in enumerate(stages):
        queued = []
        if si > 0 or fixed:
            if not fixed:
                queued.append("threshold")
            if prefix_cut:
                queued.append("prefix_cut")
            else:
                if refine and fixed and si == 0 and len(stages) > 1:
                    queued.append("gate")
                if refine:
                    queued.append("refine")
                queued.append("list")
        out.append((b, e, i, tuple(queued)))
    return out


CASES = [
    # one segment: split; no head; head equal to the segment; head longer than it
    (ONE, dict(head_pairs=4)), (ONE, dict(head_pairs=0)), (ONE, dict(head_pairs=10)), (ONE, dict(head_pairs=12)),
    # several segments: the head is ignored
    (THREE, dict(head_pairs=0)), (THREE, dict(head_pairs=4)),
    # a caller's threshold: the gate on stage 0 only, and only with a second level; one segment is one cut stage
    (THREE, dict(fixed=True, refine=0)), (THREE, dict(fixed=True, refine=128)), (ONE, dict(fixed=True)),
    # the second level without a caller's threshold
    (TWO, dict(refine=64)),
    # the prefix cut
    (THREE, dict(prefix_cut=True)),
]


@pytest.mark.parametrize("segments,plan", CASES)
def test_stages_follow_the_rules(swg, segments, plan):
    assert swg.debug_prune_stages(segments, **plan) == _expected(segments, **plan)


def test_the_answers_spelled_out(swg):
    """The same list read off by hand for the cases where one rule flips, so that a mistake shared by the hook and the
    restatement above does not pass."""
    cut, lst = ("threshold", "list"), ("list",)
    assert swg.debug_prune_stages(ONE, head_pairs=4) == [(0, 4, 0, ()), (4, 10, 0, cut)]
    for head in (0, 10, 12):
        assert swg.debug_prune_stages(ONE, head_pairs=head) == [(0, 10, 0, ())]
    for head in (0, 4):
        assert swg.debug_prune_stages(THREE, head_pairs=head) == [(0, 5, 0, ()), (5, 9, 1, cut), (9, 10, 2, cut)]
    assert swg.debug_prune_stages(THREE, fixed=True) == [(0, 5, 0, lst), (5, 9, 1, lst), (9, 10, 2, lst)]
    assert swg.debug_prune_stages(THREE, fixed=True, refine=128) == [
        (0, 5, 0, ("gate", "refine", "list")), (5, 9, 1, ("refine", "list")), (9, 10, 2, ("refine", "list"))]
    assert swg.debug_prune_stages(ONE, fixed=True) == [(0, 10, 0, lst)]
    assert swg.debug_prune_stages(ONE, fixed=True, refine=128) == [(0, 10, 0, ("refine", "list"))]
    assert swg.debug_prune_stages(TWO, refine=64) == [(0, 6, 0, ()), (6, 10, 1, ("threshold", "refine", "list"))]
    assert swg.debug_prune_stages(THREE, prefix_cut=True, refine=64) == [
        (0, 5, 0, ()), (5, 9, 1, ("threshold", "prefix_cut")), (9, 10, 2, ("threshold", "prefix_cut"))]
