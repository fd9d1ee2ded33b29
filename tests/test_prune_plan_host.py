"""CPU: what a search decides about hits-only pruning, through the plan hook (swg_debug_prune_plan ->
swg_prune_plan, the one function swg_search_begin asks).

The rules: pruned only for k > 0 within the device top-K's capacity, no score array (option prune = 2 prunes with one),
non-positive gap scores, the 16-bit lane groups off the work queue with one class and one cell form, not a gapless
search and not a query of a batch call.  Option prune = 1 (auto) prunes ranges of several segments only, stage = segment,
and leaves a range of fewer than 4 x prune_head pairs per lane group alone.  Option prune = 2 also splits a range of one
segment into a head (at least k sequences = ceil(k / 2) pairs, and prune_head pairs per lane group, at most a quarter of
the range) and the rest."""
import pytest


def test_default_ask_is_pruned_by_segment(swg):
    assert swg.debug_prune_plan() == (True, 0)
    assert swg.debug_prune_plan(mode=2) == (True, 0)


@pytest.mark.parametrize("range_pairs", [1000, 1000000, 50000000])
def test_auto_never_splits_a_single_segment(swg, range_pairs):
    assert swg.debug_prune_plan(n_segments=1, range_pairs=range_pairs) == (False, 0)
    assert swg.debug_prune_plan(n_segments=0, range_pairs=range_pairs) == (False, 0)
    assert swg.debug_prune_plan(n_segments=1, range_pairs=range_pairs, mode=2)[0]


@pytest.mark.parametrize("groups,prune_head", [(1024, 4), (1000, 2), (12288, 8), (64, 1)])
def test_no_split_below_four_heads_per_lane_group(swg, groups, prune_head):
    floor = 4 * prune_head * groups
    # auto, several segments: the floor, and the stages are the segments
    assert swg.debug_prune_plan(range_pairs=floor - 1, groups=groups, prune_head=prune_head, n_segments=8) == (False, 0)
    assert swg.debug_prune_plan(range_pairs=floor, groups=groups, prune_head=prune_head, n_segments=8) == (True, 0)
    assert swg.debug_prune_plan(range_pairs=floor, groups=groups, prune_head=prune_head, n_segments=2) == (True, 0)
    # one segment (diagnostic mode only): from the floor on the head is prune_head pairs per lane group
    assert swg.debug_prune_plan(mode=2, n_segments=1, range_pairs=floor, groups=groups, prune_head=prune_head, k=10) == (True, prune_head * groups)
    assert swg.debug_prune_plan(mode=2, n_segments=1, range_pairs=floor - 4, groups=groups, prune_head=prune_head, k=2) == (True, prune_head * groups - 1)


@pytest.mark.parametrize("k", [1, 2, 99, 100, 101, 4096])
def test_head_holds_k_sequences(swg, k):
    # few lane groups: the k sequences decide
    on, head = swg.debug_prune_plan(mode=2, n_segments=1, k=k, groups=4, prune_head=4, range_pairs=100000)
    assert on and head == max((k + 1) // 2, 16) and 2 * head >= k
    # many: the lane groups do
    on, head = swg.debug_prune_plan(mode=2, n_segments=1, k=k, groups=4096, prune_head=4, range_pairs=1000000)
    assert on and head == max((k + 1) // 2, 4 * 4096) and 2 * head >= k


def test_k_as_large_as_the_range_is_not_pruned(swg):
    assert swg.debug_prune_plan(k=200, groups=1, prune_head=4, range_pairs=100, n_segments=1) == (False, 0)
    assert swg.debug_prune_plan(k=200, groups=1, prune_head=4, range_pairs=100, n_segments=1, mode=2) == (False, 0)
    assert swg.debug_prune_plan(k=198, groups=1, prune_head=4, range_pairs=100, n_segments=1, mode=2) == (True, 99)


def test_modes(swg):
    small = dict(range_pairs=2000, groups=8192, prune_head=4, k=10, n_segments=1)
    assert swg.debug_prune_plan(mode=0) == (False, 0)
    assert swg.debug_prune_plan(mode=0, **small) == (False, 0)
    assert swg.debug_prune_plan(mode=1, **small) == (False, 0)            # the size rule
    assert swg.debug_prune_plan(mode=2, **small) == (True, 500)           # ignored: a head of a quarter of the range
    assert swg.debug_prune_plan(mode=2, **dict(small, n_segments=5)) == (True, 0)
    assert swg.debug_prune_plan(mode=1, **dict(small, n_segments=5)) == (False, 0)
    assert swg.debug_prune_plan(mode=2, n_segments=1, range_pairs=2000, groups=8192, prune_head=0, k=10) == (True, 5)   # k sequences at least
    assert swg.debug_prune_plan(mode=2, n_segments=1, range_pairs=2000, groups=8192, prune_head=4, k=2000) == (True, 1000)
    # scores requested: only the diagnostic mode
    assert swg.debug_prune_plan(mode=1, want_scores=1) == (False, 0)
    assert swg.debug_prune_plan(mode=2, want_scores=1) == (True, 0)
    assert swg.debug_prune_plan(mode=2, want_scores=1, n_segments=1) == (True, 4 * 1024)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("excluded", [
    dict(k=0), dict(k=4097), dict(gap_open=1), dict(gap_extend=1), dict(gap_open=5, gap_extend=-1), dict(bits=32),
    dict(use_diag=0), dict(n_classes=2), dict(work_queue=0), dict(both_forms=1), dict(gapless=1), dict(batch=1),
    dict(range_pairs=0)], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_excluded_routes_stay_unpruned(swg, mode, excluded):
    """The long class (two classes), the both-forms split, the systolic engine and the int32 fills (no lane-group 16-bit
    fill), fixed streams (no work queue), gapless searches, the queries of swg_search_multi* / the lists' fall-back
    (batch), positive gap scores, and k outside the device top-K."""
    assert swg.debug_prune_plan(mode=mode, **excluded) == (False, 0)
    for seg in (1, 8):
        assert swg.debug_prune_plan(mode=mode, n_segments=seg, **excluded) == (False, 0)


def test_zero_gaps_are_on_the_packed_path(swg):
    assert swg.debug_prune_plan(gap_open=0, gap_extend=0)[0]
    assert swg.debug_prune_plan(gap_open=-11, gap_extend=-1)[0]


def test_hook_argument_errors(swg):
    assert swg.lib.swg_debug_prune_plan(None, None) == swg.SWG_ERR_ARG
    with pytest.raises(TypeError):
        swg.debug_prune_plan(nonsense=1)
    with pytest.raises(swg.SwgError):
        swg.debug_prune_plan(k=-1)
