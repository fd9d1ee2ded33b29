"""CPU: the pruned search's host decisions, held to what they answered before the refinement levels became rows of one table
(tests/golden/grids/prune_levels_grid.npz, recorded by tests/golden/make_prune_levels_grid.py): the chain of levels, the gate
and the stage list over the grids of prune_levels_grid.py, array for array; and every hook from before a level was added
answers the matching columns of the full hook with the later options at 0 -- which is what lets them share one body."""
import os

import numpy as np
import pytest

import prune_levels_grid as grid
from conftest import GOLDEN_DIR


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN_DIR, "grids", "prune_levels_grid.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def answers(swg):
    return grid.compute(swg)


def _same(name, inputs, got_rc, got, want_rc, want):
    assert got.shape == want.shape and got_rc.shape == want_rc.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero((got_rc != want_rc) | np.any((got != want).reshape(len(got), -1), axis=1))
    if len(bad):
        i = int(bad[0])
        print("%s: %d rows differ; the first, row %d: in = %s\n  recorded: rc %d, %s\n  now:      rc %d, %s" % (
            name, len(bad), i, inputs[i].tolist(), want_rc[i], want[i].tolist(), got_rc[i], got[i].tolist()))
    assert len(bad) == 0, name


def test_the_chain_of_levels_answers_as_recorded(golden, answers):
    inputs = grid.choice_inputs()
    assert len(inputs) == 82944
    _same("choice", inputs, answers["choice_rc"], answers["choice_out"], golden["choice_rc"], golden["choice_out"])
    assert not np.any(golden["choice_rc"]) and len(np.unique(golden["choice_out"], axis=0)) == 120


def test_the_gate_answers_as_recorded(golden, answers):
    _same("gate", grid.gate_inputs(), answers["gate_rc"], answers["gate_out"], golden["gate_rc"], golden["gate_out"])
    assert not np.any(golden["gate_rc"]) and set(np.unique(golden["gate_out"][:, 2]).tolist()) == {0, 1}


def test_the_stage_list_answers_as_recorded(golden, answers):
    _same("stages", grid.stage_inputs(), answers["stage_rc"], answers["stage_out"], golden["stage_rc"], golden["stage_out"])
    assert not np.any(golden["stage_rc"])


# (hook, words of in it reads, answers it gives): the hooks from before the third, fourth and fifth levels
CHOICE_PREFIXES = (("swg_debug_prune_refine_choice", 8, 3), ("swg_debug_prune_refine3_choice", 10, 4), ("swg_debug_prune_refine4_choice", 12, 5))


@pytest.mark.parametrize("hook, n_in, n_out", CHOICE_PREFIXES)
def test_an_earlier_choice_hook_is_the_full_hooks_first_columns(swg, answers, hook, n_in, n_out):
    inputs = grid.choice_inputs()
    later = inputs[:, n_in:].copy()
    later[:, [c - n_in for c in (9, 11, 13, 14) if c >= n_in]] = 0  # (the widths and the fifth level's two flags are no options: any)
    rows = np.flatnonzero(~np.any(later, axis=1))
    assert len(rows) >= 3072
    rc, out = grid.run_choice_hook(getattr(swg.lib, hook), inputs[rows, :n_in], n_out)
    _same(hook, inputs[rows], rc, out, answers["choice_rc"][rows], answers["choice_out"][rows, :n_out].astype(np.int64))


# (hook, words in front of the segments): the hooks from before the third level, the fourth, the gate and the fifth;
# the words they lack, by their place in the full hook's head (refine3, refine4, gate, refine5, n)
STAGE_PREFIXES = (("swg_debug_prune_stages", 5), ("swg_debug_prune_stages3", 6), ("swg_debug_prune_stages4", 7), ("swg_debug_prune_stages5", 8))


@pytest.mark.parametrize("hook, head", STAGE_PREFIXES)
def test_an_earlier_stage_hook_is_the_full_hook_with_the_later_words_at_zero(swg, answers, hook, head):
    inputs = grid.stage_inputs()
    keep = list(range(head - 1))                                    # (the hook's own words; its last is n)
    rows = np.flatnonzero(~np.any(inputs[:, head - 1:8], axis=1))
    assert len(rows) >= 32
    short = np.concatenate([inputs[rows][:, keep], inputs[rows][:, 8:]], axis=1)
    rc, out = grid.run_stage_hook(getattr(swg.lib, hook), short)
    _same(hook, inputs[rows], rc, out, answers["stage_rc"][rows], answers["stage_out"][rows].astype(np.int64))
