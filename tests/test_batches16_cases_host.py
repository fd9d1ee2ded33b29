"""CPU: the calls of tests/batches16_cases.py are what they claim -- every shape present, every pair of lanes told
apart, the planted ceilings reached, a gap that pays across the passes, more than two staging runs -- and, where the
reference's own fill is built (oracle/_ref/), that alignment_fill_matrices itself gives these truths lane for lane
(wrapped where it wraps).  The GPU half (tests/test_gpu_batches16.py) then needs nothing of the reference."""
import numpy as np
import pytest

import batches16_cases as bc

CASES = {"shape_matrix": bc.shape_matrix, "shuffled": bc.shuffled, "ceilings": bc.ceilings, "multipass": bc.multipass,
         "staging": bc.staging, "mixed": bc.mixed}


def _columns(case):
    for b, (a, vs) in enumerate(case["batches"]):
        for l in range(vs):
            yield b, l, a[:, l]


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_are_legal_where_live_and_illegal_where_dead(name):
    c = CASES[name]()
    assert len(c["batches"]) == len(c["truth"])
    assert c["query"].min() >= 1 and c["query"].max() <= 30          # no residue 31: a pad row matches nothing
    dead = 0
    for (a, vs), t in zip(c["batches"], c["truth"]):
        assert a.dtype == np.int8 and a.ndim == 2 and a.shape[1] == 16 and a.shape[0] >= 1 and a.flags.c_contiguous
        assert 0 <= vs <= 16 and t.shape == (vs,) and t.dtype == np.int32
        live = a[:, :vs]
        assert live.size == 0 or (live.min() >= 1 and live.max() <= 31)
        for l in range(vs, 16):
            col = a[:, l].astype(np.int64)
            assert ((col < 1) | (col > 31)).all()
            dead += 1
    assert dead > 0
    assert all(int(t.max(initial=0)) != bc.SENTINEL and int(t.min(initial=0)) >= 0 for t in c["truth"])


def test_truth_is_the_oracle_on_the_columns_as_given(orc):
    """Spot check of the bookkeeping in batches16_cases._case: single pairs through orc.pair, pad rows included."""
    for name in ("shape_matrix", "ceilings", "multipass", "mixed"):
        c = CASES[name]()
        cols = list(_columns(c))
        for b, l, col in cols[::max(1, len(cols) // 25)]:
            assert orc.pair(c["query"], col, c["sub"], *c["gaps"]) == int(c["truth"][b][l]), (name, b, l)


def test_shape_matrix_covers_every_shape_and_tells_every_lane_apart():
    for seed in (0, 1):
        c = bc.shape_matrix(seed)
        seen = {(a.shape[0], vs) for a, vs in c["batches"]}
        assert {m for m, _ in seen} == set(bc.MAX_LENS) and {v for _, v in seen} == set(bc.VECTOR_SIZES)
        assert seen == {(m, v) for m in bc.MAX_LENS for v in bc.VECTOR_SIZES if m > 1 or v <= 3}
        for (a, vs), t in zip(c["batches"], c["truth"]):
            max_len = a.shape[0]
            if vs:
                assert int(t[0]) == 127 * max_len                     # lane 0: a copy of max_len columns
            for l in range(vs):
                n = int((a[:, l] != bc.PAD).sum())
                assert (a[n:, l] == bc.PAD).all() and int(t[l]) == 127 * n and (l == 0 or n < max_len)
            for i in range(vs // 2):
                assert t[2 * i] != t[2 * i + 1], (max_len, vs, i)
        # zero and odd counts in the middle of the call, not only last
        vss = [vs for _, vs in c["batches"]]
        assert any(v == 0 for v in vss[1:-1]) and any(v % 2 for v in vss[1:-1]) and vss[-1] not in (0,)
        assert [a.shape[0] for a, _ in c["batches"]] == sorted((a.shape[0] for a, _ in c["batches"]), reverse=True)
    assert not np.array_equal(bc.shape_matrix(0)["query"], bc.shape_matrix(1)["query"])


def test_shuffled_is_the_same_batches_out_of_order():
    c, s = bc.shape_matrix(), bc.shuffled()
    perm = bc.permutation(len(c["batches"]))
    assert sorted(perm) == list(range(len(c["batches"]))) and perm != sorted(perm)
    for k, i in enumerate(perm):
        assert s["batches"][k][0] is c["batches"][i][0] and s["batches"][k][1] == c["batches"][i][1]
        assert s["truth"][k] is c["truth"][i]
    lens = [a.shape[0] for a, _ in s["batches"]]
    assert lens != sorted(lens, reverse=True)                          # the library has to sort
    assert len(set(lens)) < len(lens)                                  # ... with ties


def test_ceilings_are_reached():
    c = bc.ceilings()
    assert len(c["query"]) == 600
    assert int((c["query"] == 30).sum()) == 1 and c["query"][0] == 30 and int((c["query"] == 29).sum()) == 1 and c["query"][-1] == 29
    t = np.concatenate(c["truth"])
    for v in bc.CEILINGS:
        assert int((t == v).sum()) >= bc.PER_CEILING, v
    planted = np.isin(t, bc.CEILINGS)
    assert int((~planted).sum()) >= 16 and int(t[~planted].max()) < 1000 and int(t[~planted].min()) >= 100   # the hundreds
    # each ceiling value sits in an even and in an odd lane somewhere, and next to a small neighbour somewhere
    lanes = np.concatenate([np.arange(len(x)) for x in c["truth"]])
    for v in bc.CEILINGS:
        assert {int(l) % 2 for l in lanes[t == v]} == {0, 1}, v
    assert any(vs % 2 for _, vs in c["batches"])


def test_multipass_has_gaps_that_pay_across_the_passes(orc):
    c = bc.multipass()
    lq = len(c["query"])
    assert lq == bc.MULTIPASS_LQ > 64 * 32
    assert max(a.shape[0] for a, _ in c["batches"]) == 60
    paid, across = 0, set()
    for b, l in c["gapped"]:
        sc, co, ops = orc.pair_trace(c["query"], c["batches"][b][0][:, l], c["sub"], *c["gaps"])
        assert sc == int(c["truth"][b][l])
        paid += ("I" in ops or "D" in ops)
    for b, l, col in _columns(c):
        sc, co, ops = orc.pair_trace(c["query"], col, c["sub"], *c["gaps"])
        across |= {e for e in bc.MULTIPASS_BOUNDARIES if co[0] < e < co[1]}
    assert paid >= 20, paid
    assert across == set(bc.MULTIPASS_BOUNDARIES), across
    t = np.concatenate(c["truth"])
    assert int((t >= 4096).sum()) >= 8 and int((t < 4096).sum()) >= 8     # either side of the f16 cells' flag


def test_staging_needs_three_runs_and_plants_at_both_ends(orc):
    c = bc.staging()
    assert bc.staged_bytes(c) > 9 * 1000 * 1000
    # the runs as the library cuts them: batches longest first, a run closed once it holds 4 MB
    sizes = sorted((a.shape[0] * 16 for a, _ in c["batches"]), reverse=True)
    runs, cur = 0, 0
    for s in sizes:
        cur += s
        if cur >= bc.STAGE_RUN:
            runs, cur = runs + 1, 0
    runs += cur > 0
    assert runs >= 3
    lens = [a.shape[0] for a, _ in c["batches"]]
    assert lens != sorted(lens, reverse=True) and len(c["batches"]) == len(bc.STAGING_LONG) + 30
    where = set()
    for b, l, row, n in c["planted"]:
        max_len = c["batches"][b][0].shape[0]
        where.add("first" if row == 0 else "last" if row + n == max_len else "middle")
        # the copy makes the lane's score: without its rows the score drops
        col = c["batches"][b][0][:, l].copy()
        col[row:row + n] = bc.PAD
        assert int(c["truth"][b][l]) >= 127 * n > orc.pair(c["query"], col, c["sub"], *c["gaps"]) + 127
    assert where == {"first", "middle", "last"}
    for b in range(len(bc.STAGING_LONG)):
        assert c["truth"][b][0] != c["truth"][b][1]
    assert sum(a.shape[0] * vs for a, vs in c["batches"]) * len(c["query"]) < 50 * 1000 * 1000     # cells: small


def test_mixed_has_every_vector_size():
    c = bc.mixed()
    assert {vs for _, vs in c["batches"]} == set(range(17))
    t = np.concatenate(c["truth"])
    assert int(t.max()) < 4096 and len(set(t.tolist())) > 30


@pytest.mark.parametrize("name", sorted(set(CASES) - {"shuffled"}))
def test_reference_gives_these_truths(orc, name):
    """The reference's own alignment_fill_matrices on every batch (its dead lanes replaced by pad rows: it would index its
    table with them): the truth on every live lane whose truth is below 32767, the wrapped score on the rest."""
    if not orc.have_ref():
        pytest.skip("oracle/_ref/libswref.so not built (reference not mounted)")
    c = CASES[name]()
    wrapped = 0
    for b, (a, vs) in enumerate(c["batches"]):
        if vs == 0:
            continue
        clean = a.copy()
        clean[:, vs:] = bc.PAD
        ref = orc.ref_batch16(c["query"], clean, c["sub"], *c["gaps"])
        for l in range(vs):
            t = int(c["truth"][b][l])
            if t < 32767:
                assert int(ref[l]) == t, (name, b, l)
            else:
                wrapped += 1
                assert int(ref[l]) == orc.pair_wrap16(c["query"], a[:, l], c["sub"], *c["gaps"]), (name, b, l, t)
    assert (wrapped > 0) == (name == "ceilings")
