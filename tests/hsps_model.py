"""A scalar statement of the rule of swg_align_hsps* (include/swg.h), independent of the library and of the
oracle: the full matrix per round, a row-major scan for the best cell, a walk by predecessor codes, a set of used cells.

Alignment 0 is the three-state local alignment with the tie rules of swg.h.  Alignment r >= 1 is the same with the H
state of every used cell -- a cell an 'M' step of an earlier alignment of the pair went through -- at minus infinity;
the used cell's gap states A and B are computed as ever."""

NEG = -(1 << 29)


def _pick(m, x, y):
    return 0 if m == 0 else 1 if x == m else 2 if y == m else 3


def consensus(pssm):
    """Per position the lowest residue index in 1..31 whose score is the row's maximum over 1..31 (swg.h)."""
    out = []
    for row in pssm:
        at = 1
        for b in range(2, 32):
            if int(row[b]) > int(row[at]):
                at = b
        out.append(at)
    return out


def _fill(score, lq, len_, go, ge, used):
    """One round -> (best, bj, bi, codes) with codes[(j, i)] = (from of H, from of A, from of B); cells from 1."""
    zero = [0] * (lq + 1)
    Hp, Ap, Bp = zero[:], zero[:], zero[:]
    codes = {}
    best, bj, bi = 0, 0, 0
    for j in range(1, len_ + 1):
        H, A, B = zero[:], zero[:], zero[:]
        for i in range(1, lq + 1):
            hd, ad, bd = Hp[i - 1], Ap[i - 1], Bp[i - 1]
            mh = max(hd, ad, bd, 0)
            xa, ya, za = Hp[i] + go, Ap[i] + ge, Bp[i] + go
            ma = max(xa, ya, za, 0)
            xb, yb, zb = H[i - 1] + go, A[i - 1] + go, B[i - 1] + ge
            mb = max(xb, yb, zb, 0)
            codes[(j, i)] = (_pick(mh, hd, ad), _pick(ma, xa, ya), _pick(mb, xb, yb))
            h = NEG if (j, i) in used else mh + score(i - 1, j - 1)
            H[i], A[i], B[i] = h, ma, mb
            if h > best:                       # row by row: smallest database position, then smallest query position
                best, bj, bi = h, j, i
        Hp, Ap, Bp = H, A, B
    return best, bj, bi, codes


def align(sub, gap_open, gap_extend, seq, max_hsps, min_score, query=None, pssm=None):
    """-> (alignments, info).  alignments: dicts with score, q_begin, q_end, d_begin, d_end, n_ops, ops, n_ident, n_match,
    n_gap_open, n_gap and `cells`, the set of (j, i) of its M steps (from 1).  info: `stop` is "cap", "score" (the next
    best is positive and below min_score) or "exhausted" (nothing positive is left); `crossings` counts the gap-state
    steps of later paths that stand on a used cell."""
    assert (query is None) != (pssm is None)
    lq, len_ = len(query) if query is not None else len(pssm), len(seq)
    if query is not None:
        ident = [int(x) for x in query]

        def score(i, j):
            return int(sub[int(query[i])][int(seq[j])])
    else:
        ident = consensus(pssm)

        def score(i, j):
            return int(pssm[i][int(seq[j])])
    go, ge = gap_open + gap_extend, gap_extend
    used, out, crossings, stop = set(), [], 0, "cap"
    for _ in range(max_hsps):                  # (the loop runs out: the cap, without a further fill)
        best, j, i, codes = _fill(score, lq, len_, go, ge, used)
        if best < min_score:
            stop = "score" if best > 0 else "exhausted"
            break
        a = {"score": best, "q_end": i, "d_end": j}
        ops, cells, same, state = [], set(), 0, 1
        while j > 0 and i > 0 and len(ops) < lq + len_:
            c = codes[(j, i)]
            if state == 1:
                cells.add((j, i))
                same += ident[i - 1] == int(seq[j - 1])
                ops.append("M")
                frm = c[0]
                j, i = j - 1, i - 1
            elif state == 2:
                crossings += (j, i) in used
                ops.append("I")
                frm = c[1]
                j -= 1
            else:
                crossings += (j, i) in used
                ops.append("D")
                frm = c[2]
                i -= 1
            if frm == 0:
                break
            state = frm
        ops = "".join(reversed(ops))
        assert not (cells & used)
        used |= cells
        runs = sum(1 for k, op in enumerate(ops) if op != "M" and (k == 0 or ops[k - 1] != op))
        a.update(q_begin=i, d_begin=j, n_ops=len(ops), ops=ops, n_ident=same, n_match=ops.count("M"), n_gap_open=runs,
                 n_gap=len(ops) - ops.count("M"), cells=cells)
        out.append(a)
    return out, {"stop": stop, "crossings": crossings}
