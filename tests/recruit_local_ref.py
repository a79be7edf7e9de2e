"""The yardstick of Context.recruit in local mode (mgta_recruit_params.mode = MGTA_RECRUIT_LOCAL, include/megagta_hip.h) in plain
Python: every stop-free stretch of every frame, and within a stretch the best placement of any substring, as one sweep.

  all_stretches(tr, min_aa)     every maximal run without a stop of at least min_aa residues, ascending
  stretches(reads, min_aa)      the scored stretches of every frame of every read
  sweep(hm, seq)                the local sweep in three nested loops over Python floats, entry column and entry row carried
  sweep_many(hm, seqs)          the same operations element by element over numpy arrays across sequences (of any lengths: a sequence
                                takes no part in the rows behind its last residue) and columns, so every element sees the adds and
                                comparisons of the scalar loops
  combine(...)                  best stretch, status -> records; outputs(...) as in global mode

The sweep is the recurrence of tests/recruit_ref.score_carry with three changes: the match state of every row takes B = 0 as its first
candidate (entering at that row and column; B wins an equality), the delete state is fed by the match value WITHOUT its B candidate
(no delete straight after the first match), and the alignment ends in the match state of any row: the lowest column that reaches the
maximum, in it the lowest row.  Translation, the letters and the threshold are tests/recruit_ref's (a yardstick itself); nothing here
comes from the library."""
import numpy as np

from tests.recruit_ref import LN2, MM, MI, MD, IM, II, DM, DD, NEG, STABLE, frames, outputs  # noqa: F401


def all_stretches(tr, min_aa):
    """[(aa_from, aa_len)] of every maximal run without a stop that has at least max(1, min_aa) residues, ascending"""
    out, start = [], 0
    for p, c in enumerate(tr + "*"):
        if c == "*":
            if p - start >= max(1, min_aa):
                out.append((start, p - start))
            start = p + 1
    return out


def stretches(reads, min_aa):
    """[(read, frame, aa_from, aa_len, residues)] of every scored stretch: reads, frames and positions ascending"""
    out = []
    for r, codes in enumerate(reads):
        for f, tr in enumerate(frames(codes)):
            for a, n in all_stretches(tr, min_aa):
                out.append((r, f, a, n, tr[a:a + n]))
    return out


NONE = (NEG, 0, 0, 0, 0)


def sweep(hm, seq):
    """-> (score, model_from, model_to, first, length): the aligned span is seq[first:first + length]; (-inf, 0, 0, 0, 0) when no cell
    has a score"""
    M, L = hm.M, len(seq)
    msc, tsc, alpha = hm.msc.tolist(), hm.tsc.tolist(), hm.alpha.tolist()
    pM, pI, pD = [NEG] * (M + 1), [NEG] * (M + 1), [NEG] * (M + 1)
    pEM, pEI, pED = [None] * (M + 1), [None] * (M + 1), [None] * (M + 1)
    col_best = [(NEG, 0, None)] * (M + 1)                                 # per column: score, row, entry; the lowest row that reaches it
    for i in range(1, L + 1):
        x = ord(seq[i - 1])
        a = alpha[x] if x < 127 else -1
        cM, cI, cD, cC = [NEG] * (M + 1), [NEG] * (M + 1), [NEG] * (M + 1), [NEG] * (M + 1)
        eM, eI, eD, eC = [None] * (M + 1), [None] * (M + 1), [None] * (M + 1), [None] * (M + 1)
        for j in range(1, M + 1):
            e = msc[j][a] if a >= 0 else 0.0
            cont, ent = NEG, None                                         # the first of M, I, D that reaches their maximum
            if i > 1 and j > 1:
                cont, ent = pM[j - 1] + tsc[MM][j - 1], pEM[j - 1]
                v = pI[j - 1] + tsc[IM][j - 1]
                if v > cont:
                    cont, ent = v, pEI[j - 1]
                v = pD[j - 1] + tsc[DM][j - 1]
                if v > cont:
                    cont, ent = v, pED[j - 1]
            cC[j], eC[j] = cont + e, ent                                  # the match value without B
            if cont > 0.0:                                                # B = 0 is the first candidate
                cM[j], eM[j] = cont + e, ent
            else:
                cM[j], eM[j] = 0.0 + e, (j, i)
            if i > 1 and j < M:
                best, ent = pM[j] + tsc[MI][j], pEM[j]
                v = pI[j] + tsc[II][j]
                if v > best:
                    best, ent = v, pEI[j]
                cI[j], eI[j] = best, ent
            if i > 1 and j > 1:
                best, ent = cC[j - 1] + tsc[MD][j - 1], eC[j - 1]
                v = cD[j - 1] + tsc[DD][j - 1]
                if v > best:
                    best, ent = v, eD[j - 1]
                cD[j], eD[j] = best, ent
            if cM[j] > col_best[j][0]:
                col_best[j] = (cM[j], i, eM[j])
        pM, pI, pD, pEM, pEI, pED = cM, cI, cD, eM, eI, eD
    score, j_end = NEG, 0
    for j in range(1, M + 1):
        if col_best[j][0] > score:
            score, j_end = col_best[j][0], j
    if score == NEG:
        return NONE
    _, i_end, (j0, i0) = col_best[j_end]
    return score, j0, j_end, i0 - 1, i_end - i0 + 1


def sweep_many(hm, seqs, block=1024):
    """sweep of every sequence of `seqs` over numpy arrays -> [(score, model_from, model_to, first, length)].  The arrays run across
    the sequences (sorted by length and taken `block` at a time, so a block is swept only as far as its longest) and across the
    columns: the match and insert states of a row depend on the row before only, so all their columns are computed at once; the
    delete states of a row are a chain along the columns and are computed column after column.  Every element sees exactly the adds
    and comparisons of the scalar loops."""
    out = [NONE] * len(seqs)
    order = sorted(range(len(seqs)), key=lambda k: len(seqs[k]))
    for at in range(0, len(order), block):
        ks = order[at:at + block]
        for k, res in zip(ks, _sweep_block(hm, [seqs[k] for k in ks])):
            out[k] = res
    return out


def _sweep_block(hm, seqs):
    n, M = len(seqs), hm.M
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    L = int(lens.max())
    if L == 0:
        return [NONE] * n
    msc, tsc = np.asarray(hm.msc, dtype=np.float64), np.asarray(hm.tsc, dtype=np.float64)
    alpha = np.asarray(hm.alpha, dtype=np.int64)
    letters = np.zeros((n, L), dtype=np.int64)
    for k, s in enumerate(seqs):
        letters[k, :len(s)] = [ord(c) for c in s]
    col = np.where(letters < 127, alpha[np.minimum(letters, 126)], -1)
    SH = 1 << 32                                                          # an entry = row * SH + column
    cols = np.arange(M + 1, dtype=np.int64)[None, :]
    msc_t = np.ascontiguousarray(msc.T)                                   # [A, M + 1]

    def first_max(cands):
        best, ent = cands[0]
        for v, e in cands[1:]:
            take = v > best
            best, ent = np.where(take, v, best), np.where(take, e, ent)
        return best, ent

    # [n, M + 1] per state, column 0 stays -inf: it is what column 1 continues from
    pM, pI, pD = (np.full((n, M + 1), NEG) for _ in range(3))
    pEM, pEI, pED = (np.zeros((n, M + 1), dtype=np.int64) for _ in range(3))
    cb, cb_row, cb_ent = np.full((n, M + 1), NEG), np.zeros((n, M + 1), dtype=np.int64), np.zeros((n, M + 1), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(1, L + 1):
            a = col[:, i - 1]
            e = np.where((a >= 0)[:, None], msc_t[np.maximum(a, 0)], 0.0)
            # what continues into the match state of column j: M, I, D of column j - 1 in the row before (all -inf in row 1 and column 1)
            cont, ent = np.full((n, M + 1), NEG), np.zeros((n, M + 1), dtype=np.int64)
            cont[:, 1:], ent[:, 1:] = first_max([(pM[:, :-1] + tsc[MM][:-1], pEM[:, :-1]), (pI[:, :-1] + tsc[IM][:-1], pEI[:, :-1]), (pD[:, :-1] + tsc[DM][:-1], pED[:, :-1])])
            cC, eC = cont + e, ent                                        # the match value without B
            go_on = cont > 0.0                                            # B = 0 is the first candidate
            cM, eM = np.where(go_on, cont, 0.0) + e, np.where(go_on, ent, i * SH + cols)
            cM[:, 0] = NEG
            cI, eI = first_max([(pM + tsc[MI], pEM), (pI + tsc[II], pEI)])
            cI[:, 0] = cI[:, M] = NEG                                     # node M has no insert state
            # the delete states: a chain along the columns, fed by cC
            cCt, eCt = np.ascontiguousarray(cC.T), np.ascontiguousarray(eC.T)
            cDt, eDt = np.full((M + 1, n), NEG), np.zeros((M + 1, n), dtype=np.int64)
            for j in range(2, M + 1):
                cDt[j], eDt[j] = first_max([(cCt[j - 1] + tsc[MD][j - 1], eCt[j - 1]), (cDt[j - 1] + tsc[DD][j - 1], eDt[j - 1])])
            take = (lens >= i)[:, None] & (cM > cb)
            cb, cb_row, cb_ent = np.where(take, cM, cb), np.where(take, i, cb_row), np.where(take, eM, cb_ent)
            pM, pI, pD, pEM, pEI, pED = cM, cI, np.ascontiguousarray(cDt.T), eM, eI, np.ascontiguousarray(eDt.T)
    out = []
    for s in range(n):
        score = float(cb[s, 1:].max())
        if score == NEG:
            out.append(NONE)
            continue
        j = 1 + int(np.argmax(cb[s, 1:] == score))                        # the lowest column that reaches the score
        i0, j0 = divmod(int(cb_ent[s, j]), SH)
        out.append((score, j0, j, i0 - 1, int(cb_row[s, j]) - i0 + 1))
    return out


def score_all(hm, seqs, batch_len=51):
    """sweep_many over the sequences of at most batch_len residues (what a read of 150 bases gives) where there are enough of them to
    gain from arrays, sweep for the others, in the order of `seqs`"""
    short = [k for k, s in enumerate(seqs) if len(s) <= batch_len]
    if len(short) < 4:
        short = []
    out = [None] * len(seqs)
    for k, res in zip(short, sweep_many(hm, [seqs[k] for k in short])):
        out[k] = res
    return [sweep(hm, s) if res is None else res for s, res in zip(seqs, out)]


def combine(n_reads, stretch_list, scores):
    """the record of every read from its scored stretches and their sweeps -> list of dict(status, score, frame, aa_from, aa_len,
    model_from, model_to); aa_from, aa_len = the aligned span in the frame's translation (status 0), the whole first scored stretch
    (status 1)"""
    recs = [dict(status=2, score=NEG, frame=0, aa_from=0, aa_len=0, model_from=0, model_to=0) for _ in range(n_reads)]
    for (r, f, a, n, _), (score, m_from, m_to, first, length) in zip(stretch_list, scores):
        rec = recs[r]
        if rec["status"] == 2:
            rec.update(status=1, frame=f, aa_from=a, aa_len=n)
        if score > rec["score"]:                                          # frames and positions ascend: an equal score keeps the earlier stretch
            rec.update(status=0, score=score, frame=f, aa_from=a + first, aa_len=length, model_from=m_from, model_to=m_to)
    return recs


def recruit(hm, reads, min_aa=20, min_score=20 * LN2, scorer=None):
    """the yardstick end to end; scorer(seqs) -> [(score, model_from, model_to, first, length)] replaces the sweep"""
    sl = stretches(reads, min_aa)
    seqs = [s[4] for s in sl]
    scores = scorer(seqs) if scorer else score_all(hm, seqs)
    recs = combine(len(reads), sl, scores)
    out = outputs(recs, sl, hm.M, min_score)
    out.update(recs=recs, stretches=sl, scores=scores)
    return out
