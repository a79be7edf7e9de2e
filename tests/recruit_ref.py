"""The yardstick of Context.recruit (mgta_reads_recruit, include/megagta_hip.h) in plain Python: translation, stretch choice, frame
choice, threshold and column depth, and the score of mgta_seqs_align restated with the entry column carried instead of traced back.

  score_carry(hm, seq)          three nested loops over Python floats (IEEE doubles, one add per +)
  score_carry_equal(hm, seqs)   the same operations element by element over numpy arrays across sequences of EQUAL length: every
                                array element sees exactly the adds and comparisons of the scalar loops, so it is exact too
  stretches(reads, min_aa)      the scored stretch of every frame of every read
  combine(...)                  best frame, status, threshold -> records; outputs(...) -> hit bits, column depth, the stable stats

Not the code under test and not derived from it: it shares nothing with the library but the rule's text."""
import numpy as np

CODON = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"   # codon = 16 b0 + 4 b1 + b2, A C G T = 0 .. 3
NEG = float("-inf")
MM, MI, MD, IM, II, DM, DD = range(7)
LN2 = 0.6931471805599453
MAX_BASES = 3 * 4096 + 2


def codes_of(text):
    return np.array(["ACGT".index(c) for c in text], dtype=np.uint8)


def translate(codes):
    c = [int(x) for x in codes]
    return "".join(CODON[16 * c[i] + 4 * c[i + 1] + c[i + 2]] for i in range(0, len(c) - 2, 3))


def frames(codes):
    """the six translations: frames 0 .. 2 the read as sequenced from base f, 3 .. 5 its reverse complement from base f - 3"""
    codes = np.asarray(codes, dtype=np.uint8)
    rc = (3 - codes[::-1]).astype(np.uint8)
    return [translate(codes[f:]) for f in range(3)] + [translate(rc[f:]) for f in range(3)]


def stretch(tr):
    """(aa_from, aa_len) of the longest run without a stop, the first of equally long ones; (0, 0) when there is none"""
    best_from, best_len, start = 0, 0, 0
    for p, c in enumerate(tr + "*"):
        if c == "*":
            if p - start > best_len:
                best_from, best_len = start, p - start
            start = p + 1
    return best_from, best_len


def stretches(reads, min_aa):
    """[(read, frame, aa_from, aa_len, residues)] of every scored stretch, reads and frames ascending"""
    out = []
    for r, codes in enumerate(reads):
        for f, tr in enumerate(frames(codes)):
            a, n = stretch(tr)
            if n >= max(1, min_aa):
                out.append((r, f, a, n, tr[a:a + n]))
    return out


def score_carry(hm, seq):
    """-> (score, model_from, model_to); (-inf, 0, 0) when no path has a score"""
    M, L = hm.M, len(seq)
    msc, tsc, alpha = hm.msc.tolist(), hm.tsc.tolist(), hm.alpha.tolist()
    if L == 0:
        return NEG, 0, 0
    pM, pI, pD = [NEG] * (M + 1), [NEG] * (M + 1), [NEG] * (M + 1)
    pEM, pEI, pED = [0] * (M + 1), [0] * (M + 1), [0] * (M + 1)
    for i in range(1, L + 1):
        x = ord(seq[i - 1])
        a = alpha[x] if x < 127 else -1
        cM, cI, cD = [NEG] * (M + 1), [NEG] * (M + 1), [NEG] * (M + 1)
        eM, eI, eD = [0] * (M + 1), [0] * (M + 1), [0] * (M + 1)
        for j in range(1, M + 1):
            e = msc[j][a] if a >= 0 else 0.0
            # the match state: B on row 1, else the first of M, I, D that reaches the maximum
            if i == 1:
                best, ent = 0.0, j
            elif j > 1:
                best, ent = pM[j - 1] + tsc[MM][j - 1], pEM[j - 1]
                v = pI[j - 1] + tsc[IM][j - 1]
                if v > best:
                    best, ent = v, pEI[j - 1]
                v = pD[j - 1] + tsc[DM][j - 1]
                if v > best:
                    best, ent = v, pED[j - 1]
            else:
                best, ent = NEG, 0
            cM[j], eM[j] = best + e, ent                                  # the maximum first, then + e
            if i > 1 and j < M:
                best, ent = pM[j] + tsc[MI][j], pEM[j]
                v = pI[j] + tsc[II][j]
                if v > best:
                    best, ent = v, pEI[j]
                cI[j], eI[j] = best, ent
            if i > 1 and j > 1:
                best, ent = cM[j - 1] + tsc[MD][j - 1], eM[j - 1]
                v = cD[j - 1] + tsc[DD][j - 1]
                if v > best:
                    best, ent = v, eD[j - 1]
                cD[j], eD[j] = best, ent
        pM, pI, pD, pEM, pEI, pED = cM, cI, cD, eM, eI, eD
    score = max(pM[1:])
    if score == NEG:
        return NEG, 0, 0
    j = pM.index(score, 1)                                                # the lowest column that reaches the score
    return score, pEM[j], j


def score_carry_equal(hm, seqs):
    """score_carry of every sequence of `seqs`, all of one length, vectorised ACROSS the sequences -> [(score, model_from, model_to)]"""
    n = len(seqs)
    if n == 0:
        return []
    M, L = hm.M, len(seqs[0])
    assert all(len(s) == L for s in seqs)
    if L == 0:
        return [(NEG, 0, 0)] * n
    msc, tsc = np.asarray(hm.msc, dtype=np.float64), np.asarray(hm.tsc, dtype=np.float64)
    alpha = np.asarray(hm.alpha, dtype=np.int64)
    letters = np.array([[ord(c) for c in s] for s in seqs], dtype=np.int64)             # [n, L]
    col = np.where(letters < 127, alpha[np.minimum(letters, 126)], -1)
    ninf, zero = np.full(n, NEG), np.zeros(n, dtype=np.int64)
    pM, pI, pD = [ninf] * (M + 1), [ninf] * (M + 1), [ninf] * (M + 1)
    pEM, pEI, pED = [zero] * (M + 1), [zero] * (M + 1), [zero] * (M + 1)

    def first_max(cands):
        best, ent = cands[0]
        for v, e in cands[1:]:
            take = v > best
            best, ent = np.where(take, v, best), np.where(take, e, ent)
        return best, ent

    with np.errstate(invalid="ignore"):
        for i in range(1, L + 1):
            a = col[:, i - 1]
            cM, cI, cD = [ninf] * (M + 1), [ninf] * (M + 1), [ninf] * (M + 1)
            eM, eI, eD = [zero] * (M + 1), [zero] * (M + 1), [zero] * (M + 1)
            for j in range(1, M + 1):
                e = np.where(a >= 0, msc[j][np.maximum(a, 0)], 0.0)
                if i == 1:
                    best, ent = np.zeros(n), np.full(n, j, dtype=np.int64)
                elif j > 1:
                    best, ent = first_max([(pM[j - 1] + tsc[MM][j - 1], pEM[j - 1]), (pI[j - 1] + tsc[IM][j - 1], pEI[j - 1]), (pD[j - 1] + tsc[DM][j - 1], pED[j - 1])])
                else:
                    best, ent = ninf, zero
                cM[j], eM[j] = best + e, ent
                if i > 1 and j < M:
                    cI[j], eI[j] = first_max([(pM[j] + tsc[MI][j], pEM[j]), (pI[j] + tsc[II][j], pEI[j])])
                if i > 1 and j > 1:
                    cD[j], eD[j] = first_max([(cM[j - 1] + tsc[MD][j - 1], eM[j - 1]), (cD[j - 1] + tsc[DD][j - 1], eD[j - 1])])
            pM, pI, pD, pEM, pEI, pED = cM, cI, cD, eM, eI, eD
    last = np.stack(pM[1:], axis=1)                                       # [n, M]
    ents = np.stack(pEM[1:], axis=1)
    out = []
    for s in range(n):
        score = float(last[s].max())
        if score == NEG:
            out.append((NEG, 0, 0))
            continue
        j = int(np.argmax(last[s] == score))                              # the lowest column that reaches the score
        out.append((score, int(ents[s, j]), j + 1))
    return out


def score_all(hm, seqs):
    """score_carry_equal group by group of equal length (score_carry where a group is too small to gain from arrays), in the order of
    `seqs`"""
    by_len = {}
    for k, s in enumerate(seqs):
        by_len.setdefault(len(s), []).append(k)
    out = [None] * len(seqs)
    for ks in by_len.values():
        group = [seqs[k] for k in ks]
        for k, res in zip(ks, score_carry_equal(hm, group) if len(ks) >= 4 else [score_carry(hm, s) for s in group]):
            out[k] = res
    return out


def combine(n_reads, stretch_list, scores):
    """the record of every read from its scored stretches (stretch_list as `stretches` gives it) and their (score, model_from,
    model_to) -> list of dict(status, score, frame, aa_from, aa_len, model_from, model_to)"""
    recs = [dict(status=2, score=NEG, frame=0, aa_from=0, aa_len=0, model_from=0, model_to=0) for _ in range(n_reads)]
    for (r, f, a, n, _), (score, m_from, m_to) in zip(stretch_list, scores):
        rec = recs[r]
        if rec["status"] == 2:                                            # the lowest scored frame, until a frame has a score
            rec.update(status=1, frame=f, aa_from=a, aa_len=n)
        if score > rec["score"]:                                          # frames ascend: an equal score keeps the lower frame
            rec.update(status=0, score=score, frame=f, aa_from=a, aa_len=n, model_from=m_from, model_to=m_to)
    return recs


def outputs(recs, stretch_list, M, min_score):
    """-> dict(bits = bool[n], col_depth = uint64[M], stats = the fields of mgta_recruit_stats that are functions of the input)"""
    n = len(recs)
    bits = np.array([r["status"] == 0 and r["score"] >= min_score for r in recs], dtype=bool).reshape(n)
    depth = np.zeros(M, dtype=np.uint64)
    per_frame = [0] * 6
    for r, hit in zip(recs, bits):
        if hit:
            depth[r["model_from"] - 1:r["model_to"]] += np.uint64(1)
            per_frame[r["frame"]] += 1
    stats = dict(n_reads=n, n_frames_scored=len(stretch_list), n_cells=sum(s[3] for s in stretch_list) * M, n_unaligned=sum(r["status"] == 1 for r in recs),
                 n_unscored=sum(r["status"] == 2 for r in recs), n_recruited=int(bits.sum()), n_recruited_frame=per_frame)
    return dict(bits=bits, col_depth=depth, stats=stats)


def recruit(hm, reads, min_aa=20, min_score=20 * LN2, scorer=None):
    """yardstick (a) end to end; scorer(seqs) -> [(score, model_from, model_to)] replaces the scoring (yardstick (b) passes the
    device's mgta_seqs_align here)"""
    sl = stretches(reads, min_aa)
    seqs = [s[4] for s in sl]
    scores = scorer(seqs) if scorer else score_all(hm, seqs)
    recs = combine(len(reads), sl, scores)
    out = outputs(recs, sl, hm.M, min_score)
    out.update(recs=recs, stretches=sl, scores=scores)
    return out


STABLE = ("n_reads", "n_frames_scored", "n_cells", "n_unaligned", "n_unscored", "n_recruited", "n_recruited_frame")
