"""The legacy-heuristic thermo score restated in plain Python for the thermo tests (test_thermo_legacy.py,
test_gpu_thermo.py): internal/thermovisitors/score.go:1522-1552, :363-458, :282-297 and core/thermo/mismatch.go:108-189.
Independent of the library: the triplet values are read from the fixture (tests/golden/thermo), the pair-family values and
the N heuristic are written out here, and everything is computed from strings the caller made."""
import csv
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thermo")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
INF = 1e9
PEN_GAP_1NT = 6.0

# curated pair-family ddG (kcal/mol) by (primer base, target base): wobble, transitions, transversions, like with like
PAIR = {}
for _keys, _v in ((("GT", "TG"), 0.60), (("AG", "GA", "CT", "TC"), 0.85), (("AC", "CA"), 1.10),
                  (("AT", "TA", "CG", "GC"), 1.20), (("AA", "CC", "GG", "TT"), 1.40)):
    for _k in _keys:
        PAIR[(_k[0], _k[1])] = _v


def golden_rows(name):
    with open(os.path.join(GOLDEN, name), newline="") as fh:
        return list(csv.DictReader(fh, delimiter="\t"))


def load_triplets():
    """(p5, p, p3, t5, t, t3) -> ddG from mismatch_triplet_goldens.golden: each row is a 7-mer duplex with one mismatch at
    index 3, so primer[2:5] / target[2:5] is the context"""
    out = {}
    for r in golden_rows("mismatch_triplet_goldens.golden"):
        p, t = r["primer"], r["target"]
        out[(p[2], p[3], p[4], t[2], t[3], t[4])] = float(r["expected_delta_delta_g_kcal"])
    return out


def _flank(b):
    return b if b in "ACGT" else "N"


def ddg(p5, p, p3, t5, t, t3, trip):
    """LookupDeltaG: None where the reference returns ok == false"""
    if p not in "ACGT" or len(p) != 1 or t not in "ACGTN" or len(t) != 1:
        return None
    k = (_flank(p5), p, _flank(p3), _flank(t5), t, _flank(t3))
    if k in trip:                                                       # the exact triplet (the wildcard keys hold nothing)
        return trip[k]
    if (p, t) in PAIR:                                                  # the curated pair family
        return PAIR[(p, t)]
    base = 1.0                                                          # t == 'N': the heuristic's conservative default
    flanks = (p5, p3, t5, t3)
    gc = sum(b in "GC" for b in flanks)
    at = sum(b in "AT" for b in flanks)
    if gc >= at + 2:
        base -= 0.05
    return max(base, -0.10)


def weight(i, n):
    if i >= n - 3:
        return 2.0
    if i < 3:
        return 1.5
    return 1.0


def _at(s, i):
    return s[i] if 0 <= i < len(s) else "N"


def single_mm(P, T, i, j, D, trip):
    d = ddg(_at(P, i - 1), P[i], _at(P, i + 1), _at(T, j - 1), T[j], _at(T, j + 1), trip)
    if d is None:
        pen = 4.0
    else:
        pen = (d * 1000.0) / D if D > 0 else 4.0
    return pen * weight(i, len(P))


def _norm(primer, target):
    P, T = primer.upper(), target.upper()
    if any(c not in "ACGT" for c in P):
        P = ""
    if any(c not in "ACGTN" for c in T):
        T = ""
    return P, T


def closed_form(primer, target, D, trip):
    """the plain sum of the issue, for |primer| == |target|"""
    P, T = _norm(primer, target)
    if not P or not T:
        return 0.0
    assert len(P) == len(T)
    s = 0.0
    for i in range(len(P)):
        if COMP[P[i]] != T[i]:
            s = s + single_mm(P, T, i, i, D, trip)
    return 0.0 if s < 0 else s


def gap_dp(primer, target, D, allow_gap, trip):
    """alignPenaltyC_contextualD_ss, literally (single-stranded mode off)"""
    P, T = _norm(primer, target)
    n, m = len(P), len(T)
    if n == 0 or m == 0:
        return 0.0
    gaps = 1 if allow_gap else 0
    dp = [[[INF, INF] for _ in range(m + 1)] for _ in range(n + 1)]
    dp[0][0][0] = 0.0
    for i in range(n + 1):
        for j in range(m + 1):
            for g in range(gaps + 1):
                cur = dp[i][j][g]
                if cur >= INF / 2:
                    continue
                if i < n and j < m:
                    pen = 0.0
                    if COMP[P[i]] != T[j]:
                        pen = single_mm(P, T, i, j, D, trip)
                    if cur + pen < dp[i + 1][j + 1][g]:
                        dp[i + 1][j + 1][g] = cur + pen
                if g == 0 and i < n:
                    val = cur + PEN_GAP_1NT * weight(i, n)
                    if val < dp[i + 1][j][1]:
                        dp[i + 1][j][1] = val
                if g == 0 and j < m:
                    val = cur + PEN_GAP_1NT * weight(i, n)
                    if val < dp[i][j + 1][1]:
                        dp[i][j + 1][1] = val
    best = min(dp[n][m][0], dp[n][m][1])
    if best >= INF / 2:
        return 0.0
    return 0.0 if best < 0 else best


def comp_window(b: bytes) -> str:
    """comp5to3: base by base, not reversed; everything but upper-case ACGT becomes N"""
    return "".join(COMP.get(chr(c), "N") for c in b)


def product_score(record: bytes, start: int, end: int, fwd_primer: str, rev_primer: str, denom_f, denom_r, trip):
    """visitLegacyHeuristic over the bytes of the product's record; start > end: a product across the origin"""
    seq = record[start:end] if start <= end else record[start:] + record[:end]
    pen = 0.0
    f, _ = _norm(fwd_primer, "")
    if f and len(seq) >= len(f):
        pen += closed_form(f, comp_window(seq[:len(f)]), denom_f, trip)
    r, _ = _norm(rev_primer, "")
    if r and len(seq) >= len(r):
        pen += closed_form(r, comp_window(seq[len(seq) - len(r):]), denom_r, trip)
    return -pen
