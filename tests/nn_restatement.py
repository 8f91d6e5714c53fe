"""The nn-duplex-v1 thermo score restated in plain Python for the NN tests (test_thermo_nn.py, test_gpu_thermo_nn.py):
internal/thermovisitors/score.go:594-690 and core/thermo/imperfect.go:248-436, :451-493, given the perfect duplex of each
primer as (tm_c, denom).  Independent of the library: ddG and the triplets come from thermo_restatement.py, the sixteen
5'-dangling values are read from the fixture (tests/golden/thermo_nn), and everything is computed from strings the caller
made.  Python floats are IEEE float64 and nothing here fuses a multiply with an add, so the library's results are expected
to equal these bit for bit."""
import csv
import math
import os

import thermo_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thermo_nn")
NAN = float("nan")


def golden_rows(name):
    with open(os.path.join(GOLDEN, name), newline="") as fh:
        return list(csv.DictReader(fh, delimiter="\t"))


def load_dangling():
    """(dangling base, template base of the closing pair) -> dG37 from the 5p rows of dangling_end_goldens.golden"""
    out = {}
    for r in golden_rows("dangling_end_goldens.golden"):
        if r["template_end"] == "5p":
            out[(r["dangling_base"], r["terminal_target_base"])] = float(r["expected_delta_g37_kcal"])
    assert len(out) == 16
    return out


def _at(s, i):
    return s[i] if 0 <= i < len(s) else "N"


def _read(ch):
    """what a site byte reads as once case is folded: A/C/G/T, else N"""
    ch = ch.upper()
    return ch if ch in "ACGT" else "N"


class End:
    """one end: the fields of ipcr_thermo_nn_end"""

    def __init__(self, tm_c=NAN, pen=0.0, adj=0.0, mm=0, n_count=0, status=0):
        self.tm_c, self.pen, self.adj, self.mm, self.n_count, self.status = tm_c, pen, adj, mm, n_count, status

    def key(self):
        import struct
        return (struct.pack("<3d", self.tm_c, self.pen, self.adj), self.mm, self.n_count, self.status)


def end(primer, target, dangling, tm, D, trip, dang):
    """ImperfectDuplexWithOptionsAndContext with the default options and ThreePrimeBase = dangling ("" = none), on the perfect
    duplex (tm, D); case folded, a target byte outside ACGT reads N"""
    P = primer.upper()
    if any(c not in "ACGT" for c in P):
        return End(status=1)
    T = "".join(_read(c) for c in target)
    assert len(P) == len(T) and P and D > 0
    n, pen, mm = len(P), 0.0, 0
    for i in range(n):
        if R.COMP[P[i]] == T[i]:
            continue
        d = R.ddg(_at(P, i - 1), P[i], _at(P, i + 1), _at(T, i - 1), T[i], _at(T, i + 1), trip)
        raw = (d * 1000.0) / D
        mult = R.weight(i, n)
        term = 1.5 if i == n - 1 else 0.5 if i == 0 else 0.0
        w = raw * mult + term
        if w < 0:
            w = 0.0
        pen = pen + w
        mm += 1
    if pen < 0:
        pen = 0.0
    adj = 0.0
    x = _read(dangling) if dangling else "N"
    if x != "N" and R.COMP[P[-1]] == T[-1]:
        adj = adj + (-(dang[(x, T[-1])] * 1000.0) / D)
    return End((tm - pen) + adj, pen, adj, mm, T.count("N"), 0)


def _tile(b: bytes) -> str:
    """a record's bytes as the tiles hold them: an upper-case A/C/G/T, else N (no case folding: a raw lower-case base reads N)"""
    return "".join(chr(c) if chr(c) in "ACGT" else "N" for c in b)


def product(record: bytes, start: int, end_: int, left_primer: str, right_primer: str, base_l, base_r, anneal, trip, dang):
    """scoreNNDuplexComponents over the bytes of the product's record; start > end_: a product across the origin.
    base_l / base_r: (tm_c, denom) of the left / right primer.  -> (score, left End, right End); a product that is not
    scorable gets NaN, the end at fault status 1 (primer not pure ACGT) or 2 (amplicon shorter than the primer)"""
    seq = _tile(record[start:end_] if start <= end_ else record[start:] + record[:end_])
    L = len(seq)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}

    def one(primer, base, left):
        n = len(primer)
        if any(c not in "ACGT" for c in primer):
            return End(status=1)
        if L < n:
            return End(status=2)
        if left:
            target = "".join(comp[c] for c in seq[:n])
            dangling = comp[seq[n]] if L > n else ""
        else:
            target = seq[L - n:][::-1]
            dangling = seq[L - n - 1] if L > n else ""
        return end(primer, target, dangling, base[0], base[1], trip, dang)
    le, re_ = one(left_primer, base_l, True), one(right_primer, base_r, False)
    if le.status or re_.status:
        return NAN, le, re_
    score = le.tm_c - anneal
    if re_.tm_c - anneal < score:
        score = re_.tm_c - anneal
    assert not math.isnan(score)
    return score, le, re_
