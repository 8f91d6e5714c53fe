"""ipcr-thermo, --thermo-model nn-duplex-v1, on the device: ipcr_thermo_nn_duplex_products / _scratch_products.  Every
expected score and every expected end is computed by tests/nn_restatement.py from the records this file made and compared
bit for bit (struct.pack('<d')) -- never from bytes or numbers the library returned; EVERY product a scan reports is compared,
and the planted cases are then looked up among them so that none can go missing unnoticed.  Bit equality is the bar, not a
tolerance: both sides do the same IEEE operations in the same order on the same inputs, with no fused term.

The per-term clamp `w < 0` of the model cannot be reached with the tables as they stand (every ddG is at least 0.60, the N
heuristic at least 0.95), so no case is made up for it."""
import ctypes as C
import math
import random
import struct

import pytest

import nn_restatement as NN
import thermo_restatement as R

pytestmark = pytest.mark.gpu

TRIP = R.load_triplets()
DANG = NN.load_dangling()
COL = 4096
EDGES = (128, 4096, 262144)                                             # strand, column, block (tests/test_gpu_sites.py)
ANNEAL = 60.0


def dbits(x):
    return "nan" if x != x else struct.pack("<d", x)


def end_key(e):
    """an _lib.ThermoNNEnd or an NN.End, comparably"""
    if isinstance(e, NN.End):
        return (dbits(e.tm_c), dbits(e.pen), dbits(e.adj), e.mm, e.n_count, e.status)
    return (dbits(e.tm_c), dbits(e.mismatch_penalty_c), dbits(e.dangling_adjustment_c), e.mismatch_count, e.n_count, e.status)


def rc(s: str) -> str:
    return "".join(R.COMP.get(c, "N") for c in reversed(s))


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(site: str, positions, with_n=()):
    s = list(site)
    for p in positions:
        s[p] = {"A": "C", "C": "A", "G": "T", "T": "G"}[s[p]]
    for p in with_n:
        s[p] = "N"
    return "".join(s)


class Plan:
    """a panel and records with planted products"""

    def __init__(self, seed=7):
        from ipcr_amd import primer
        rng = random.Random(seed)
        self.F, self.Rv = rnd(rng, 20), rnd(rng, 22)                    # main: plain ACGT primers
        half = rnd(rng, 10)
        self.F2, self.Pal = rnd(rng, 20), half + rc(half)               # pal: a reverse primer that is its own reverse complement
        f3 = rnd(rng, 20)
        self.F3, self.Rv3 = f3[:5] + "R" + f3[6:], rnd(rng, 21)         # iupac: the forward primer is not pure ACGT
        self.F4 = rnd(rng, 30)                                          # short: a 17-base product under a 30-base left primer
        self.Rv4 = rc(self.F4[5:17])
        self.F5 = rnd(rng, 30)                                          # exact: a product exactly as long as its left primer,
        self.Rv5 = rc(self.F5[18:30])                                   # the right primer's site is that primer's tail
        self.L1, self.L2 = rnd(rng, 61), rnd(rng, 128)                  # long: primers up to the device limit
        self.K = [(rnd(rng, 19) + b, rnd(rng, 21) + b) for b in "ACGT"]  # k0..k3: both primers end in A, C, G, T
        self.pairs = [primer.Pair("main", self.F, self.Rv), primer.Pair("pal", self.F2, self.Pal),
                      primer.Pair("iupac", self.F3, self.Rv3), primer.Pair("short", self.F4, self.Rv4),
                      primer.Pair("exact", self.F5, self.Rv5), primer.Pair("long", self.L1, self.L2)]
        self.pairs += [primer.Pair("k%d" % i, f, r) for i, (f, r) in enumerate(self.K)]
        self.rng = rng
        self.planted = []                                               # (record, start, end, pair, type, what)

    def amplicon(self, left_site, right_site, fill=60, after_left=None, before_right=None):
        """after_left / before_right: the amplicon's base next to the left / right window (a random one when None)"""
        mid = list(rnd(self.rng, fill))
        if after_left is not None:
            mid[0] = after_left
        if before_right is not None:
            mid[-1] = before_right
        return left_site + "".join(mid) + right_site

    def records(self):
        """r0: 300 000 bases: the mismatch / N / dangling cases, the LEFT window across every edge, the pal, iupac and revcomp
        products; r1: one amplicon that is the whole record (windows at its first and last base); r2: the short, exact and
        long products and the right window across 128; r3: 270 000 bases, the RIGHT window across 4096 and 262144"""
        rng, F, Rv = self.rng, self.F, self.Rv
        recs = [bytearray(rnd(rng, 300_000).encode()), bytearray(), bytearray(rnd(rng, 9000).encode()),
                bytearray(rnd(rng, 270_000).encode())]
        used = [[] for _ in recs]

        def put(rid, pos, amp, pair, typ, what, start=None, end=None):
            assert pos >= 0 and all(pos + len(amp) + 150 <= a or b + 150 <= pos for a, b in used[rid]), (rid, pos, what)
            used[rid].append((pos, pos + len(amp)))
            recs[rid][pos:pos + len(amp)] = amp.encode()
            self.planted.append((rid, pos if start is None else start, pos + len(amp) if end is None else end, pair, typ, what))

        fwd_cases = [((), (), "perfect forward end"), ((0,), (), "5' terminal"), ((1, 2), (), "5' zone, adjacent"), ((3,), (), "first inner"),
                     ((10,), (), "inner"), ((16,), (), "last inner"), ((17,), (), "3' zone"), ((19,), (), "3' terminal next to a dangling base"),
                     ((2, 18), (), "both zones"), ((9,), (8,), "N next to a mismatch"), ((), (0,), "N first"), ((), (19,), "N last"),
                     ((10, 11), (), "adjacent inner")]
        pos = 10_000
        for mm, ns, what in fwd_cases:
            put(0, pos, self.amplicon(mutate(F, mm, ns), rc(Rv)), "main", "forward", what)
            pos += 700
        for mm, ns, what in (((0,), (), "right 5' terminal"), ((21,), (), "right 3' terminal"), ((11,), (10,), "right N next to a mismatch")):
            put(0, pos, self.amplicon(F, rc(mutate(Rv, mm, ns))), "main", "forward", what)   # (positions in the primer's direction)
            pos += 700
        # the sixteen (dangling, paired) keys at the left ends, then at the right ends: the paired base follows from the
        # primer's last base, so four pairs with four neighbours each
        pos = 30_000
        for i, (f, r) in enumerate(self.K):
            for x in "ACGT":
                put(0, pos, self.amplicon(f, rc(r), after_left=x), "k%d" % i, "forward", "left key")
                pos += 700
                put(0, pos, self.amplicon(f, rc(r), before_right=x), "k%d" % i, "forward", "right key")
                pos += 700
        put(0, 60_000, self.amplicon(F, rc(Rv), after_left="N"), "main", "forward", "N as the left dangling base")
        put(0, 60_700, self.amplicon(F, rc(Rv), before_right="N"), "main", "forward", "N as the right dangling base")
        for e in EDGES:
            put(0, e - 7, self.amplicon(mutate(F, (4,)), rc(mutate(Rv, (15,)))), "main", "forward", f"left window across {e}")
        put(0, 150_000, self.amplicon(self.F2, self.Pal), "pal", "forward", "two perfect ends")
        put(0, 151_000, self.amplicon(mutate(self.F3, (2,)), rc(self.Rv3)), "iupac", "forward", "IUPAC forward primer")
        put(0, 152_000, self.amplicon(Rv, rc(mutate(F, (18,)))), "main", "revcomp", "revcomp product")
        put(1, 0, self.amplicon(mutate(F, (0,)), rc(mutate(Rv, (0,)))), "main", "forward", "first and last base of a record")
        a = self.amplicon(mutate(F, (1,)), rc(mutate(Rv, (20,))))
        put(2, 128 + 9 - len(a), a, "main", "forward", "right window across 128")
        put(2, 1000, self.F4, "short", "forward", "shorter than its left primer", 1000, 1017)
        put(2, 2000, self.amplicon(mutate(self.L1, (0, 30, 60)), rc(mutate(self.L2, (1, 64, 126)))), "long", "forward", "long primers")
        put(2, 4000, self.amplicon(self.L2, rc(self.L1)), "long", "revcomp", "long revcomp")
        put(2, 6000, self.F5, "exact", "forward", "exactly as long as its left primer")
        for e in EDGES[1:]:
            a = self.amplicon(mutate(F, (1,)), rc(mutate(Rv, (20,))))
            put(3, e + 9 - len(a), a, "main", "forward", f"right window across {e}")
        return [bytes(r) for r in recs]


def expected(products, recs, base, pairs, anneal=ANNEAL):
    """the restatement's (score, left End, right End) of every product, from the test's own records"""
    idx = {p.ID: i for i, p in enumerate(pairs)}
    out = []
    for p in products:
        k = idx[p.ExperimentID]
        bl, br = (base[2 * k], base[2 * k + 1]) if p.Type == "forward" else (base[2 * k + 1], base[2 * k])
        out.append(NN.product(recs[p.Record], p.Start, p.End, p.FwdPrimer, p.RevPrimer, bl, br, anneal, TRIP, DANG))
    return out


def assert_same(got, want, products, what):
    scores, ends = got
    assert len(scores) == len(ends) == len(want) == len(products)
    bad = []
    for p, s, (le, re_), (ws, wl, wr) in zip(products, scores, ends, want):
        if dbits(s) != dbits(ws) or end_key(le) != end_key(wl) or end_key(re_) != end_key(wr):
            bad.append((what, p.ExperimentID, p.Record, p.Start, p.End, p.Type, s, ws, end_key(le), end_key(wl), end_key(re_), end_key(wr)))
    assert not bad, (len(bad), bad[:2])


def new_genome(recs):
    from ipcr_amd import engine
    cols = sum((len(s) + 128 + 8191) // 8192 * 2 for s in recs)
    return engine.Genome(cols * COL + 4 * 8192, len(recs) + 2)


@pytest.fixture(scope="module")
def scanned():
    from ipcr_amd import engine, thermo
    plan = Plan()
    recs = plan.records()
    eng = engine.New(engine.Config(MaxMM=3, TerminalWindow=0, MinLen=0, MaxLen=400, SeedLen=12))
    cp = eng.CompilePanel(plan.pairs)
    sc = eng.NewSimulationScratch(cp)
    g = new_genome(recs)
    for i, s in enumerate(recs):
        g.add_record("r%d" % i, s)
    base = thermo.panel_nn_base(plan.pairs, thermo.DefaultConditions())
    yield plan, recs, eng, cp, sc, g, base
    g.close()
    sc.close()
    cp.close()


def test_tiny_case_first():
    """one product pair, one launch: the first thing to run on a device"""
    from ipcr_amd import engine, primer, thermo
    eng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, SeedLen=3, MaxLen=2000))
    rec = b"ACGTACAAAAAAGGTACC"
    pairs = [primer.Pair("manual", "AAGTAC", "GGTACC")]
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    g = new_genome([rec])
    g.add_record("s", rec)
    prods = eng.ScanGenome(g, cp, sc)
    base = thermo.panel_nn_base(pairs, thermo.DefaultConditions())
    assert sorted((p.Start, p.End) for p in prods) == [(0, 18), (11, 18)]
    assert_same(sc.thermo_nn_scores(g, base, ANNEAL, details=True), expected(prods, [rec], base, pairs), prods, "tiny")
    assert [dbits(x) for x in sc.thermo_nn_scores(g, base, ANNEAL)] == [dbits(w[0]) for w in expected(prods, [rec], base, pairs)]
    g.close()


def test_planted_products_bit_for_bit(scanned):
    plan, recs, eng, cp, sc, g, base = scanned
    prods = eng.ScanGenome(g, cp, sc)
    found = {(p.Record, p.Start, p.End, p.ExperimentID, p.Type) for p in prods}
    missing = [c for c in plan.planted if c[:5] not in found]
    assert not missing, missing                                         # every planted case is among the products
    odd = [(40.0 + 1.75 * k, 150.0 + 33.25 * k) for k in range(2 * len(plan.pairs))]   # any finite table is taken as given
    for what, b, anneal in (("auto", base, ANNEAL), ("odd", odd, 48.5)):
        assert_same(sc.thermo_nn_scores(g, b, anneal, details=True), expected(prods, recs, b, plan.pairs, anneal), prods, what)
    scores, ends = sc.thermo_nn_scores(g, base, ANNEAL, details=True)
    assert [dbits(x) for x in sc.thermo_nn_scores(g, base, ANNEAL)] == [dbits(x) for x in scores]   # ends = NULL: the same scores
    by = {(p.Record, p.Start, p.End, p.ExperimentID, p.Type): (s, e) for p, s, e in zip(prods, scores, ends)}
    cases = {}
    for c in plan.planted:
        cases.setdefault(c[5], []).append(by[c[:5]])
    bF, bR = base[0], base[1]
    # the perfect product: both ends keep their primer's Tm but for the dangling term
    s, (le, re_) = cases["perfect forward end"][0]
    assert (le.mismatch_count, re_.mismatch_count) == (0, 0) and le.dangling_adjustment_c != 0 and re_.dangling_adjustment_c != 0
    assert dbits(le.tm_c) == dbits((bF[0] - 0.0) + le.dangling_adjustment_c) and dbits(s) == dbits(min(le.tm_c, re_.tm_c) - ANNEAL)
    # a terminal mismatch next to a dangling base gives no term; N as the dangling base gives none either
    s, (le, re_) = cases["3' terminal next to a dangling base"][0]
    assert le.mismatch_count == 1 and le.dangling_adjustment_c == 0.0 and re_.dangling_adjustment_c != 0.0
    assert cases["N as the left dangling base"][0][1][0].dangling_adjustment_c == 0.0
    assert cases["N as the left dangling base"][0][1][0].n_count == 0 and cases["N as the left dangling base"][0][1][1].dangling_adjustment_c != 0.0
    assert cases["N as the right dangling base"][0][1][1].dangling_adjustment_c == 0.0
    assert cases["N next to a mismatch"][0][1][0].n_count == 1 and cases["N next to a mismatch"][0][1][0].mismatch_count == 2
    assert cases["right N next to a mismatch"][0][1][1].n_count == 1
    # the terminal terms: 0.5 at the primer's first base, 1.5 at its last, on top of raw * mult
    assert cases["5' terminal"][0][1][0].mismatch_penalty_c > 0.5 and cases["right 3' terminal"][0][1][1].mismatch_penalty_c > 1.5
    assert cases["5' zone, adjacent"][0][1][0].mismatch_count == 2 and cases["adjacent inner"][0][1][0].mismatch_count == 2
    # the sixteen keys, at both ends: each product's term is the table value of its key
    for side, what in ((0, "left key"), (1, "right key")):
        keys = set()
        for c in plan.planted:
            if c[5] != what:
                continue
            e = by[c[:5]][1][side]
            rec, a, b = recs[c[0]], c[1], c[2]
            k = [q.ID for q in plan.pairs].index(c[3])
            if side == 0:
                x, paired = R.COMP[chr(rec[a + 20])], R.COMP[chr(rec[a + 19])]
            else:
                x, paired = chr(rec[b - 23]), chr(rec[b - 22])
            D = base[2 * k + side][1]
            assert e.status == 0 and e.mismatch_count == 0
            assert dbits(e.dangling_adjustment_c) == dbits(0.0 + (-(DANG[(x, paired)] * 1000.0) / D)), (what, x, paired)
            keys.add((x, paired))
        assert keys == set(DANG), (what, sorted(set(DANG) - keys))
    # not scorable: NaN and a status, the call itself succeeds
    s, (le, re_) = cases["shorter than its left primer"][0]
    assert math.isnan(s) and (le.status, re_.status) == (2, 0) and math.isnan(le.tm_c) and not math.isnan(re_.tm_c)
    s, (le, re_) = cases["IUPAC forward primer"][0]
    assert math.isnan(s) and (le.status, re_.status) == (1, 0) and re_.mismatch_count == 0
    # exactly as long as its left primer: no left dangling base; the right one lies inside the left window
    s, (le, re_) = cases["exactly as long as its left primer"][0]
    assert not math.isnan(s) and (le.status, re_.status) == (0, 0) and le.dangling_adjustment_c == 0.0 and re_.dangling_adjustment_c != 0.0
    # the whole record: both windows at its ends, both dangling bases inside
    s, (le, re_) = cases["first and last base of a record"][0]
    assert (le.mismatch_count, re_.mismatch_count) == (1, 1) and not math.isnan(s)
    s, (le, re_) = cases["long primers"][0]
    assert (le.mismatch_count, re_.mismatch_count) == (3, 3)
    s, (le, re_) = cases["two perfect ends"][0]
    assert (le.mismatch_count, re_.mismatch_count) == (0, 0)            # (the self-complementary primer: its base has X = 1)
    assert len({dbits(x) for x in scores}) > 30                         # the cases do score differently
    assert any(p.Type == "revcomp" for p in prods)


def test_piece_boundary(scanned, monkeypatch):
    plan, recs, eng, cp, sc, g, base = scanned
    prods = eng.ScanGenome(g, cp, sc)
    whole = sc.thermo_nn_scores(g, base, ANNEAL, details=True)

    def keyed(r):
        return [dbits(x) for x in r[0]], [(end_key(a), end_key(b)) for a, b in r[1]]
    piece = next(k for k in (7, 6, 5) if len(prods) % k)              # several launches, the last one short
    monkeypatch.setenv("IPCR_TEST_THERMO_PIECE", str(piece))
    assert len(prods) > 21
    assert keyed(sc.thermo_nn_scores(g, base, ANNEAL, details=True)) == keyed(whole)
    monkeypatch.setenv("IPCR_TEST_THERMO_PIECE", "1")
    assert [dbits(x) for x in sc.thermo_nn_scores(g, base, ANNEAL)] == keyed(whole)[0]


def test_chunked_and_streamed_scans_score_the_same(scanned):
    plan, recs, eng, cp, sc, g, base = scanned
    prods = eng.ScanGenomeChunked(g, cp, sc, 5000, 400)                 # window-local products: the library puts them back
    wins = sc.chunk_windows()
    assert len(prods) > 40
    want = []
    for p in prods:
        w = wins[p.Record]
        q = type(p)(**{**p.__dict__, "Record": w.record, "Start": p.Start + w.start, "End": p.End + w.start})
        want.append(expected([q], recs, base, plan.pairs)[0])
    assert_same(sc.thermo_nn_scores(g, base, ANNEAL, details=True), want, prods, "chunked")
    # streamed: chunks through ipcr_scan_chunk, scored from the chunk's own tiles -- the two short records whole, and the
    # stretches of the long one that hold the mismatch, key and N cases
    total = 0
    spans = [(1, lo) for lo in range(0, 1, 4600)] + [(2, lo) for lo in range(0, 9000 - 400, 4600)]
    spans += [(0, lo) for lo in range(9_200, 23_000, 4600)] + [(0, 29_500), (0, 34_100), (0, 58_000), (0, 149_500)]
    for r, lo in spans:
        chunk = recs[r][lo:lo + 5000]
        ps = eng.SimulateCompiledWithScratch("c", chunk, cp, sc)
        assert_same(sc.thermo_nn_scores(None, base, ANNEAL, details=True), expected(ps, [chunk], base, plan.pairs), ps, "streamed")
        total += len(ps)
    assert total > 40
    empty = eng.SimulateCompiledWithScratch("c", b"ACGTACGTAAAAAAAAAAAAAACCCCCCCCCCCCCGT", cp, sc)
    assert empty == [] and sc.thermo_nn_scores(None, base, ANNEAL) == []


def test_circular_products_across_the_origin():
    """the amplicon's base next to a window lies on the other side of the origin: the left window ends at the record's last
    base (its dangling base is the record's first), then the right window begins at the record's first base (its dangling
    base is the record's last).  Both last columns are Watson-Crick pairs, so a term must come out: a kernel that looked
    for the neighbour by arithmetic would read the padding behind the record, or the base before it."""
    from ipcr_amd import engine, primer, thermo
    rng = random.Random(11)
    F, Rv = rnd(rng, 20), rnd(rng, 22)
    pairs = [primer.Pair("c", F, Rv)]
    base = thermo.panel_nn_base(pairs, thermo.DefaultConditions())
    eng = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=0, MaxLen=400, SeedLen=12, Circular=True))
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    amp = mutate(F, (1,)) + rnd(rng, 80) + rc(mutate(Rv, (2,)))
    for cut, side in ((len(F), 0), (len(amp) - len(Rv), 1)):
        rec = (amp[cut:] + rnd(rng, 3000) + amp[:cut]).encode()
        g = new_genome([rec])
        g.add_record("r", rec)
        prods = eng.ScanGenome(g, cp, sc)
        wrap = [i for i, p in enumerate(prods) if p.Start > p.End]
        assert wrap and (prods[wrap[0]].Start, prods[wrap[0]].End) == (len(rec) - cut, len(amp) - cut)
        got = sc.thermo_nn_scores(g, base, ANNEAL, details=True)
        assert_same(got, expected(prods, [rec], base, pairs), prods, "circular %d" % side)
        e = got[1][wrap[0]][side]
        x, paired = (R.COMP[chr(rec[0])], R.COMP[F[-1]]) if side == 0 else (chr(rec[-1]), R.COMP[Rv[-1]])
        assert e.status == 0 and dbits(e.dangling_adjustment_c) == dbits(0.0 + (-(DANG[(x, paired)] * 1000.0) / base[side][1]))
        # and from the chunk's own tiles
        ps = eng.SimulateCompiledWithScratch("r", rec, cp, sc)
        assert any(p.Start > p.End for p in ps)
        assert_same(sc.thermo_nn_scores(None, base, ANNEAL, details=True), expected(ps, [rec], base, pairs), ps, "circular chunk %d" % side)
        g.close()
    sc.close()
    cp.close()


def test_argument_errors_come_from_the_host_check(scanned):
    from ipcr_amd import _lib
    plan, recs, eng, cp, sc, g, base = scanned
    L = _lib.lib()
    prods = eng.ScanGenome(g, cp, sc)
    n, nb = len(prods), len(base)
    out = (C.c_double * (n + 1))()
    ends = (_lib.ThermoNNEnd * (2 * n + 2))()

    def table(entries):
        return (_lib.ThermoNNPrimer * len(entries))(*(_lib.ThermoNNPrimer(t, d) for t, d in entries))
    b = table(base)

    def status(*a):
        return L.ipcr_thermo_nn_duplex_products(*a)
    assert status(sc._h, g._h, b, nb, ANNEAL, out, ends, n) == _lib.OK
    assert status(sc._h, g._h, b, nb, ANNEAL, out, None, n) == _lib.OK
    assert status(sc._h, g._h, b, nb, ANNEAL, out, ends, n + 1) == _lib.ERR_INVALID
    assert status(sc._h, g._h, b, nb, ANNEAL, out, ends, n - 1) == _lib.ERR_INVALID
    assert status(sc._h, g._h, b, nb - 1, ANNEAL, out, ends, n) == _lib.ERR_INVALID    # not twice the pair count
    assert status(sc._h, g._h, b, 0, ANNEAL, out, ends, n) == _lib.ERR_INVALID
    assert status(sc._h, g._h, None, nb, ANNEAL, out, ends, n) == _lib.ERR_INVALID     # a count without a table
    zero = table(base[:5] + [(base[5][0], 0.0)] + base[6:])
    assert status(sc._h, g._h, zero, nb, ANNEAL, out, ends, n) == _lib.ERR_INVALID     # denom = 0
    assert "base entry 5" in L.ipcr_last_error().decode()
    assert status(sc._h, g._h, b, nb, math.nan, out, ends, n) == _lib.ERR_INVALID
    assert status(None, g._h, b, nb, ANNEAL, out, ends, n) == _lib.ERR_INVALID
    assert status(sc._h, None, b, nb, ANNEAL, out, ends, n) == _lib.ERR_INVALID
    assert status(sc._h, g._h, b, nb, ANNEAL, None, ends, n) == _lib.ERR_INVALID
    assert L.ipcr_thermo_nn_duplex_scratch_products(sc._h, b, nb, ANNEAL, out, ends, n) == _lib.ERR_INVALID   # the last scan was no chunk scan
    # another genome: records the products do not fit are refused before anything is launched
    small = new_genome([recs[1]])
    small.add_record("x", recs[1])                                     # (one short record)
    assert status(sc._h, small._h, b, nb, ANNEAL, out, ends, n) == _lib.ERR_INVALID
    assert "record" in L.ipcr_last_error().decode()
    small.close()
    ps = eng.SimulateCompiledWithScratch("c", recs[1], cp, sc)
    assert ps
    assert status(sc._h, g._h, b, nb, ANNEAL, out, ends, len(ps)) == _lib.ERR_INVALID  # ... a chunk scan: the scratch form scores it
    assert L.ipcr_thermo_nn_duplex_scratch_products(sc._h, b, nb, ANNEAL, out, ends, len(ps) + 1) == _lib.ERR_INVALID
    assert L.ipcr_thermo_nn_duplex_scratch_products(sc._h, zero, nb, ANNEAL, out, ends, len(ps)) == _lib.ERR_INVALID
    assert L.ipcr_thermo_nn_duplex_scratch_products(sc._h, b, nb, ANNEAL, out, ends, len(ps)) == _lib.OK
