"""ipcr-thermo, --thermo-model legacy-heuristic, on the device: ipcr_thermo_legacy_products / _scratch_products and
`python -m ipcr_amd.thermo_cli`.  Every expected score is computed by tests/thermo_restatement.py from the records this
file made and compared bit for bit (struct.pack('<d')) -- never from bytes or numbers the library returned; EVERY product a
scan reports is compared, and the planted cases are then looked up among them so that none can go missing unnoticed."""
import ctypes as C
import io
import json
import os
import random
import struct

import pytest

import thermo_restatement as R

pytestmark = pytest.mark.gpu

TRIP = R.load_triplets()
CLI = json.load(open(os.path.join(R.GOLDEN, "legacy_cli.json")))
LIT = json.load(open(os.path.join(R.GOLDEN, "literals.json")))
COL = 4096
EDGES = (128, 4096, 262144)                                             # strand, column, block (tests/test_gpu_sites.py)


def bits(x):
    return struct.pack("<d", x)


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

    def __init__(self, seed=5):
        from ipcr_amd import primer
        rng = random.Random(seed)
        self.F, self.Rv = rnd(rng, 20), rnd(rng, 22)                    # main: plain ACGT primers
        half = rnd(rng, 10)
        self.F2, self.Pal = rnd(rng, 20), half + rc(half)               # pal: a reverse primer that is its own reverse complement
        f3 = rnd(rng, 20)
        self.F3, self.Rv3 = f3[:5] + "R" + f3[6:], rnd(rng, 21)         # iupac: the forward primer's end adds nothing
        self.F4 = rnd(rng, 30)                                          # short: the right primer's site lies inside the left
        self.Rv4 = rc(self.F4[5:17])                                    # one's: a 17-base product under a 30-base left primer
        self.L1, self.L2 = rnd(rng, 61), rnd(rng, 128)                  # long: primers up to the device limit
        self.pairs = [primer.Pair("main", self.F, self.Rv), primer.Pair("pal", self.F2, self.Pal),
                      primer.Pair("iupac", self.F3, self.Rv3), primer.Pair("short", self.F4, self.Rv4),
                      primer.Pair("long", self.L1, self.L2)]
        self.rng = rng
        self.planted = []                                               # (record, start, end, pair, type, what)

    def amplicon(self, left_site, right_site, fill=60):
        return left_site + rnd(self.rng, fill) + right_site

    def records(self):
        """r0: 300 000 bases: the mismatch / N cases, the LEFT window across every edge, the pal, iupac and revcomp
        products; r1: one amplicon that is the whole record (windows at its first and last base); r2: the short and the
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

        fwd_cases = [((), (), "perfect forward end"), ((0,), (), "5' zone"), ((1, 2), (), "5' zone x2"), ((3,), (), "first inner"),
                     ((10,), (), "inner"), ((16,), (), "last inner"), ((17,), (), "3' zone"), ((19,), (), "last base"),
                     ((2, 18), (), "both zones"), ((9,), (8,), "N next to a mismatch"), ((), (0,), "N first"), ((), (19,), "N last"),
                     ((5, 6, 7), (), "run")]
        pos = 10_000
        for mm, ns, what in fwd_cases:
            put(0, pos, self.amplicon(mutate(F, mm, ns), rc(Rv)), "main", "forward", what)
            pos += 700
        for mm, ns, what in (((0,), (), "right 5'"), ((21,), (), "right 3'"), ((11,), (10,), "right N next to a mismatch")):
            put(0, pos, self.amplicon(F, rc(mutate(Rv, mm, ns))), "main", "forward", what)   # (positions in the primer's direction)
            pos += 700
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
        for e in EDGES[1:]:
            a = self.amplicon(mutate(F, (1,)), rc(mutate(Rv, (20,))))
            put(3, e + 9 - len(a), a, "main", "forward", f"right window across {e}")
        return [bytes(r) for r in recs]


def expected(products, recs, denoms, pairs):
    """the restatement's score of every product, from the test's own records"""
    idx = {p.ID: i for i, p in enumerate(pairs)}
    out = []
    for p in products:
        k = idx[p.ExperimentID]
        fwd = p.Type == "forward"
        d = denoms or [200.0] * (2 * len(pairs))
        df, dr = (d[2 * k], d[2 * k + 1]) if fwd else (d[2 * k + 1], d[2 * k])
        out.append(R.product_score(recs[p.Record], p.Start, p.End, p.FwdPrimer, p.RevPrimer, df, dr, TRIP))
    return out


def assert_same(got, want, products, what):
    assert len(got) == len(want) == len(products)
    bad = [(what, p.ExperimentID, p.Record, p.Start, p.End, p.Type, g, w) for p, g, w in zip(products, got, want) if bits(g) != bits(w)]
    assert not bad, (len(bad), bad[:3])


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
    yield plan, recs, eng, cp, sc, g, thermo
    g.close()
    sc.close()
    cp.close()


def test_tiny_case_first():
    """one product, one launch: the first thing to run on a device"""
    from ipcr_amd import engine, primer
    eng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, SeedLen=3, MaxLen=2000))
    rec = b"ACGTACAAAAAAGGTACC"
    cp = eng.CompilePanel([primer.Pair("manual", "AAGTAC", "GGTACC")])
    sc = eng.NewSimulationScratch(cp)
    g = new_genome([rec])
    g.add_record("s", rec)
    prods = eng.ScanGenome(g, cp, sc)
    got = sc.thermo_scores(g)
    assert sorted((p.Start, p.End, s) for p, s in zip(prods, got)) == [(0, 18, -18.975), (11, 18, -29.625)]
    g.close()


def test_planted_products_bit_for_bit(scanned):
    plan, recs, eng, cp, sc, g, thermo = scanned
    prods = eng.ScanGenome(g, cp, sc)
    found = {(p.Record, p.Start, p.End, p.ExperimentID, p.Type) for p in prods}
    missing = [c for c in plan.planted if c[:5] not in found]
    assert not missing, missing                                         # every planted case is among the products
    auto = thermo.panel_denoms(plan.pairs, thermo.DefaultConditions())
    odd = [200.0, 0.0, -3.0, 1e-3, 150.0, 150.0, 333.25, 1e9, 97.0, 12.5]      # D <= 0: every mismatch costs 4.0
    for what, den in (("fixed", None), ("auto", auto), ("odd", odd)):
        got = sc.thermo_scores(g, den)
        assert_same(got, expected(prods, recs, den, plan.pairs), prods, what)
    got = sc.thermo_scores(g)
    by = {(p.Record, p.Start, p.End, p.ExperimentID, p.Type): s for p, s in zip(prods, got)}
    name = {c[:5]: c[5] for c in plan.planted}
    two_perfect = [k for k in name if name[k] == "two perfect ends"][0]
    assert bits(by[two_perfect]) == bits(-0.0)
    short = [k for k in name if name[k] == "shorter than its left primer"][0]
    assert short[2] - short[1] == 17 < len(plan.F4)                      # the left end is skipped, the right one scored
    assert bits(by[short]) == bits(-(0.0 + R.closed_form(plan.Rv4, R.comp_window(plan.F4[5:17].encode()), 200.0, TRIP))) != bits(-0.0)
    assert len({bits(s) for s in got}) > 15                             # the cases do score differently
    assert any(p.Type == "revcomp" for p in prods)


def test_iupac_reverse_end_still_counts(scanned):
    """the IUPAC pair's reverse primer is plain ACGT: its end is scored although the forward end is not"""
    plan, recs, eng, cp, sc, g, thermo = scanned
    prods = eng.ScanGenome(g, cp, sc)
    got = sc.thermo_scores(g)
    iu = [(p, s) for p, s in zip(prods, got) if p.ExperimentID == "iupac" and p.Type == "forward"]
    assert iu
    for p, s in iu:
        w = R.comp_window(recs[p.Record][p.End - len(plan.Rv3):p.End])
        assert bits(s) == bits(-(0.0 + R.closed_form(plan.Rv3, w, 200.0, TRIP)))


def test_piece_boundary(scanned, monkeypatch):
    plan, recs, eng, cp, sc, g, thermo = scanned
    prods = eng.ScanGenome(g, cp, sc)
    whole = sc.thermo_scores(g)
    monkeypatch.setenv("IPCR_TEST_THERMO_PIECE", "7")
    assert len(prods) > 21 and len(prods) % 7 != 0
    assert [bits(x) for x in sc.thermo_scores(g)] == [bits(x) for x in whole]
    monkeypatch.setenv("IPCR_TEST_THERMO_PIECE", "1")
    assert [bits(x) for x in sc.thermo_scores(g)] == [bits(x) for x in whole]


def test_chunked_and_streamed_scans_score_the_same(scanned):
    plan, recs, eng, cp, sc, g, thermo = scanned
    auto = thermo.panel_denoms(plan.pairs, thermo.DefaultConditions())
    prods = eng.ScanGenomeChunked(g, cp, sc, 5000, 400)                 # window-local products: the library puts them back
    wins = sc.chunk_windows()
    assert len(prods) > 20
    want = []
    for p in prods:
        w = wins[p.Record]
        q = type(p)(**{**p.__dict__, "Record": w.record, "Start": p.Start + w.start, "End": p.End + w.start})
        want.append(expected([q], recs, auto, plan.pairs)[0])
    assert_same(sc.thermo_scores(g, auto), want, prods, "chunked")
    # streamed: every chunk through ipcr_scan_chunk, scored from the chunk's own tiles
    total = 0
    for r, rec in enumerate(recs):
        for lo in range(0, max(len(rec) - 400, 1), 4600):
            chunk = rec[lo:lo + 5000]
            ps = eng.SimulateCompiledWithScratch("c", chunk, cp, sc)
            got = sc.thermo_scores(None, auto)
            assert_same(got, expected(ps, [chunk], auto, plan.pairs), ps, "streamed")
            total += len(ps)
    assert total > 20
    empty = eng.SimulateCompiledWithScratch("c", b"ACGTACGTAAAAAAAAAAAAAACCCCCCCCCCCCCGT", cp, sc)
    assert empty == [] and sc.thermo_scores(None) == []


def test_circular_product_across_the_origin():
    from ipcr_amd import engine, primer
    rng = random.Random(9)
    F, Rv = rnd(rng, 20), rnd(rng, 22)
    body = rnd(rng, 3000)
    # the amplicon F' ... rc(Rv') is cut inside its filler: its tail opens the record, its head closes it
    amp = mutate(F, (1, 18)) + rnd(rng, 80) + rc(mutate(Rv, (2,)))
    rec = (amp[60:] + body + amp[:60]).encode()
    eng = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=0, MaxLen=400, SeedLen=12, Circular=True))
    pairs = [primer.Pair("c", F, Rv)]
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    g = new_genome([rec])
    g.add_record("r", rec)
    prods = eng.ScanGenome(g, cp, sc)
    wrap = [p for p in prods if p.Start > p.End]
    assert wrap and (wrap[0].Start, wrap[0].End) == (len(rec) - 60, len(amp) - 60)
    assert_same(sc.thermo_scores(g), expected(prods, [rec], None, pairs), prods, "circular")
    assert all(s < 0 for p, s in zip(prods, sc.thermo_scores(g)) if p.Start > p.End)
    # and from the chunk's own tiles
    ps = eng.SimulateCompiledWithScratch("r", rec, cp, sc)
    assert any(p.Start > p.End for p in ps)
    assert_same(sc.thermo_scores(None), expected(ps, [rec], None, pairs), ps, "circular chunk")
    g.close()


def test_raw_lower_case_reads_as_n():
    """a record given raw with lower-case bases: the reference's compBase makes N of them (score.go:307-320), and so does
    the inv plane the kernel reads"""
    from ipcr_amd import engine, primer
    rng = random.Random(4)
    F, Rv = rnd(rng, 20), rnd(rng, 22)
    left = F[:6] + F[6].lower() + F[7:]
    rec = (rnd(rng, 300) + left + rnd(rng, 50) + rc(Rv) + rnd(rng, 300)).encode()
    eng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, MaxLen=400, SeedLen=12))
    pairs = [primer.Pair("lc", F, Rv)]
    cp = eng.CompilePanel(pairs)
    sc = eng.NewSimulationScratch(cp)
    g = new_genome([rec])
    g.add_record("r", rec)
    prods = eng.ScanGenome(g, cp, sc)
    assert [(p.Start, p.FwdMismatchIdx) for p in prods] == [(300, (6,))]
    got = sc.thermo_scores(g)
    assert_same(got, expected(prods, [rec], None, pairs), prods, "lower case")
    w = R.comp_window(rec[300:320])
    assert w[6] == "N" and got[0] < -R.closed_form(Rv, R.comp_window(rec[370:392]), 200.0, TRIP)
    g.close()


def test_argument_errors_come_from_the_host_check(scanned):
    from ipcr_amd import _lib
    plan, recs, eng, cp, sc, g, thermo = scanned
    L = _lib.lib()
    prods = eng.ScanGenome(g, cp, sc)
    n = len(prods)
    out = (C.c_double * (n + 1))()
    den = (C.c_double * 10)(*([200.0] * 10))

    def status(*a):
        return L.ipcr_thermo_legacy_products(*a)
    assert status(sc._h, g._h, None, 0, out, n) == _lib.OK
    assert status(sc._h, g._h, None, 0, out, n + 1) == _lib.ERR_INVALID
    assert status(sc._h, g._h, None, 0, out, n - 1) == _lib.ERR_INVALID
    assert status(sc._h, g._h, den, 9, out, n) == _lib.ERR_INVALID      # not twice the pair count
    assert status(sc._h, g._h, None, 10, out, n) == _lib.ERR_INVALID    # a count without a table
    assert status(sc._h, g._h, den, 10, out, n) == _lib.OK
    assert status(None, g._h, None, 0, out, n) == _lib.ERR_INVALID
    assert status(sc._h, None, None, 0, out, n) == _lib.ERR_INVALID
    assert status(sc._h, g._h, None, 0, None, n) == _lib.ERR_INVALID
    assert L.ipcr_thermo_legacy_scratch_products(sc._h, None, 0, out, n) == _lib.ERR_INVALID   # the last scan was no chunk scan
    # another genome: records the products do not fit are refused before anything is launched
    small = new_genome([recs[1]])
    small.add_record("x", recs[1])                                     # (one short record)
    assert status(sc._h, small._h, None, 0, out, n) == _lib.ERR_INVALID
    assert "record" in L.ipcr_last_error().decode()
    small.close()
    ps = eng.SimulateCompiledWithScratch("c", recs[1], cp, sc)
    assert ps
    assert status(sc._h, g._h, None, 0, out, len(ps)) == _lib.ERR_INVALID   # ... a chunk scan: the scratch form scores it
    assert L.ipcr_thermo_legacy_scratch_products(sc._h, None, 0, out, len(ps) + 1) == _lib.ERR_INVALID
    assert L.ipcr_thermo_legacy_scratch_products(sc._h, None, 0, out, len(ps)) == _lib.OK


def test_every_product_consumer_translates_and_refuses_alike():
    """The probe rescan, the nested scan, the site read and the thermo score of a chunked scan's window-local products equal
    those of the whole-record scan, product for product in record coordinates; against a genome whose records end before
    the products do, all four refuse with IPCR_ERR_INVALID (a probe `end` after the refused `begin` too), and the same
    scratch then serves the right genome."""
    from ipcr_amd import _lib, engine, nested, primer
    rng = random.Random(21)
    F, Rv, IF, IR, probe = rnd(rng, 20), rnd(rng, 22), rnd(rng, 18), rnd(rng, 18), rnd(rng, 16)

    def amp(mm_f, mm_r, with_probe):                                    # outer sites, the inner pair inside, the probe between
        return (mutate(F, mm_f) + rnd(rng, 15) + IF + rnd(rng, 20) + (probe if with_probe else rnd(rng, 16)) + rnd(rng, 30)
                + rc(IR) + rnd(rng, 15) + rc(mutate(Rv, mm_r)))
    recs = [bytearray(rnd(rng, 6200).encode()), bytearray(rnd(rng, 6100).encode())]
    # windows of 4000 every 3000: [0, 4000) and [3000, end).  500: the first window only (and inside a 2 kb record);
    # 3300: both windows; 5200 and record 1's 4500: the second window only, whose start is not 0
    plan = [(0, 500, (), (), True), (0, 3300, (1,), (), True), (0, 5200, (), (20,), False), (1, 4500, (3, 17), (2,), True)]
    for r, pos, mm_f, mm_r, with_probe in plan:
        a = amp(mm_f, mm_r, with_probe).encode()
        recs[r][pos:pos + len(a)] = a
    recs = [bytes(r) for r in recs]
    oeng = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=0, MaxLen=400, SeedLen=12))
    ieng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, SeedLen=12))
    cpo, cpi = oeng.CompilePanel([primer.Pair("outer", F, Rv)]), ieng.CompilePanel([primer.Pair("inner", IF, IR)])
    sco, scc, sci = oeng.NewSimulationScratch(cpo), oeng.NewSimulationScratch(cpo), ieng.NewSimulationScratch(cpi)
    g, small = new_genome(recs), new_genome([r[:2000] for r in recs])
    for i, s in enumerate(recs):
        g.add_record("r%d" % i, s)
        small.add_record("s%d" % i, s[:2000])

    def consumers(sc, prods):
        """per product: (probe hit, inner product, sites, score bits)"""
        hits = [(h.found, h.strand, h.pos, h.mm) for h in sc.probe_products(probe, 1, g)]
        inner = [(n.InnerFound, n.InnerPairID, n.InnerStart, n.InnerEnd, n.InnerLength, n.InnerType, n.InnerFwdMM, n.InnerRevMM)
                 for n in nested.NestedProducts(sc, prods, g, cpi, sci)]
        return list(zip(hits, inner, sc.product_sites(g), [bits(x) for x in sc.thermo_scores(g)]))

    whole = oeng.ScanGenome(g, cpo, sco)
    assert sorted((p.Record, p.Start) for p in whole) == sorted(c[:2] for c in plan)
    want = {(p.Record, p.Start, p.End, p.Type): c for p, c in zip(whole, consumers(sco, whole))}
    assert sum(c[0][0] for c in want.values()) == 3 and all(c[1][0] for c in want.values())   # the probe and the inner pair are found
    assert len({c[3] for c in want.values()}) == len(plan)             # ... and the products score differently
    for (r, a, b, _), c in want.items():
        assert c[2] == (recs[r][a:a + len(F)].decode(), rc(recs[r][b - len(Rv):b].decode()))
    chunked = oeng.ScanGenomeChunked(g, cpo, scc, 4000, 1000)
    wins = scc.chunk_windows()
    assert len(chunked) == len(whole) + 1 and sum(wins[p.Record].start > 0 for p in chunked) == 3
    got = consumers(scc, chunked)
    for p, c in zip(chunked, got):
        w = wins[p.Record]
        k = (w.record, w.start + p.Start, w.start + p.End, p.Type)
        assert c == want[k], (k, c, want[k])
    # the refusal: the first product fits the short records, the others end behind them
    L = _lib.lib()
    for sc, prods, was in ((sco, whole, list(want.values())), (scc, chunked, got)):
        n = len(prods)
        ph, nh, sc_out = (_lib.ProbeHit * n)(), (_lib.NestedHit * n)(), (C.c_double * n)()
        offs, need, buf = (C.c_uint64 * (2 * n + 1))(), C.c_uint64(), C.create_string_buffer(2 * n * _lib.IPCR_MAX_PRIMER_LEN)

        def calls(genome):
            return [L.ipcr_probe_products_begin(sc._h, genome._h, probe.encode(), 1),
                    L.ipcr_probe_products_end(sc._h, ph, n),
                    L.ipcr_nested_products(sc._h, genome._h, cpi._h, sci._h, nh, n),
                    L.ipcr_product_sites(sc._h, genome._h, buf, len(buf), offs, n, C.byref(need)),
                    L.ipcr_thermo_legacy_products(sc._h, genome._h, None, 0, sc_out, n)]
        assert calls(small) == [_lib.ERR_INVALID] * 5
        assert calls(g) == [_lib.OK] * 5
        assert [((h.found, h.strand, h.pos, h.mm), bits(x)) for h, x in zip(ph, sc_out)] == [(c[0], c[3]) for c in was]
        assert [bool(h.found) for h in nh] == [c[1][0] for c in was]
    g.close()
    small.close()


# ---------------------------------------------------------------- the driver

def run_cli(argv, env=None, monkeypatch=None):
    from ipcr_amd import thermo_cli
    out, err = io.StringIO(), io.StringIO()
    rc_ = thermo_cli.run(argv, out, err)
    return rc_, out.getvalue(), err.getvalue()


def test_reference_known_answer_byte_for_byte(tmp_path, monkeypatch):
    """TestThermo_ExplicitLegacyModelGoldenOutput (internal/thermointegration/denom_subtests_test.go:117-142)"""
    monkeypatch.chdir(tmp_path)
    (tmp_path / CLI["fasta_name"]).write_text(CLI["fasta"])
    argv = [CLI["fasta_name"] if a == "{fasta}" else a for a in CLI["argv"]]
    assert "--thermo-model" in argv                                     # given, as in the fixture's argv
    rc_, out, err = run_cli(argv)
    assert (rc_, out) == (CLI["exit"], CLI["stdout"]), err
    assert "-18.975" in out and "-29.625" in out


def first_score(text):
    lines = text.strip().split("\n")
    col = lines[0].split("\t").index("score")
    return float(lines[1].split("\t")[col])


def test_denom_subtests(tmp_path, monkeypatch):
    """TestThermo_DenomMode_Subtests (denom_subtests_test.go:58-115), as relations"""
    d = LIT["denom_subtests"]
    monkeypatch.chdir(tmp_path)
    (tmp_path / d["fasta_name"]).write_text(d["fasta"])
    base = [d["fasta_name"] if a == "{fasta}" else a for a in d["argv"]]

    def score(extra):
        rc_, out, err = run_cli(base + extra)
        assert rc_ == 0, err
        return first_score(out)
    fixed, auto = score([]), score(d["auto"])
    assert fixed != auto
    assert score(d["low"]) == score(d["high"]) == fixed                 # fixed ignores the solution
    assert score(d["auto"] + d["low"]) != score(d["auto"] + d["high"])  # auto follows it
    assert score(["--allow-indel"]) == fixed


@pytest.fixture(scope="module")
def fasta_case(tmp_path_factory):
    plan = Plan(seed=6)
    recs = plan.records()
    d = tmp_path_factory.mktemp("thermo_cli")
    path = d / "g.fa"
    with open(path, "wb") as fh:
        for i, s in enumerate(recs):
            fh.write(b">r%d some text\n" % i)
            for j in range(0, len(s), 70):
                fh.write(s[j:j + 70] + b"\n")
    tsv = d / "panel.tsv"
    tsv.write_text("".join(f"{p.ID}\t{p.Forward}\t{p.Reverse}\n" for p in plan.pairs))
    return plan, recs, str(path), str(tsv)


def cli_args(path, tsv, *extra):
    return ["--thermo-model", "legacy-heuristic", "--primers", tsv, "-m", "3", "--terminal-window", "0", "--max-length", "400",
            "--self=false", *extra, path]


def test_three_data_paths_give_the_same_rows(fasta_case, monkeypatch):
    plan, recs, path, tsv = fasta_case
    for fmt in ("text", "jsonl", "fasta"):
        for den in ("fixed", "auto"):
            rc0, whole, err = run_cli(cli_args(path, tsv, "--output", fmt, "--denom", den))
            assert rc0 == 0 and whole.count("\n") > 20, err
            rc1, chunked, _ = run_cli(cli_args(path, tsv, "--output", fmt, "--denom", den, "--chunk-size", "5000"))
            monkeypatch.setenv("IPCR_CLI_STREAM_CHUNKS", "1")
            rc2, streamed, _ = run_cli(cli_args(path, tsv, "--output", fmt, "--denom", den, "--chunk-size", "5000"))
            monkeypatch.delenv("IPCR_CLI_STREAM_CHUNKS")
            assert (rc1, rc2) == (0, 0)
            assert chunked == whole and streamed == whole, (fmt, den)


def test_cli_rows_carry_the_restated_scores_in_rank_order(fasta_case):
    from ipcr_amd import thermo
    plan, recs, path, tsv = fasta_case
    _, out, _ = run_cli(cli_args(path, tsv))
    rows = [ln.split("\t") for ln in out.strip().split("\n")]
    assert rows[0][-1] == "score" and len(rows) > 20
    ids = {"r%d" % i: i for i in range(len(recs))}
    pid = {p.ID: p for p in plan.pairs}
    scores = []
    for r in rows[1:]:
        rec, pair, start, end, typ = recs[ids[r[1]]], pid[r[2]], int(r[3]), int(r[4]), r[6]
        f, v = (pair.Forward, pair.Reverse) if typ == "forward" else (pair.Reverse, pair.Forward)
        want = R.product_score(rec, start, end, f, v, 200.0, 200.0, TRIP)
        assert r[-1] == thermo.go_g(want), r
        scores.append(want)
    assert scores == sorted(scores, reverse=True) and "-0" in {r[-1] for r in rows[1:]}
    # --rank coord: the same rows in coordinate order
    _, coord, _ = run_cli(cli_args(path, tsv, "--rank", "coord"))
    crow = coord.strip().split("\n")
    assert crow[0] == out.split("\n")[0] and sorted(crow[1:]) == sorted(out.strip().split("\n")[1:]) and crow != out.strip().split("\n")
    keys = [(r.split("\t")[1], int(r.split("\t")[3]), int(r.split("\t")[4])) for r in crow[1:]]
    assert keys == sorted(keys)
    # jsonl: seq is the amplicon, score is left out for the zeros
    _, jl, _ = run_cli(cli_args(path, tsv, "--output", "jsonl"))
    objs = [json.loads(x) for x in jl.strip().split("\n")]
    assert len(objs) == len(rows) - 1
    for o, want in zip(objs, scores):
        assert o["seq"] == recs[ids[o["sequence_id"]]][o["start"]:o["end"]].decode()
        assert o.get("score", 0.0) == want
        assert ("score" in o) == (want != 0)


def test_no_products_exit_code(tmp_path):
    fa = tmp_path / "n.fa"
    fa.write_text(">s\nACGTACGTACGTACGTACGTACGTACGT\n")
    rc_, out, _ = run_cli(["--thermo-model", "legacy-heuristic", "-f", "GGGGGGGGGGGGGGGG", "-r", "CCCCCCCCCCCCCCCCC",
                           "--no-match-exit-code", "7", str(fa)])
    assert rc_ == 7 and out.strip().endswith("score")
