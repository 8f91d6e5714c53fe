"""Short sites from resident genomes: ipcr_genome_read_sites (exact bytes, reverse complement on the device),
ipcr_product_sites and NeedSites on ScanGenome / ScanGenomeChunked.  Every expected byte is a Python slice of the records
this file made, complemented with the table written here (core/primer/rc.go:8-24) -- never something the library gave."""
import ctypes
import random
import re
import threading

import pytest

pytestmark = pytest.mark.gpu

COL = 4096
COMP = {ord(a): ord(b) for a, b in zip("ACGTRYSWKMBVDHN", "TGCAYRSWMKVBHDN")}
_TABLE = bytes(COMP.get(b, 0) for b in range(256))
EDGES = (128, 4096, 262144, 524288)                    # strand, column, block, second block
LENGTHS = (1, 4, 20, 33, 128)


def revcomp(b: bytes):
    """reverse complement, or None when a byte has no complement (where RevComp panics, rc.go:28-33)"""
    t = b.translate(_TABLE)[::-1]
    return None if 0 in t else t


def record_cols(n):
    return (n + 128 + 8191) // 8192 * 2


def new_genome(seqs, extra_records=2):
    from ipcr_amd import engine
    return engine.Genome(sum(record_cols(len(s)) for s in seqs) * COL + 4 * 8192, len(seqs) + extra_records)


def make_record(rng, n, raw: bool):
    """n bases: N runs, IUPAC codes (single and in runs) at and around every edge; raw (add_record keeps bytes as
    given): lower case, '-', '*' and 'U' too"""
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    codes = b"RYSWKMBDHVN"
    for k, p in enumerate(range(37, n, 211)):
        s[p] = codes[k % len(codes)]
    for e in (0,) + EDGES + (n,):
        for d in (-3, -1, 0, 2):
            if 0 <= e + d < n:
                s[e + d] = codes[(e + d) % len(codes)]
    if n > 3000:
        s[1000:1040] = b"N" * 40
        s[2000:2010] = b"RRRRRYYYYY"
    if raw:
        for p in range(100, n, 557):
            s[p] = s[p] | 0x20 if s[p] in b"ACGT" else s[p]
        for k, p in enumerate(range(300, n, 1201)):
            s[p] = b"-*U"[k % 3]
        if n > 5000:
            s[4090:4100] = b"acgtacgtac"
    return bytes(s)


def edge_sites(seqs):
    """(record, pos, len, revcomp): every length at position 0, at the record's end and across every edge, forward and
    -- where every byte has a complement -- reversed"""
    out = []
    for r, s in enumerate(seqs):
        n = len(s)
        for ln in LENGTHS:
            if ln > n:
                continue
            starts = {0, n - ln}
            for e in EDGES:
                for p in (e - ln, e - ln // 2, e - 1, e):
                    if 0 <= p and p + ln <= n:
                        starts.add(p)
            for k in range(37, min(n, 3000), 211):       # around the planted codes
                if k - ln // 3 >= 0 and k - ln // 3 + ln <= n:
                    starts.add(k - ln // 3)
            for p in (990, 1030, 1999, 2003, 4085):
                if p + ln <= n:
                    starts.add(p)
            for p in sorted(starts):
                out.append((r, p, ln, 0))
                if revcomp(s[p:p + ln]) is not None:
                    out.append((r, p, ln, 1))
    return out


def random_sites(seqs, rng, count):
    out = []
    for _ in range(count):
        r = rng.randrange(len(seqs))
        n = len(seqs[r])
        ln = rng.randint(1, min(128, n))
        p = rng.randrange(n - ln + 1)
        rc = rng.random() < 0.5 and revcomp(seqs[r][p:p + ln]) is not None
        out.append((r, p, ln, 1 if rc else 0))
    return out


def want_of(seqs, sites):
    return [revcomp(seqs[r][p:p + ln]) if rc else seqs[r][p:p + ln] for r, p, ln, rc in sites]


def check_sites(g, seqs, sites, what):
    got = g.read_sites(sites)
    want = want_of(seqs, sites)
    assert len(got) == len(want)
    bad = [(sites[i], got[i], want[i]) for i in range(len(sites)) if got[i] != want[i]]
    assert not bad, (what, len(bad), bad[:3])


def write_fasta(path, seqs, width=60):
    with open(path, "wb") as fh:
        for i, s in enumerate(seqs):
            fh.write(b">r%d desc\n" % i)
            for j in range(0, len(s), width):
                fh.write(s[j:j + width] + b"\n")


SIZES = (1, 130, 300, 9000, 600_000)


@pytest.fixture(params=["add_record", "fasta_hostpack", "fasta_device"])
def loaded(request, tmp_path, monkeypatch):
    """the same kind of records through the three tile writers"""
    rng = random.Random(11)
    raw = request.param == "add_record"
    seqs = [make_record(rng, n, raw) for n in SIZES]
    g = new_genome(seqs)
    if raw:
        for i, s in enumerate(seqs):
            g.add_record("r%d" % i, s)
    else:
        if request.param == "fasta_device":
            monkeypatch.setenv("IPCR_FASTA_HOSTPACK", "0")
            monkeypatch.setenv("IPCR_FASTA_SLAB", "64")
        write_fasta(tmp_path / "g.fa", seqs)
        assert g.add_fasta(str(tmp_path / "g.fa")) == len(seqs)
    yield g, seqs, request.param
    g.close()


# ---- 6. exact bytes

def test_edge_sites(loaded):
    g, seqs, how = loaded
    sites = edge_sites(seqs)
    assert {ln for _, _, ln, _ in sites} == set(LENGTHS)
    want = want_of(seqs, sites)
    assert any(rc and set(w) & set(b"RYKMBVDHSW") for (_, _, _, rc), w in zip(sites, want)), "no IUPAC byte complemented"
    assert any(b"N" in w for w in want)
    if how == "add_record":
        assert any(not rc and (set(w) & set(b"acgt")) for (_, _, _, rc), w in zip(sites, want))
        assert any(not rc and b"-" in w for (_, _, _, rc), w in zip(sites, want))
    for e in EDGES:                                     # a site of every length across every edge of the long record
        for ln in LENGTHS[1:]:
            assert any(r == 4 and p < e < p + ln and l2 == ln for r, p, l2, _ in sites), (e, ln)
    check_sites(g, seqs, sites, how)
    assert g.read_sites([]) == []


def test_random_sites_one_call_and_in_pieces(loaded, monkeypatch):
    g, seqs, how = loaded
    sites = random_sites(seqs, random.Random(12), 100_000)
    assert sum(rc for _, _, _, rc in sites) > 10_000
    check_sites(g, seqs, sites, how)
    monkeypatch.setenv("IPCR_TEST_SITE_PIECE", "7001")  # 15 launches, the last one short
    check_sites(g, seqs, sites, how + ", pieces of 7001 sites")


def test_genome_without_runs_and_plain_acgt():
    rng = random.Random(13)
    s = bytearray(rng.choice(b"ACGT") for _ in range(300_000))
    s[1000:2000] = b"N" * 1000
    s = bytes(s)
    g = new_genome([s])
    g.add_record("r", s)
    assert g.exception_runs == 0
    check_sites(g, [s], edge_sites([s]) + random_sites([s], rng, 5000), "no runs")
    g.close()


# ---- 7. errors

def _raw_call(g, sites, cap):
    from ipcr_amd import _lib
    n = len(sites)
    arr = (_lib.Site * max(n, 1))()
    for i, (r, p, ln, rc) in enumerate(sites):
        arr[i].record, arr[i].pos, arr[i].len, arr[i].revcomp = r, p, ln, rc
    offs = (ctypes.c_uint64 * (n + 1))(*([0xDEAD] * (n + 1)))
    need = ctypes.c_uint64(0xDEAD)
    buf = ctypes.create_string_buffer(max(cap, 1))
    st = _lib.lib().ipcr_genome_read_sites(g._h, arr, n, buf, cap, offs, ctypes.byref(need))
    return st, list(offs), need.value, buf.raw[:cap]


def test_errors():
    from ipcr_amd import _lib
    s = make_record(random.Random(14), 5000, raw=True)
    g = new_genome([s])
    g.add_record("r", s)
    sites = [(0, 10, 100, 0), (0, 4990, 10, 0), (0, 500, 20, 1)]
    assert revcomp(s[500:520]) is not None
    st, offs, need, _ = _raw_call(g, sites, 50)
    assert (st, offs, need) == (_lib.ERR_CAPACITY, [0, 100, 110, 130], 130)
    st, offs, need, out = _raw_call(g, sites, 130)
    assert (st, offs, need) == (_lib.OK, [0, 100, 110, 130], 130)
    assert out == s[10:110] + s[4990:] + revcomp(s[500:520])
    for bad in ((0, 4990, 11, 0), (0, 5000, 1, 0), (1, 0, 1, 0), (-1, 0, 1, 0), (0, -1, 3, 0), (0, 10, 0, 0), (0, 10, 129, 0),
                (0, 10, 129, 1)):
        st, _, _, _ = _raw_call(g, [sites[0], bad], 400)
        assert st == _lib.ERR_INVALID, bad
    assert _raw_call(g, [], 0)[0] == _lib.OK
    assert _lib.lib().ipcr_genome_read_sites(g._h, None, 0, None, 0, None, None) == _lib.ERR_INVALID
    g.close()


@pytest.mark.parametrize("byte", [b"-", b"a", b"U", b"*"])
def test_revcomp_of_a_byte_without_complement(byte, monkeypatch):
    from ipcr_amd import _lib
    rng = random.Random(15)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in (3000, 9000)]
    s1 = bytearray(seqs[1])
    s1[4100:4101] = byte                                 # the first offender of site 5, in the record's direction
    s1[4103:4104] = b"-"
    s1[7000:7001] = byte                                 # inside site 9 as well: site 5 is named
    seqs[1] = bytes(s1)
    g = new_genome(seqs)
    for i, s in enumerate(seqs):
        g.add_record("r%d" % i, s)
    sites = [(0, 10 * i, 20, i & 1) for i in range(5)] + [(1, 4090, 20, 1)] + [(1, 100 * i, 30, 1) for i in range(3)] + \
            [(1, 6990, 20, 1)]
    forward = [(r, p, ln, 0) for r, p, ln, _ in sites]
    check_sites(g, seqs, forward, "forward over " + repr(byte))   # forward the byte is just a byte
    for piece in ("", "2"):
        monkeypatch.setenv("IPCR_TEST_SITE_PIECE", piece)
        with pytest.raises(_lib.IpcrError) as e:
            g.read_sites(sites)
        assert e.value.status == _lib.ERR_PRIMER
        m = re.search(r"site (\d+) \(record (\d+), position (\d+)\): byte 0x([0-9a-f]{2})", e.value.message)
        assert m, e.value.message
        assert [int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4), 16)] == [5, 1, 4100, byte[0]], e.value.message
    g.close()


def _primers_from(s: bytes, a: int, b: int, n: int = 20):
    """a pair whose forward product is s[a:b]"""
    return s[a:a + n].decode(), revcomp(s[b - n:b]).decode()


def test_dropped_runs_unsupported_and_the_batch_falls_back(monkeypatch, tmp_path):
    from ipcr_amd import _lib, engine, pipeline, primer
    rng = random.Random(16)
    s = bytearray(rng.choice(b"ACGT") for _ in range(300_000))
    for p in range(5000, 300_000, 50):
        s[p] = ord("R")
    s[1010] = ord("Y")                                   # inside the forward site: one mismatch
    s = bytes(s)
    clean = bytearray(s)
    clean[1010] = ord("A")
    fw, rv = _primers_from(bytes(clean), 1000, 3021)
    write_fasta(tmp_path / "g.fa", [s])
    monkeypatch.setenv("IPCR_TEST_EXCEPTION_MAX", "100")
    g = new_genome([s])
    assert g.add_fasta(str(tmp_path / "g.fa")) == 1
    with pytest.raises(_lib.IpcrError) as e:
        g.read_sites([(0, 0, 10, 0)])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    eng = engine.New(engine.Config(MaxMM=1, TerminalWindow=0, MinLen=10, MaxLen=5000, HitCap=0, SeedLen=12, NeedSites=True))
    cp = eng.CompilePanel([primer.Pair("p", fw, rv, 10, 5000)])
    sc = eng.NewSimulationScratch(cp)
    with pytest.raises(_lib.IpcrError) as e:
        eng.ScanGenome(g, cp, sc)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    prods = eng.ScanGenome(g, cp, sc, sites=False)
    assert [(p.Start, p.End) for p in prods] == [(1000, 3021)] and prods[0].FwdSite == ""
    b = pipeline.Batch(prods, sc, g, None, path=str(tmp_path / "g.fa"))
    assert b.sites() == [(s[1000:1020].decode(), revcomp(s[3001:3021]).decode())]
    assert "Y" in b.sites()[0][0]
    g.close()


# ---- 8. NeedSites on the resident scans

F, R = "ACGTTGCATGCAAGCTTAGC", "GGCCTTAAGGCCATATCGTATG"          # 20 and 22 nt: the two sites differ in length


def _rc(s: str) -> str:
    return revcomp(s.encode()).decode()


def planted_records(rng):
    """forward and revcomp products, sites with a substituted base, with an N and with an IUPAC byte inside, one pair of
    sites across the origin of a short record"""
    a = bytearray(rng.choice(b"ACGT") for _ in range(20_000))
    a[1000:1020] = F.encode(); a[1300:1322] = _rc(R).encode()                     # forward
    a[5000:5022] = R.encode(); a[5400:5420] = _rc(F).encode()                     # revcomp
    a[8000:8020] = F.encode(); a[8200:8222] = _rc(R).encode()
    a[8004] = ord("N"); a[8210] = ord("R")                                         # N / IUPAC byte inside the sites
    a[12000:12020] = F.encode(); a[12500:12522] = _rc(R).encode()
    a[12003] = ord("A") if a[12003] != ord("A") else ord("C")                      # substitutions
    a[12515] = ord("A") if a[12515] != ord("A") else ord("C")
    a[4090:4110] = F.encode(); a[4300:4322] = _rc(R).encode()                      # a site across a column edge
    b = bytearray(rng.choice(b"ACGT") for _ in range(3000))
    b[2900:2920] = F.encode(); b[50:72] = _rc(R).encode()                          # across the origin when circular
    b[2910] = ord("K")
    c = bytearray(rng.choice(b"ACGT") for _ in range(9000))
    c[7000:7022] = R.encode(); c[7700:7720] = _rc(F).encode()
    return [("chrA", bytes(a)), ("plasmid", bytes(b)), ("chrC", bytes(c))]


def own_sites(rec: bytes, p):
    """(FwdSite, RevSite) in record coordinates: engine.go:177-185"""
    return (rec[p.Start:p.Start + len(p.FwdPrimer)].decode(),
            revcomp(rec[p.End - len(p.RevPrimer):p.End]).decode())


def load(recs):
    g = new_genome([s for _, s in recs])
    for name, s in recs:
        g.add_record(name, s)
    return g


def test_scan_genome_need_sites():
    from ipcr_amd import engine, primer
    recs = planted_records(random.Random(17))
    by_id = dict(recs)
    g = load(recs)
    for circular in (False, True):
        cfg = dict(MaxMM=2, TerminalWindow=0, MinLen=10, MaxLen=1000, HitCap=0, SeedLen=12, Circular=circular)
        eng = engine.New(engine.Config(NeedSites=True, **cfg))
        cp = eng.CompilePanel([primer.Pair("p", F, R, 10, 1000)])
        sc = eng.NewSimulationScratch(cp)
        prods = eng.ScanGenome(g, cp, sc)
        assert len(prods) >= 6
        for p in prods:
            assert (p.FwdSite, p.RevSite) == own_sites(by_id[p.SequenceID], p), p
            assert (len(p.FwdSite), len(p.RevSite)) == ((20, 22) if p.Type == "forward" else (22, 20))
        assert {p.Type for p in prods} == {"forward", "revcomp"}
        assert any(p.FwdMM and "N" in p.FwdSite for p in prods) and any(p.RevMM and "Y" in p.RevSite for p in prods)
        assert any(p.FwdMM and p.RevMM and set(p.FwdSite + p.RevSite) <= set("ACGT") for p in prods)
        wrap = [p for p in prods if p.Start > p.End]
        assert bool(wrap) == circular
        if circular:
            assert wrap[0].SequenceID == "plasmid" and "K" in wrap[0].FwdSite
        # the untouched chunk path fills the same strings for the same record
        for name, s in recs:
            chunk = eng.SimulateCompiledWithScratch(name, s, cp, eng.NewSimulationScratch(cp))
            assert [(p.sig(), p.FwdSite, p.RevSite) for p in chunk] == \
                [(p.sig(), p.FwdSite, p.RevSite) for p in prods if p.SequenceID == name]
        # without NeedSites: the same products, no sites, no extra call
        eng0 = engine.New(engine.Config(**cfg))
        cp0 = eng0.CompilePanel([primer.Pair("p", F, R, 10, 1000)])
        plain = eng0.ScanGenome(g, cp0, eng0.NewSimulationScratch(cp0))
        assert [p.sig() for p in plain] == [p.sig() for p in prods]
        assert all(p.FwdSite == "" and p.RevSite == "" for p in plain)
    g.close()


def test_scan_genome_chunked_need_sites():
    from ipcr_amd import cli, engine, primer
    recs = planted_records(random.Random(18))
    by_id = dict(recs)
    g = load(recs)
    eng = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=10, MaxLen=1000, HitCap=0, SeedLen=12, NeedSites=True))
    cp = eng.CompilePanel([primer.Pair("p", F, R, 10, 1000)])
    sc = eng.NewSimulationScratch(cp)
    whole = {(p.SequenceID, p.Start, p.End, p.Type): (p.FwdSite, p.RevSite) for p in eng.ScanGenome(g, cp, sc)}
    chunked = eng.ScanGenomeChunked(g, cp, sc, 4000, 1000)
    assert any(":" in p.SequenceID for p in chunked)
    seen = {}
    for p in chunked:
        base, off, ok = cli.split_chunk_suffix(p.SequenceID)
        rec = by_id[base]
        assert p.FwdSite == rec[off + p.Start:off + p.Start + len(p.FwdPrimer)].decode(), p
        assert p.RevSite == revcomp(rec[off + p.End - len(p.RevPrimer):off + p.End]).decode(), p
        seen[(base, off + p.Start, off + p.End, p.Type)] = (p.FwdSite, p.RevSite)
    assert seen == whole
    eng0 = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=10, MaxLen=1000, HitCap=0, SeedLen=12))
    cp0 = eng0.CompilePanel([primer.Pair("p", F, R, 10, 1000)])
    plain = eng0.ScanGenomeChunked(g, cp0, eng0.NewSimulationScratch(cp0), 4000, 1000)
    assert len(plain) == len(chunked) and all(p.FwdSite == "" and p.RevSite == "" for p in plain)
    g.close()


def test_reference_literal_through_scan_genome():
    """the literal of core/engine's NeedSites test (tests/test_gpu_parity.py::test_need_sites) over a resident genome"""
    from ipcr_amd import engine, primer
    seq = b"TTTTCGTACAAAAGGTACCTTT"
    g = new_genome([seq])
    g.add_record("seq", seq)
    eng = engine.New(engine.Config(MaxMM=1, TerminalWindow=3, MinLen=1, MaxLen=100, SeedLen=12, NeedSites=True))
    cp = eng.CompilePanel([primer.Pair("x", "ACGTAC", "GGTACC")])
    sc = eng.NewSimulationScratch(cp)
    by = {(p.Type, p.Start): p for p in eng.ScanGenome(g, cp, sc)}
    f = by[("forward", 3)]
    assert (f.FwdPrimer, f.RevPrimer, f.FwdSite, f.RevSite) == ("ACGTAC", "GGTACC", "TCGTAC", "GGTACC")
    r = by[("revcomp", 13)]
    assert (r.FwdPrimer, r.RevPrimer, r.FwdSite, r.RevSite) == ("GGTACC", "ACGTAC", "GGTACC", "AGGTAC")
    assert sc.product_sites(g) == [(p.FwdSite, p.RevSite) for p in eng.ScanGenome(g, cp, sc)]
    g.close()


def test_product_sites_errors():
    from ipcr_amd import _lib, engine, primer
    seq = b"TTTTCGTACAAAAGGTACCTTT"
    g = new_genome([seq])
    g.add_record("seq", seq)
    eng = engine.New(engine.Config(MaxMM=1, TerminalWindow=3, MinLen=1, MaxLen=100, SeedLen=12))
    cp = eng.CompilePanel([primer.Pair("x", "ACGTAC", "GGTACC")])
    sc = eng.NewSimulationScratch(cp)
    n = len(eng.ScanGenome(g, cp, sc))
    assert n >= 2
    offs = (ctypes.c_uint64 * (2 * n + 1))()
    need = ctypes.c_uint64()
    buf = ctypes.create_string_buffer(256 * n)
    lib = _lib.lib()
    assert lib.ipcr_product_sites(sc._h, g._h, buf, 256 * n, offs, n - 1, ctypes.byref(need)) == _lib.ERR_INVALID
    assert lib.ipcr_product_sites(sc._h, g._h, buf, 5, offs, n, ctypes.byref(need)) == _lib.ERR_CAPACITY
    assert need.value == 12 * n and list(offs) == [6 * i for i in range(2 * n + 1)]
    assert lib.ipcr_product_sites(sc._h, g._h, buf, 256 * n, offs, n, ctypes.byref(need)) == _lib.OK
    eng.SimulateCompiledWithScratch("seq", seq, cp, sc)  # the products now lie in the scratch's own chunk
    assert lib.ipcr_product_sites(sc._h, g._h, buf, 256 * n, offs, sc.num_products(), ctypes.byref(need)) == _lib.ERR_INVALID
    g.close()


# ---- 9. threads

def test_eight_threads_read_sites_while_the_genome_is_scanned():
    from ipcr_amd import engine, primer
    rng = random.Random(19)
    seqs = [make_record(rng, 300_000, raw=True) for _ in range(2)]
    g = new_genome(seqs)
    for i, s in enumerate(seqs):
        g.add_record("r%d" % i, s)
    sites = random_sites(seqs, rng, 20_000)
    want = want_of(seqs, sites)
    eng = engine.New(engine.Config(MaxMM=2, TerminalWindow=0, MinLen=10, MaxLen=3000, HitCap=0, SeedLen=12))
    cp = eng.CompilePanel([primer.Pair("p", "ACGTACGTACGTACGTAC", "TTGCATTGCATTGCATTG", 10, 3000)])
    sc = eng.NewSimulationScratch(cp)
    first = [p.sig() for p in eng.ScanGenome(g, cp, sc)]
    assert g.read_sites(sites) == want
    results, errs = [None] * 8, []

    def reader(k):
        try:
            results[k] = all(g.read_sites(sites) == want for _ in range(3))
        except Exception as e:  # pragma: no cover - reported below
            errs.append(e)

    ts = [threading.Thread(target=reader, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    scans = [[p.sig() for p in eng.ScanGenome(g, cp, sc)] for _ in range(3)]
    for t in ts:
        t.join()
    assert not errs and results == [True] * 8
    assert scans == [first] * 3
    g.close()
